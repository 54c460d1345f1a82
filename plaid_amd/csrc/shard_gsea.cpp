// plaid.gsea, its multilevel p-values and one ruler on the sharded engine (shard.cpp).
#include "shard.h"

namespace plaidhip {

namespace {

// ---- plaid.gsea's multilevel chains (kernels_gsea_ml.hip; include/plaidhip.h: plaidhip_gsea_multilevel) -------------------------
// what the rulers leave: per set (in the rulers' set order) the read-off stage, count and status; per ruler its stages, end
// status and the trace of counts and levels ([ruler][PLAIDHIP_GSEA_ML_MAX_STAGES])
struct GseaMlResult {
  std::vector<int32_t> lstar, cnt, est, s_trace, nstages, end;
  std::vector<double> m_trace;
};

constexpr size_t kGseaMlBatchBytes = (size_t)1 << 30;   // ruler state one batch of rulers keeps on the device, at most

// Runs `rulers` (their set0 / nset index `gamma`) to their ends, batch by batch; a host loop advances a batch one stage per
// launch pair and reads one counter back, so no launch outlasts one stage.  h_out (nullable, one ruler): every stage's scores.
int gsea_ml_run(plaidhip_ctx* ctx, int weighted, int score_type, const double* dWpos, int32_t g,
                const std::vector<GseaMlRuler>& rulers, const std::vector<double>& gamma, int32_t n, int32_t sweeps, double eps,
                uint64_t seed, double* h_out, GseaMlResult& res) {
  constexpr int32_t S = PLAIDHIP_GSEA_ML_MAX_STAGES;
  const size_t nr_all = rulers.size(), nset_all = gamma.size();
  res.lstar.assign(nset_all, -1);
  res.cnt.assign(nset_all, 0);
  res.est.assign(nset_all, 0);
  res.s_trace.assign(nr_all * S, 0);
  res.m_trace.assign(nr_all * S, 0.0);
  res.nstages.assign(nr_all, 0);
  res.end.assign(nr_all, 0);
  if (nr_all == 0) return PLAIDHIP_OK;
  const int32_t nwg = gsea_ml_map_words(g);
  const size_t per_ruler = (size_t)n * nwg * 8 + (size_t)n * 8 + (size_t)S * 12 + sizeof(GseaMlState) + sizeof(GseaMlRuler);
  const size_t batch = std::max<size_t>(1, std::min<size_t>(nr_all, kGseaMlBatchBytes / per_ruler));
  DevBuf dru, dst, dmaps, dH, dstr, dmtr, dhtr, dgam, dls, dcn, des, dcount;
  PH_TRY(dru.alloc(batch * sizeof(GseaMlRuler)));
  PH_TRY(dst.alloc(batch * sizeof(GseaMlState)));
  PH_TRY(dmaps.alloc(batch * n * nwg * 8));
  PH_TRY(dH.alloc(batch * n * 8));
  PH_TRY(dstr.alloc(batch * S * 4));
  PH_TRY(dmtr.alloc(batch * S * 8));
  if (h_out != nullptr) PH_TRY(dhtr.alloc(batch * S * n * 8));
  PH_TRY(dcount.alloc(4));
  size_t max_nq = 1;   // the sets of the largest batch
  for (size_t r0 = 0; r0 < nr_all; r0 += batch) {
    const size_t r1 = std::min(nr_all, r0 + batch);
    max_nq = std::max(max_nq, (size_t)(rulers[r1 - 1].set0 + rulers[r1 - 1].nset - rulers[r0].set0));
  }
  PH_TRY(dgam.alloc(max_nq * 8));
  PH_TRY(dls.alloc(max_nq * 4));
  PH_TRY(dcn.alloc(max_nq * 4));
  PH_TRY(des.alloc(max_nq * 4));
  std::vector<GseaMlRuler> hr;
  std::vector<GseaMlState> hs;
  for (size_t r0 = 0; r0 < nr_all; r0 += batch) {
    const size_t r1 = std::min(nr_all, r0 + batch);
    const int32_t nr = (int32_t)(r1 - r0);
    const int32_t q0 = rulers[r0].set0, q1 = rulers[r1 - 1].set0 + rulers[r1 - 1].nset, nq = q1 - q0;
    hr.assign(rulers.begin() + (ptrdiff_t)r0, rulers.begin() + (ptrdiff_t)r1);
    for (GseaMlRuler& r : hr) r.set0 -= q0;
    GseaMlState fresh{};
    fresh.P = 1.0;
    hs.assign((size_t)nr, fresh);
    PH_HIP(hipMemcpyAsync(dru.p, hr.data(), (size_t)nr * sizeof(GseaMlRuler), hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemcpyAsync(dst.p, hs.data(), (size_t)nr * sizeof(GseaMlState), hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemcpyAsync(dgam.p, gamma.data() + q0, (size_t)nq * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemsetAsync(dls.p, 0xff, (size_t)nq * 4, ctx->stream));
    PH_HIP(hipMemsetAsync(dcn.p, 0, (size_t)nq * 4, ctx->stream));
    PH_HIP(hipMemsetAsync(des.p, 0, (size_t)nq * 4, ctx->stream));
    PH_HIP(hipMemsetAsync(dstr.p, 0, (size_t)nr * S * 4, ctx->stream));
    PH_HIP(hipMemsetAsync(dmtr.p, 0, (size_t)nr * S * 8, ctx->stream));
    if (h_out != nullptr) PH_HIP(hipMemsetAsync(dhtr.p, 0, (size_t)nr * S * n * 8, ctx->stream));
    PH_TRY(launch_gsea_ml_init(ctx, weighted, score_type, dru.as<GseaMlRuler>(), nr, n, g, dWpos, seed,
                               dmaps.as<unsigned long long>(), dH.as<double>()));
    for (int32_t stage = 0; stage < S; ++stage) {
      uint32_t unfinished = 0u;
      PH_HIP(hipMemsetAsync(dcount.p, 0, 4, ctx->stream));
      PH_TRY(launch_gsea_ml_stage(ctx, dru.as<GseaMlRuler>(), dst.as<GseaMlState>(), nr, n, g, eps,
                                  dmaps.as<unsigned long long>(), dH.as<double>(), dstr.as<int32_t>(), dmtr.as<double>(),
                                  h_out != nullptr ? dhtr.as<double>() : nullptr, dgam.as<double>(), dls.as<int32_t>(),
                                  dcn.as<int32_t>(), des.as<int32_t>(), dcount.as<uint32_t>()));
      PH_HIP(hipMemcpyAsync(&unfinished, dcount.p, 4, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      if (unfinished == 0u) break;
      PH_TRY(launch_gsea_ml_mutate(ctx, weighted, score_type, dru.as<GseaMlRuler>(), dst.as<GseaMlState>(), nr, n, g, dWpos, seed,
                                   sweeps, dmaps.as<unsigned long long>(), dH.as<double>()));
    }
    PH_HIP(hipMemcpyAsync(hs.data(), dst.p, (size_t)nr * sizeof(GseaMlState), hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(res.s_trace.data() + r0 * S, dstr.p, (size_t)nr * S * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(res.m_trace.data() + r0 * S, dmtr.p, (size_t)nr * S * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(res.lstar.data() + q0, dls.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(res.cnt.data() + q0, dcn.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(res.est.data() + q0, des.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (h_out != nullptr) PH_HIP(hipMemcpyAsync(h_out, dhtr.p, (size_t)S * n * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    for (int32_t r = 0; r < nr; ++r) {
      PH_REQUIRE(hs[(size_t)r].ended != 0, "gsea_multilevel: a ruler did not end within %d stages", S);
      res.nstages[r0 + (size_t)r] = hs[(size_t)r].stage;
      res.end[r0 + (size_t)r] = hs[(size_t)r].status;
    }
  }
  return PLAIDHIP_OK;
}

// qhat and log2err of a set read off at stage lstar with count cnt, from its ruler's counts (include/plaidhip.h: the order of
// the operations is part of the pinned form)
void gsea_ml_readoff(const int32_t* s_trace, int32_t n, int32_t lstar, int32_t cnt, double* qhat, double* log2err) {
  double P = 1.0, sum = 0.0;
  for (int32_t j = 0; j < lstar; ++j) {
    const int32_t s = s_trace[j];
    P = P * ((double)s / (double)n);
    sum += (double)(n - s) / ((double)n * (double)s);
  }
  const int32_t c1 = cnt > 1 ? cnt : 1;
  *qhat = P * ((double)c1 / (double)n);
  sum += (double)(n - c1) / ((double)n * (double)c1);
  *log2err = std::sqrt(sum) / 0.6931471805599453;   // ln 2
}

// the observed placement and walk-order weights of nl lists already on the device (dstat, dw: g x nl)
int gsea_observed_operands(plaidhip_ctx* ctx, const double* dstat, const double* dw, const uint32_t* dnan, int32_t g, int32_t nl,
                           double* dR, double* dY, double* dQ, int32_t* dpos, double* dWpos) {
  const size_t col = (size_t)g * nl;
  PH_HIP(hipMemsetAsync(dWpos, 0, col * 8, ctx->stream));
  PH_HIP(hipMemsetAsync(dpos, 0, col * 4, ctx->stream));
  PH_TRY(launch_colranks_dense_f64(ctx, dstat, g, g, nl, PLAIDHIP_TIES_MIN, 0, 1.0, dR, g, nullptr));
  PH_TRY(launch_last_ranks(ctx, dense_cols(g, nl, g), dR, dY, dQ));
  return launch_gsea_operands(ctx, dQ, dw, g, dnan, g, nl, dpos, dWpos);
}

}  // namespace

// plaidhip_gsea_ruler: one ruler of one list to the caller's target, and its trace
int gsea_ruler_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    const int32_t g = c.g;
    DevBuf dstat, dw, dR, dY, dQ, dWpos, dpos, dnan;
    for (DevBuf* b : {&dstat, &dw, &dR, &dY, &dQ, &dWpos}) PH_TRY(b->alloc((size_t)g * 8));
    PH_TRY(dpos.alloc((size_t)g * 4));
    PH_TRY(dnan.alloc(4));
    PH_HIP(hipMemcpyAsync(dstat.p, c.X, (size_t)g * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemcpyAsync(dw.p, c.weight, (size_t)g * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemsetAsync(dnan.p, 0, 4, ctx->stream));
    PH_TRY(gsea_observed_operands(ctx, dstat.as<double>(), dw.as<double>(), dnan.as<uint32_t>(), g, 1, dR.as<double>(),
                                  dY.as<double>(), dQ.as<double>(), dpos.as<int32_t>(), dWpos.as<double>()));
    const std::vector<GseaMlRuler> rulers(1, GseaMlRuler{0, c.ml_l, c.ml_side, c.ml_k, 0, 1, c.ml_gamma});
    const std::vector<double> gamma(1, c.ml_gamma);
    GseaMlResult res;
    PH_TRY(gsea_ml_run(ctx, c.gsea_weighted, c.score_type, dWpos.as<double>(), g, rulers, gamma, c.ml_sample, c.ml_sweeps,
                       c.ml_eps, c.seed, c.ml_h, res));
    *c.ml_nstages = res.nstages[0];
    *c.ml_end = res.end[0];
    std::copy(res.m_trace.begin(), res.m_trace.end(), c.ml_m);
    std::copy(res.s_trace.begin(), res.s_trace.end(), c.ml_s);
    return PLAIDHIP_OK;
  });
  return s.finish();
}

namespace {

// the side of a pair's ruler: 0 positive, 1 negative, -1 none (a NaN pair; std with ES == 0)
inline int gsea_ml_side(int score_type, double es) {
  if (es != es) return -1;
  if (score_type == PLAIDHIP_GSEA_POS) return 0;
  if (score_type == PLAIDHIP_GSEA_NEG) return 1;
  return es > 0.0 ? 0 : (es < 0.0 ? 1 : -1);
}

// This shard's rulers of plaid.gsea's multilevel p-values: the ruler list (sorted by list, side and size; the same on every
// shard, from the same observed scores) is shared out in whole rulers, and every set's (qhat, log2err, stage, status) goes
// to sh.gsea.ml[4 (l m + j) ..], which holds NaN for a pair without a ruler.
int gsea_ml_shard(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh, const double* dES, const double* dWpos) {
  const int32_t m = c.m, nl = c.n, n = c.ml_sample;
  std::vector<double> es((size_t)m * nl);
  PH_HIP(hipMemcpyAsync(es.data(), dES, es.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  struct Entry { int32_t l, side, k, j; };
  std::vector<Entry> ent;
  for (int32_t l = 0; l < nl; ++l)
    for (int32_t j = 0; j < m; ++j) {
      const int side = gsea_ml_side(c.score_type, es[(size_t)l * m + j]);
      if (side >= 0) ent.push_back(Entry{l, side, c.Gp[j + 1] - c.Gp[j], j});
    }
  std::stable_sort(ent.begin(), ent.end(), [](const Entry& a, const Entry& b) {
    return a.l != b.l ? a.l < b.l : (a.side != b.side ? a.side < b.side : a.k < b.k);
  });
  std::vector<GseaMlRuler> all;
  for (size_t q = 0; q < ent.size(); ++q) {
    const Entry& e = ent[q];
    const double ga = std::fabs(es[(size_t)e.l * m + e.j]);
    if (all.empty() || all.back().l != e.l || all.back().side != e.side || all.back().k != e.k)
      all.push_back(GseaMlRuler{e.l, e.l, e.side, e.k, (int32_t)q, 0, ga});
    all.back().nset += 1;
    all.back().gmax = std::max(all.back().gmax, ga);
  }
  int64_t lo = 0, hi = 0;
  plaidhip_shard_bounds((int64_t)all.size(), ndev, k, &lo, &hi);
  if (hi <= lo) return PLAIDHIP_OK;
  const int32_t q0 = all[(size_t)lo].set0, q1 = all[(size_t)hi - 1].set0 + all[(size_t)hi - 1].nset;
  std::vector<GseaMlRuler> mine(all.begin() + lo, all.begin() + hi);
  std::vector<double> gamma((size_t)(q1 - q0));
  for (GseaMlRuler& r : mine) r.set0 -= q0;
  for (int32_t q = q0; q < q1; ++q) gamma[(size_t)(q - q0)] = std::fabs(es[(size_t)ent[(size_t)q].l * m + ent[(size_t)q].j]);
  GseaMlResult res;
  PH_TRY(gsea_ml_run(ctx, c.gsea_weighted, c.score_type, dWpos, c.g, mine, gamma, n, c.ml_sweeps, c.ml_eps, c.seed, nullptr, res));
  for (size_t r = 0; r < mine.size(); ++r)
    for (int32_t q = mine[r].set0; q < mine[r].set0 + mine[r].nset; ++q) {
      const Entry& e = ent[(size_t)(q0 + q)];
      PH_REQUIRE(res.lstar[(size_t)q] >= 0, "gsea_multilevel: set %d of list %d was not read off", e.j, e.l);
      double* o = sh.gsea.ml.data() + 4 * ((size_t)e.l * m + e.j);
      gsea_ml_readoff(res.s_trace.data() + r * PLAIDHIP_GSEA_ML_MAX_STAGES, n, res.lstar[(size_t)q], res.cnt[(size_t)q], &o[0], &o[1]);
      o[2] = (double)res.lstar[(size_t)q];
      o[3] = (double)res.est[(size_t)q];
    }
  return PLAIDHIP_OK;
}

}  // namespace

// one device's part of plaid.gsea (kGsea, kernels_gsea.hip).  Every shard holds stat, weight and G and forms the observed
// placements and scores itself (the same bits everywhere); the permutation blocks are shared out in whole blocks
// (plaidhip_shard_bounds over the blocks) and walked slab by slab; the block partials meet on the host in block order and
// shard 0 reduces them once, so every sharding has the one-shard bits.  One rendezvous.
int gsea_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t g = c.g, nl = c.n, m = c.m, B = c.nperm;
  const int32_t nblk = (B + PLAIDHIP_GSEA_PERM_BLOCK - 1) / PLAIDHIP_GSEA_PERM_BLOCK;
  int64_t blo = 0, bhi = 0;
  plaidhip_shard_bounds(nblk, ndev, k, &blo, &bhi);
  const int64_t p_lo = blo * PLAIDHIP_GSEA_PERM_BLOCK, p_hi = std::min<int64_t>(B, bhi * PLAIDHIP_GSEA_PERM_BLOCK);
  const size_t col = (size_t)g * nl, blk_doubles = (size_t)nl * 6 * m;
  DevBuf dstat, dw, dR, dY, dQ, dWpos, dpos, dnan, dGp, dGi, dES, dpart, dslabY, dslabR, dP, dbad, dnull, dout, dall, dlen, didx;
  const int32_t slab = gsea_slab_perms(g);

  // ---- upload, the observed placements and scores -------------------------------------------------------------------------
  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    PH_TRY(dstat.alloc(col * 8));
    PH_TRY(dw.alloc(col * 8));
    PH_TRY(dR.alloc(col * 8));
    PH_TRY(dY.alloc(col * 8));
    PH_TRY(dQ.alloc(col * 8));
    PH_TRY(dWpos.alloc(col * 8));
    PH_TRY(dpos.alloc(col * 4));
    PH_TRY(dnan.alloc((size_t)nl * 4));
    PH_TRY(dES.alloc((size_t)m * nl * 8));
    PH_TRY(upload_pattern(ctx, c.Gp, c.Gi, m, dGp, dGi));
    PH_TRY(upload_pipelined(ctx, dstat.as<char>(), (size_t)g * 8, reinterpret_cast<const char*>(c.X), (size_t)g * 8, nl, nullptr));
    PH_TRY(upload_pipelined(ctx, dw.as<char>(), (size_t)g * 8, reinterpret_cast<const char*>(c.weight), (size_t)g * 8, nl,
                            nullptr));
    PH_HIP(hipMemcpyAsync(dnan.p, c.listnan.data(), (size_t)nl * 4, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(gsea_observed_operands(ctx, dstat.as<double>(), dw.as<double>(), dnan.as<uint32_t>(), g, nl, dR.as<double>(),
                                  dY.as<double>(), dQ.as<double>(), dpos.as<int32_t>(), dWpos.as<double>()));
    return launch_gsea_obs(ctx, c.gsea_weighted, c.score_type, dpos.as<int32_t>(), dWpos.as<double>(), dnan.as<uint32_t>(), g, nl,
                           dGp.as<int32_t>(), dGi.as<int32_t>(), m, dES.as<double>());
  });

  // ---- this shard's blocks of the null, slab by slab ------------------------------------------------------------------------
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (p_hi <= p_lo) return PLAIDHIP_OK;
    const int32_t smax = (int32_t)std::min<int64_t>(slab, p_hi - p_lo);
    PH_TRY(dpart.alloc((size_t)(bhi - blo) * blk_doubles * 8));
    PH_TRY(dP.alloc((size_t)g * smax * 4));
    PH_TRY(dbad.alloc(8));
    PH_HIP(hipMemsetAsync(dbad.p, 0, 8, ctx->stream));
    if (c.perm == nullptr) {
      PH_TRY(dslabY.alloc((size_t)g * smax * 8));
      PH_TRY(dslabR.alloc((size_t)g * smax * 8));
    }
    if (c.null_out != nullptr) PH_TRY(dnull.alloc((size_t)m * smax * nl * 8));
    for (int64_t b0 = p_lo; b0 < p_hi; b0 += slab) {
      const int32_t nbs = (int32_t)std::min<int64_t>(slab, p_hi - b0);
      if (c.perm == nullptr) {
        PH_TRY(launch_gsea_placements(ctx, g, b0, nbs, c.seed, dslabY.as<double>(), dslabR.as<double>(), dP.as<int32_t>()));
      } else {
        PH_TRY(upload_pipelined(ctx, dP.as<char>(), (size_t)g * 4, reinterpret_cast<const char*>(c.perm + b0 * g), (size_t)g * 4,
                                nbs, nullptr));
        PH_TRY(launch_gsea_check_perm(ctx, dP.as<int32_t>(), g, nbs, (int32_t)b0, dbad.as<uint32_t>()));
        uint32_t bad[2] = {0u, 0u};
        PH_HIP(hipMemcpyAsync(bad, dbad.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));
        PH_REQUIRE(bad[0] == 0u, "gsea: column %u of perm is no permutation of 0..%d", bad[1] - 1u, g - 1);
      }
      PH_TRY(launch_gsea_null(ctx, c.gsea_weighted, c.score_type, dP.as<int32_t>(), nbs, dWpos.as<double>(), dnan.as<uint32_t>(),
                              dES.as<double>(), g, nl, dGp.as<int32_t>(), dGi.as<int32_t>(), m, dpart.as<double>(),
                              (b0 - p_lo) / PLAIDHIP_GSEA_PERM_BLOCK, c.null_out != nullptr ? dnull.as<double>() : nullptr));
      if (c.null_out != nullptr)
        for (int32_t l = 0; l < nl; ++l)
          PH_HIP(hipMemcpyAsync(c.null_out + ((int64_t)l * B + b0) * m, dnull.as<double>() + (size_t)l * nbs * m,
                                (size_t)nbs * m * 8, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));   // (the slab's buffers are the next slab's)
    }
    if (ndev > 1) {
      PH_HIP(hipMemcpyAsync(sh.gsea.part.data() + (size_t)blo * blk_doubles, dpart.p, (size_t)(bhi - blo) * blk_doubles * 8,
                            hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PLAIDHIP_OK;
  });
  // ---- multilevel: this shard's rulers, on the observed placements it already holds ---------------------------------------
  if (c.method == kGseaMultilevel)
    s.step([&]() -> int { return gsea_ml_shard(ctx, c, ndev, k, sh, dES.as<double>(), dWpos.as<double>()); });
  sh.rv.arrive_and_wait();

  // ---- shard 0: the blocks in order, NES and pval; padj on the host ---------------------------------------------------------
  if (k == 0)
    s.step([&]() -> int {
      const double* part = dpart.as<double>();
      if (ndev > 1) {
        PH_TRY(dall.alloc((size_t)nblk * blk_doubles * 8));
        PH_HIP(hipMemcpyAsync(dall.p, sh.gsea.part.data(), (size_t)nblk * blk_doubles * 8, hipMemcpyHostToDevice, ctx->stream));
        part = dall.as<double>();
      }
      PH_TRY(dout.alloc((size_t)m * 12 * nl * 8));
      PH_TRY(launch_gsea_null_reduce(ctx, part, nblk, dES.as<double>(), dGp.as<int32_t>(), m, nl, c.score_type,
                                     dout.as<double>()));
      PH_HIP(hipMemcpyAsync(c.out, dout.p, (size_t)m * 12 * nl * 8, hipMemcpyDeviceToHost, ctx->stream));
      if (c.le_len != nullptr) {   // the leading edges, once, on the observed placements this shard already holds
        const size_t nnz = (size_t)c.Gp[m];
        PH_TRY(dlen.alloc((size_t)m * nl * 4));
        PH_TRY(didx.alloc(nnz * nl * 4));
        PH_TRY(launch_gsea_edges(ctx, c.gsea_weighted, c.score_type, dpos.as<int32_t>(), dWpos.as<double>(), dnan.as<uint32_t>(),
                                 g, nl, dGp.as<int32_t>(), dGi.as<int32_t>(), m, dlen.as<int32_t>(), didx.as<int32_t>()));
        PH_HIP(hipMemcpyAsync(c.le_len, dlen.p, (size_t)m * nl * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (nnz != 0) PH_HIP(hipMemcpyAsync(c.le_idx, didx.p, nnz * nl * 4, hipMemcpyDeviceToHost, ctx->stream));
      }
      PH_HIP(hipStreamSynchronize(ctx->stream));
      if (c.method == kGseaMultilevel) {   // the multilevel table, and the reported pval where the permutations saw too few
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const size_t mm = (size_t)m;
        for (int32_t l = 0; l < nl; ++l)
          for (int32_t j = 0; j < m; ++j) {
            double* o = c.out + (size_t)l * 12 * mm + j;
            double* q = c.ml_out + (size_t)l * 6 * mm + j;
            const double* r = sh.gsea.ml.data() + 4 * ((size_t)l * mm + j);
            const int side = gsea_ml_side(c.score_type, o[0]);
            if (side < 0 || r[0] != r[0]) {
              for (int t = 0; t < 6; ++t) q[t * mm] = nan;
              continue;
            }
            const double denom = (1.0 + o[(side == 0 ? 8 : 9) * mm]) / (1.0 + (double)B);
            const double ratio = r[0] / denom;
            q[0] = ratio < 1.0 ? ratio : 1.0;
            q[mm] = r[1];
            q[2 * mm] = r[2];
            q[3 * mm] = r[3];
            q[4 * mm] = r[0];
            q[5 * mm] = denom;
            if (o[4 * mm] < (double)c.ml_min) o[2 * mm] = q[0];
          }
      }
      std::vector<double> p, q;
      std::vector<int32_t> at;
      for (int32_t l = 0; l < nl; ++l) {   // Benjamini-Hochberg over the sets of the list that have a p-value
        double* o = c.out + (size_t)l * 12 * m;
        p.clear();
        at.clear();
        for (int32_t j = 0; j < m; ++j)
          if (o[2 * (size_t)m + j] == o[2 * (size_t)m + j]) { p.push_back(o[2 * (size_t)m + j]); at.push_back(j); }
        q.resize(p.size());
        if (!p.empty()) p_adjust_fdr(p.data(), (int64_t)p.size(), q.data());
        for (size_t e = 0; e < p.size(); ++e) o[3 * (size_t)m + at[e]] = q[e];
      }
      return PLAIDHIP_OK;
    });
  return s.finish();
}

void gsea_prepare(Shared& sh, const Call& c, int ndev) {
  if (c.method == kGseaMultilevel) sh.gsea.ml.assign((size_t)c.m * c.n * 4, std::numeric_limits<double>::quiet_NaN());
  if (ndev > 1)
    sh.gsea.part.assign((size_t)((c.nperm + PLAIDHIP_GSEA_PERM_BLOCK - 1) / PLAIDHIP_GSEA_PERM_BLOCK) * c.n * 6 * c.m, 0.0);
}

}  // namespace plaidhip
