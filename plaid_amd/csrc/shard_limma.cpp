// plaid.limma and plaid.camera on the sharded engine (shard.cpp).
#include "shard.h"
#include "roast.h"

namespace plaidhip {

namespace {

// plaid.limma with na = "fit", after the effects are chained: shard 0 merges the shards' NaN lists in shard order (a row's
// columns ascending), decides which rows are fitted (max_na) and which (row, fit) pairs are incomplete, and runs Gram and
// solve (kernels_lmfit.hip) over those: the pair's effects in sh.limma.effects become gamma, its mean the mean over the
// observed samples, and sh.limma.na_d / na_u take every row's df.residual (NaN: not fitted) and u_j.  A pair's chain runs
// over the row's own missing samples in ascending order whatever the sharding, so every sharding has the one-device bits.
int limma_na_refit(plaidhip_ctx* ctx, const Call& c, int ndev, Shared& sh, double* d_E) {
  const int32_t rows = c.g, n = c.n, p = c.ncoef, nfit = c.nfit, q = c.nq;
  const size_t R = (size_t)rows;
  const int64_t W = (int64_t)nfit * (p + 1);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int64_t> off(R + 1, 0);
  for (size_t r = 0; r < R; ++r) {
    int64_t tot = 0;
    for (int k = 0; k < ndev; ++k) tot += sh.limma.na_cnt[(size_t)k].empty() ? 0 : sh.limma.na_cnt[(size_t)k][r];
    off[r + 1] = off[r] + tot;
  }
  std::vector<int32_t> list((size_t)off[R]);
  std::vector<size_t> pos((size_t)ndev, 0);
  for (size_t r = 0; r < R; ++r) {
    int64_t w = off[r];
    for (int k = 0; k < ndev; ++k) {
      const int32_t ck = sh.limma.na_cnt[(size_t)k].empty() ? 0 : sh.limma.na_cnt[(size_t)k][r];
      std::copy(sh.limma.na_list[(size_t)k].begin() + pos[(size_t)k], sh.limma.na_list[(size_t)k].begin() + pos[(size_t)k] + ck,
                list.begin() + w);
      pos[(size_t)k] += (size_t)ck;
      w += ck;
    }
  }
  sh.limma.na_d.assign(R * nfit, nan);
  sh.limma.na_u.assign(R * nfit * q, nan);
  std::vector<int32_t> pairs, nobs;
  for (int32_t f = 0; f < nfit; ++f)
    for (size_t r = 0; r < R; ++r) {
      const bool fitted = (double)(off[r + 1] - off[r]) / (double)n <= c.max_na;   // rowMeans(is.na(X)) <= max.na
      const int64_t mis = sh.limma.na_pair[R * f + r], d = c.lm_nf[(size_t)f] - mis - p;
      if (fitted && d >= 1) sh.limma.na_d[R * f + r] = (double)d;
      for (int32_t j = 0; j < q; ++j) sh.limma.na_u[((size_t)f * q + j) * R + r] = c.lm_u[(size_t)f * q + j];
      if (mis > 0 && fitted && d >= 1) {
        pairs.push_back((int32_t)r);
        pairs.push_back(f);
        nobs.push_back((int32_t)(c.lm_nf[(size_t)f] - mis));
      }
    }
  const size_t np = nobs.size();
  if (np == 0) return PLAIDHIP_OK;
  std::vector<double> nfd((size_t)nfit), upair(np * q);
  std::vector<int32_t> okp(np);
  for (int32_t f = 0; f < nfit; ++f) nfd[(size_t)f] = (double)c.lm_nf[(size_t)f];
  DevBuf dpairs, doff, dlist, dQ, duse, dv, dnobs, dnf, du, dok;
  auto up = [&](DevBuf& b, const void* src, size_t bytes) -> int {
    PH_TRY(b.alloc(bytes));
    PH_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return PLAIDHIP_OK;
  };
  PH_TRY(up(dpairs, pairs.data(), pairs.size() * 4));
  PH_TRY(up(doff, off.data(), off.size() * 8));
  PH_TRY(up(dlist, list.data(), list.size() * 4));
  PH_TRY(up(dQ, c.lm_Q.data(), c.lm_Q.size() * 8));
  if (c.use != nullptr) PH_TRY(up(duse, c.use, (size_t)n * nfit));
  PH_TRY(up(dv, c.lm_v.data(), c.lm_v.size() * 8));
  PH_TRY(up(dnobs, nobs.data(), np * 4));
  PH_TRY(up(dnf, nfd.data(), nfd.size() * 8));
  PH_TRY(du.alloc(np * q * 8));
  PH_TRY(dok.alloc(np * 4));
  PH_HIP(hipMemcpyAsync(d_E, sh.limma.effects.data(), (size_t)W * R * 8, hipMemcpyHostToDevice, ctx->stream));
  PH_TRY(launch_lmfit_na_solve(ctx, (int64_t)np, dpairs.as<int32_t>(), doff.as<int64_t>(), dlist.as<int32_t>(), dQ.as<double>(),
                               c.use != nullptr ? duse.as<int8_t>() : nullptr, n, p, q, dv.as<double>(), dnobs.as<int32_t>(),
                               dnf.as<double>(), rows, d_E, du.as<double>(), dok.as<int32_t>()));
  PH_HIP(hipMemcpyAsync(sh.limma.effects.data(), d_E, (size_t)W * R * 8, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipMemcpyAsync(upair.data(), du.p, np * q * 8, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipMemcpyAsync(okp.data(), dok.p, np * 4, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < np; ++i) {
    const size_t r = (size_t)pairs[2 * i], f = (size_t)pairs[2 * i + 1];
    if (!okp[i]) sh.limma.na_d[R * f + r] = nan;
    for (int32_t j = 0; j < q; ++j) sh.limma.na_u[(f * q + j) * R + r] = upair[i * q + j];
  }
  return PLAIDHIP_OK;
}

// plaid.fry after plaid.limma's two rounds (include/plaidhip.h: plaidhip_fry).  Shard 0 makes the divisors c_g from the
// residual sums of squares of ALL samples (the prior needs every gene's).  Then, fit by fit: Z' of the shard's columns
// (kernels_fry.hip), T = G'Z' and the block partials of the sums of T^2, as the estimated-VIF branch of plaid.camera below;
// and for a fit under the cap the residual effects rho = Q2'z' as d (+ 1, the pass's mean column) more weight columns of the
// effects pass run over Z', chained as [d + 1][rows].  A last round chains the sums of T^2 as [nfit][m].
int fry_rounds(Shard& s, CtxBuf& dA, int64_t ld, DevBuf& dQ, DevBuf& duse, DevBuf& dmask, double* d_E) {
  plaidhip_ctx* ctx = s.ctx;
  const Call& c = s.c;
  Shared& sh = s.sh;
  const int32_t lo = s.lo, nloc = s.nloc, rows = c.g, n = c.n, p = c.ncoef, nfit = c.nfit, m = c.m;
  if (s.k == 0)
    s.step([&]() -> int {
      fry_divisors(rows, p, nfit, sh.limma.rss.data(), c.lm_nf.data(), c.standardize, sh.fry.cg.data());
      return PLAIDHIP_OK;
    });
  sh.rv.arrive_and_wait();
  int64_t dmax = 0;   // the widest fit under the cap
  for (int32_t f = 0; f < nfit; ++f)
    if (c.lm_Q2_off[(size_t)f] >= 0) dmax = std::max<int64_t>(dmax, c.lm_nf[(size_t)f] - p);
  const int64_t Wmax = dmax > 0 ? dmax + 1 : 0;
  CtxBuf dZ{ctx, 3}, dT{ctx, 4}, dsq{ctx, 5};
  DevBuf dcg, dq2, dzero, dmask2, dwt2, dws2, dchain2;
  double *d_part = nullptr, *d_chain = nullptr;
  std::vector<double> q2loc;
  plaidhip_geneset* gs = nullptr;
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    PH_TRY(acquire_geneset(ctx, rows, m, c.Gp, c.Gi, &gs));
    PH_TRY(dcg.alloc((size_t)nfit * rows * 8));
    PH_HIP(hipMemcpyAsync(dcg.p, sh.fry.cg.data(), (size_t)nfit * rows * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dZ.alloc((size_t)ld * nloc * 8));
    PH_TRY(dT.alloc((size_t)m * nloc * 8));
    const size_t npart = (size_t)camera_sumsq_ws_doubles(nloc, (int64_t)nfit * m);
    PH_TRY(dsq.alloc((npart + (size_t)nfit * m * 2) * 8));
    d_part = dsq.as<double>();
    d_chain = d_part + npart;
    if (Wmax > 0) {
      PH_TRY(dq2.alloc((size_t)nloc * dmax * 8));
      PH_TRY(dzero.alloc(8));
      PH_HIP(hipMemsetAsync(dzero.p, 0, 8, ctx->stream));   // (the weight of the effects pass's mean column: not used)
      PH_TRY(dmask2.alloc((size_t)lmfit_mask_bytes(nloc, Wmax)));
      PH_TRY(dwt2.alloc((size_t)lmfit_weight_bytes(nloc, Wmax)));
      PH_TRY(dws2.alloc((size_t)row_design_ws_doubles(rows, nloc, Wmax) * 8));
      PH_TRY(dchain2.alloc((size_t)Wmax * rows * 2 * 8));
    }
    return PLAIDHIP_OK;
  });
  for (int32_t f = 0; f < nfit; ++f) {
    const int64_t off2 = c.lm_Q2_off[(size_t)f], d = c.lm_nf[(size_t)f] - p, W = d + 1;
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      PH_TRY(launch_fry_residuals(ctx, dA.as<double>(), ld, rows, nloc, dQ.as<double>(), dmask.p, p, f, d_E, dcg.as<double>(),
                                  dZ.as<double>(), ld));
      PH_TRY(launch_spmm_dense_f64(ctx, gs, dZ.as<double>(), ld, nloc, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0, dT.as<double>(), m,
                                   nullptr));
      PH_TRY(launch_camera_sumsq(ctx, dT.as<double>(), m, m, nloc, d_part + (size_t)f * m, (int64_t)nfit * m));
      if (off2 < 0) return PLAIDHIP_OK;
      PH_HIP(hipStreamSynchronize(ctx->stream));   // (q2loc below is the source of the previous fit's upload)
      q2loc.resize((size_t)nloc * d);
      for (int64_t col = 0; col < d; ++col)
        std::copy(c.lm_Q2.begin() + off2 + col * n + lo, c.lm_Q2.begin() + off2 + col * n + lo + nloc,
                  q2loc.begin() + col * nloc);
      PH_HIP(hipMemcpyAsync(dq2.p, q2loc.data(), q2loc.size() * 8, hipMemcpyHostToDevice, ctx->stream));
      PH_TRY(launch_lmfit_masks(ctx, dq2.as<double>(), c.use != nullptr ? duse.as<int8_t>() + (size_t)f * nloc : nullptr,
                                dzero.as<double>(), nloc, (int32_t)d, 1, dmask2.p, dwt2.as<double>()));
      return launch_row_design_effects(ctx, dZ.as<double>(), ld, rows, nloc, dmask2.p, dwt2.as<double>(), (int32_t)W,
                                       dws2.as<double>());
    });
    if (off2 >= 0)
      chain_flat_sums(s, sh.fry.rho[(size_t)f], dws2.as<double>(), W * rows, dchain2.as<double>(),
                      dchain2.as<double>() + (size_t)W * rows);
  }
  chain_flat_sums(s, sh.camera.ss, d_part, (int64_t)nfit * m, d_chain, d_chain + (size_t)nfit * m);
  return s.finish();
}

}  // namespace

// one device's part of plaid.limma (kLimma, kernels_lmfit.hip; include/plaidhip.h: plaidhip_limma).  The SAMPLES are shared
// out at multiples of 128 columns, as for plaid.test.contrasts: a shard takes its columns of A and its rows of every Q_f and
// of use.  Round one chains the effects and means [W][rows] from shard to shard; after it every shard holds the effects of
// all samples and takes the residual sums of squares of its own columns, which round two chains as [nfit][rows].  The block
// partials are added in the order of the one-device call, so every sharding has its bits.  2 ndev rendezvous.
// na = "fit" (c.na_fit): both passes take the select "used and not NaN"; round one also lists the NaN of the shard's columns
// (the count pass), and between the rounds shard 0 refits the incomplete (row, fit) pairs (limma_na_refit): one more rendezvous.
int limma_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc, rows = c.g, n = c.n, p = c.ncoef, nfit = c.nfit;
  const int64_t W = (int64_t)nfit * (p + 1), ld = even_ld(rows);
  if (c.method == kCamera || c.method == kFry) s.force_f64();   // (T = G'Z stays on the fp64 kernels whatever precision the context was given)
  CtxBuf dA{ctx, 0};
  DevBuf dQ, duse, dinvn, dmask, dwt, dws, drows;
  double *d_seed = nullptr, *d_run = nullptr, *d_E = nullptr;
  // host sources of asynchronous uploads: they live until the worker's last synchronisation
  std::vector<double> qloc;
  std::vector<int8_t> uloc;

  // ---- upload; the shard's rows of Q and use, their masks and tile weights; the effects' block partials ----------------------
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    PH_HIP(hipSetDevice(ctx->device));
    if (nloc == 0) return PLAIDHIP_OK;
    PH_TRY(drows.alloc((size_t)W * rows * 3 * 8));   // [seed | running sums | the effects of all samples], [W][rows] each
    d_seed = drows.as<double>();
    d_run = d_seed + W * rows;
    d_E = d_run + W * rows;
    qloc.resize((size_t)nloc * p * nfit);
    for (int64_t col = 0; col < (int64_t)p * nfit; ++col)
      std::copy(c.lm_Q.begin() + col * n + lo, c.lm_Q.begin() + col * n + lo + nloc, qloc.begin() + col * nloc);
    PH_TRY(dQ.alloc(qloc.size() * 8));
    PH_HIP(hipMemcpyAsync(dQ.p, qloc.data(), qloc.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (c.use != nullptr) {
      uloc.resize((size_t)nloc * nfit);
      for (int32_t f = 0; f < nfit; ++f)
        std::copy(c.use + (size_t)f * n + lo, c.use + (size_t)f * n + lo + nloc, uloc.begin() + (size_t)f * nloc);
      PH_TRY(duse.alloc(uloc.size()));
      PH_HIP(hipMemcpyAsync(duse.p, uloc.data(), uloc.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    PH_TRY(dinvn.alloc((size_t)nfit * 8));
    PH_HIP(hipMemcpyAsync(dinvn.p, c.lm_invn.data(), (size_t)nfit * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dmask.alloc((size_t)lmfit_mask_bytes(nloc, W)));
    PH_TRY(dwt.alloc((size_t)lmfit_weight_bytes(nloc, W)));
    PH_TRY(launch_lmfit_masks(ctx, dQ.as<double>(), c.use != nullptr ? duse.as<int8_t>() : nullptr, dinvn.as<double>(), nloc, p,
                              nfit, dmask.p, dwt.as<double>()));
    PH_TRY(dws.alloc((size_t)row_design_ws_doubles(rows, nloc, W) * 8));   // (W >= nfit: the RSS partials fit too)
    PH_TRY(dA.alloc((size_t)ld * nloc * 8));
    PH_TRY(upload_pipelined(ctx, dA.as<char>(), (size_t)ld * 8, reinterpret_cast<const char*>(c.X + (int64_t)lo * rows),
                            (size_t)rows * 8, nloc, nullptr));
    PH_TRY(launch_row_design_effects(ctx, dA.as<double>(), ld, rows, nloc, dmask.p, dwt.as<double>(), (int32_t)W,
                                     dws.as<double>(), c.na_fit != 0));
    if (!c.na_fit) return PLAIDHIP_OK;
    // the count pass: the NaN of every (column block, row) of the shard, their columns in ascending order (a second sweep,
    // once the space is known), and the NaN of every (fit, row) inside the fit's used samples
    std::vector<int32_t>& cnt = sh.limma.na_cnt[(size_t)k];
    std::vector<int32_t>& list = sh.limma.na_list[(size_t)k];
    const size_t R = (size_t)rows, nblk = ((size_t)nloc + 127) / 128;
    std::vector<int32_t> bcnt(nblk * R);                   // [block][row]
    DevBuf dcnt, doff, drow, dlist, dpc;
    PH_TRY(dcnt.alloc(bcnt.size() * 4));
    PH_TRY(launch_lmfit_nan_rows(ctx, dA.as<double>(), ld, rows, nloc, nullptr, dcnt.as<int32_t>(), nullptr));
    PH_HIP(hipMemcpyAsync(bcnt.data(), dcnt.p, bcnt.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    cnt.assign(R, 0);
    std::vector<int64_t> off(nblk * R), rowoff(R + 1, 0);   // where (block, row) writes; where a row's list starts
    int64_t run = 0;
    for (size_t r = 0; r < R; ++r) {
      for (size_t b = 0; b < nblk; ++b) {
        off[b * R + r] = run;
        run += bcnt[b * R + r];
      }
      cnt[r] = (int32_t)(run - rowoff[r]);
      rowoff[r + 1] = run;
    }
    const size_t total = (size_t)run;
    if (total == 0) return PLAIDHIP_OK;
    std::vector<int32_t> pc((size_t)nfit * rows);
    list.resize(total);
    PH_TRY(doff.alloc(off.size() * 8));
    PH_HIP(hipMemcpyAsync(doff.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(drow.alloc(rowoff.size() * 8));
    PH_HIP(hipMemcpyAsync(drow.p, rowoff.data(), rowoff.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dlist.alloc(total * 4));
    PH_TRY(dpc.alloc(pc.size() * 4));
    PH_TRY(launch_lmfit_nan_rows(ctx, dA.as<double>(), ld, rows, nloc, doff.as<int64_t>(), nullptr, dlist.as<int32_t>()));
    PH_TRY(launch_lmfit_nan_pairs(ctx, drow.as<int64_t>(), dlist.as<int32_t>(), c.use != nullptr ? duse.as<int8_t>() : nullptr,
                                  rows, nloc, nfit, dpc.as<int32_t>()));
    PH_HIP(hipMemcpyAsync(list.data(), dlist.p, total * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(pc.data(), dpc.p, pc.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    for (int32_t& col : list) col += lo;
    std::lock_guard<std::mutex> lk(sh.mu);
    for (size_t i = 0; i < pc.size(); ++i) sh.limma.na_pair[i] += pc[i];
    return PLAIDHIP_OK;
  });
  chain_flat_sums(s, sh.limma.effects, dws.as<double>(), W * rows, d_seed, d_run);
  if (c.na_fit) {   // (every shard's lists are complete: chain_flat_sums has met ndev times since)
    if (k == 0) s.step([&]() -> int { return limma_na_refit(ctx, c, ndev, sh, d_E); });
    sh.rv.arrive_and_wait();
  }

  // ---- the residual sums of squares of the shard's columns at the effects of ALL samples -------------------------------------
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    PH_HIP(hipMemcpyAsync(d_E, sh.limma.effects.data(), (size_t)W * rows * 8, hipMemcpyHostToDevice, ctx->stream));
    return launch_row_design_rss(ctx, dA.as<double>(), ld, rows, nloc, dQ.as<double>(), dmask.p, p, nfit, d_E,
                                 dws.as<double>(), c.na_fit != 0);
  });
  chain_flat_sums(s, sh.limma.rss, dws.as<double>(), (int64_t)nfit * rows, d_seed, d_run);
  if (c.method == kFry) return fry_rounds(s, dA, ld, dQ, duse, dmask, d_E);
  if (c.method != kCamera || !std::isnan(c.inter_gene_cor)) return s.finish();

  // ---- plaid.camera, the estimated correlation: fit by fit, Z of the shard's columns from the effects and the residual sums of
  // squares of ALL samples (every shard has met ndev times since the last of them was added), T = G'Z by the dense crossprod,
  // and the block partials of the sums of T^2, [nblk][nfit][m]; round three chains them as [nfit][m].  One fit's Z and T are
  // alive at a time. ----------------------------------------------------------------------------------------------------------
  const int32_t m = c.m;
  CtxBuf dZ{ctx, 3}, dT{ctx, 4}, dsq{ctx, 5};   // (they live in the context between calls, as A does)
  double *d_part = nullptr, *d_chain = nullptr;   // dsq: [the block partials | the chain's seed | its running sums]
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    plaidhip_geneset* gs = nullptr;
    PH_TRY(acquire_geneset(ctx, rows, m, c.Gp, c.Gi, &gs));
    double* d_rss = d_seed;   // (the chains above are done with it; W >= nfit)
    PH_HIP(hipMemcpyAsync(d_rss, sh.limma.rss.data(), (size_t)nfit * rows * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dZ.alloc((size_t)ld * nloc * 8));
    PH_TRY(dT.alloc((size_t)m * nloc * 8));
    const size_t npart = (size_t)camera_sumsq_ws_doubles(nloc, (int64_t)nfit * m);
    PH_TRY(dsq.alloc((npart + (size_t)nfit * m * 2) * 8));
    d_part = dsq.as<double>();
    d_chain = d_part + npart;
    for (int32_t f = 0; f < nfit; ++f) {
      PH_TRY(launch_camera_residuals(ctx, dA.as<double>(), ld, rows, nloc, dQ.as<double>(), dmask.p, p, f, d_E, d_rss,
                                     (double)(c.lm_nf[(size_t)f] - p), dZ.as<double>(), ld));
      PH_TRY(launch_spmm_dense_f64(ctx, gs, dZ.as<double>(), ld, nloc, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0, dT.as<double>(), m,
                                   nullptr));
      PH_TRY(launch_camera_sumsq(ctx, dT.as<double>(), m, m, nloc, d_part + (size_t)f * m, (int64_t)nfit * m));
    }
    return PLAIDHIP_OK;
  });
  chain_flat_sums(s, sh.camera.ss, d_part, (int64_t)nfit * m, d_chain, d_chain + (size_t)nfit * m);
  return s.finish();
}

bool limma_empty(const Call& c) {
  return c.g == 0 || c.nfit == 0 || c.nq == 0 || ((c.method == kCamera || c.method == kFry || c.method == kRoast || c.method == kRomer) && c.m == 0);
}

void limma_prepare(Shared& sh, const Call& c, int ndev) {
  if (c.method == kCamera || c.method == kFry) sh.camera.ss.assign((size_t)c.nfit * c.m, 0.0);
  if (c.method == kFry) {
    sh.fry.cg.assign((size_t)c.nfit * c.g, 0.0);
    sh.fry.rho.assign((size_t)c.nfit, std::vector<double>());
    for (int32_t f = 0; f < c.nfit; ++f)
      if (c.lm_Q2_off[(size_t)f] >= 0) sh.fry.rho[(size_t)f].assign((size_t)(c.lm_nf[(size_t)f] - c.ncoef + 1) * c.g, 0.0);
  }
  sh.limma.effects.assign((size_t)c.nfit * (c.ncoef + 1) * c.g, 0.0);
  sh.limma.rss.assign((size_t)c.nfit * c.g, 0.0);
  if (c.weighted) {
    sh.limma.wsum.assign((size_t)c.nfit * (size_t)lmfit_w_columns(c.ncoef) * c.g, 0.0);
    sh.limma.wcnt.assign((2 * (size_t)c.nfit + 1) * c.g, 0.0);
  }
  if (c.na_fit) {
    sh.limma.na_cnt.resize((size_t)ndev);
    sh.limma.na_list.resize((size_t)ndev);
    sh.limma.na_pair.assign((size_t)c.nfit * c.g, 0);
  }
}

// plaid.limma after the workers: eBayes and the tables, on the host from the chained sums
int limma_tail(plaidhip_ctx*, const Call& c, Shared& sh) {
  if (!c.na_fit && !c.weighted)
    return plaidhip_limma_finish(c.g, c.ncoef, c.nfit, c.nq, sh.limma.effects.data(), sh.limma.rss.data(), c.lm_nf.data(),
                                 c.lm_v.data(), c.lm_u.data(), c.out, c.hyper);
  PH_TRY(plaidhip_limma_finish_na(c.g, c.ncoef, c.nfit, c.nq, sh.limma.effects.data(), sh.limma.rss.data(), c.lm_nf.data(),
                                  c.lm_v.data(), sh.limma.na_d.data(), sh.limma.na_u.data(), c.out, c.hyper));
  const size_t R = (size_t)c.g;   // df.residual of the rows that came out of the fit; NaN for the others
  for (int32_t f = 0; f < c.nfit; ++f) {
    const double* sigma2 = c.out + ((size_t)f * c.nq * 6 + 5) * R;   // (of the fit's first contrast: NaN = not ok)
    for (size_t r = 0; r < R; ++r)
      c.dfres[R * f + r] = std::isnan(sigma2[r]) ? std::numeric_limits<double>::quiet_NaN() : sh.limma.na_d[R * f + r];
  }
  return PLAIDHIP_OK;
}

// plaid.camera after the workers: eBayes and the gene statistics on the host (plaidhip_limma_finish), the member sums of t
// and the counts of ok members from ONE crossprod of the membership with [the t columns | the ok indicators] on the first
// context (a gene that is not ok holds 0.0 in both), then the pinned test (plaidhip_camera_finish).
int camera_tail(plaidhip_ctx* ctx, const Call& c, Shared& sh) {
  const int32_t g = c.g, m = c.m, nfit = c.nfit, q = c.nq, p = c.ncoef;
  const size_t R = (size_t)g, ncol = (size_t)nfit * q;
  std::vector<double> tab(R * 6 * ncol), hyp((size_t)nfit * 4);
  PH_TRY(plaidhip_limma_finish(g, p, nfit, q, sh.limma.effects.data(), sh.limma.rss.data(), c.lm_nf.data(), c.lm_v.data(),
                               c.lm_u.data(), tab.data(), hyp.data()));
  std::vector<double> B(R * (ncol + nfit)), t(R * ncol), S((size_t)m * (ncol + nfit)), dres((size_t)nfit), dprior((size_t)nfit);
  std::vector<int8_t> ok(R * nfit);
  for (int32_t f = 0; f < nfit; ++f) {
    const double* sigma2 = tab.data() + ((size_t)f * q * 6 + 5) * R;   // (of the fit's first contrast: NaN = not ok)
    for (size_t r = 0; r < R; ++r) {
      ok[R * f + r] = std::isnan(sigma2[r]) ? 0 : 1;
      B[(ncol + f) * R + r] = ok[R * f + r] ? 1.0 : 0.0;
    }
    for (int32_t j = 0; j < q; ++j) {
      const size_t col = (size_t)f * q + j;
      const double* tj = tab.data() + (col * 6 + 2) * R;
      for (size_t r = 0; r < R; ++r) {
        t[col * R + r] = tj[r];
        B[col * R + r] = ok[R * f + r] ? tj[r] : 0.0;
      }
    }
    dres[(size_t)f] = hyp[4 * (size_t)f];
    dprior[(size_t)f] = hyp[4 * (size_t)f + 1];
  }
  const int saved = ctx->precision;
  ctx->precision = PLAIDHIP_PRECISION_F64;
  int rc = [&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    plaidhip_geneset* gs = nullptr;
    PH_TRY(acquire_geneset(ctx, g, m, c.Gp, c.Gi, &gs));
    DevBuf dB, dS;
    PH_TRY(dB.alloc(B.size() * 8));
    PH_TRY(dS.alloc(S.size() * 8));
    PH_TRY(upload_host(ctx, dB.p, R * 8, B.data(), R * 8, (int64_t)(ncol + nfit)));
    PH_TRY(launch_spmm_dense_f64(ctx, gs, dB.as<double>(), g, (int32_t)(ncol + nfit), PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0,
                                 dS.as<double>(), m, nullptr));
    PH_HIP(hipMemcpyAsync(S.data(), dS.p, S.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    return PLAIDHIP_OK;
  }();
  ctx->precision = saved;
  if (rc != PLAIDHIP_OK) return rc;
  const bool estimate = std::isnan(c.inter_gene_cor);
  std::vector<double> gdf((size_t)nfit * 2);
  PH_TRY(plaidhip_camera_finish(g, m, nfit, q, t.data(), ok.data(), S.data(), S.data() + (size_t)m * ncol,
                                estimate ? sh.camera.ss.data() : nullptr, dres.data(), dprior.data(), c.inter_gene_cor,
                                c.allow_neg_cor, c.out, gdf.data()));
  for (int32_t f = 0; f < nfit; ++f) {
    for (int h = 0; h < 4; ++h) c.hyper[6 * (size_t)f + h] = hyp[4 * (size_t)f + h];
    c.hyper[6 * (size_t)f + 4] = gdf[2 * (size_t)f];
    c.hyper[6 * (size_t)f + 5] = gdf[2 * (size_t)f + 1];
  }
  return PLAIDHIP_OK;
}

// plaid.fry after the workers (include/plaidhip.h: plaidhip_fry).  eBayes and the gene statistics on the host
// (plaidhip_limma_finish), e_gj = logFC / (u_j c_g), the member sums of e and the counts from ONE crossprod as in
// camera_tail; for every fit under the cap the Gram matrices and their two eigenvalues on the first context, sets in
// chunks of at most 256 MiB of C; then the pinned tests (plaidhip_fry_finish).  Everything here is made from the chained
// sums, so every sharding has the one-device bits.
int fry_tail(plaidhip_ctx* ctx, const Call& c, Shared& sh) {
  const int32_t g = c.g, m = c.m, nfit = c.nfit, q = c.nq, p = c.ncoef;
  const size_t R = (size_t)g, M = (size_t)m, ncol = (size_t)nfit * q;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> tab(R * 6 * ncol), hyp((size_t)nfit * 4);
  PH_TRY(plaidhip_limma_finish(g, p, nfit, q, sh.limma.effects.data(), sh.limma.rss.data(), c.lm_nf.data(), c.lm_v.data(),
                               c.lm_u.data(), tab.data(), hyp.data()));
  std::vector<double> B(R * (ncol + nfit)), S(M * (ncol + nfit)), dres((size_t)nfit), uni((size_t)nfit, 0.0);
  std::vector<int8_t> mixed((size_t)nfit, 0);
  bool any_mixed = false;
  for (int32_t f = 0; f < nfit; ++f) {
    const double* cg = sh.fry.cg.data() + R * f;
    for (size_t r = 0; r < R; ++r) {
      const bool in = cg[r] == cg[r];
      B[(ncol + f) * R + r] = in ? 1.0 : 0.0;
      uni[(size_t)f] += in ? 1.0 : 0.0;
    }
    for (int32_t j = 0; j < q; ++j) {
      const size_t col = (size_t)f * q + j;
      const double* fc = tab.data() + col * 6 * R;
      const double uj = c.lm_u[col];
      for (size_t r = 0; r < R; ++r) B[col * R + r] = cg[r] == cg[r] ? fc[r] / (uj * cg[r]) : 0.0;
    }
    dres[(size_t)f] = hyp[4 * (size_t)f];
    mixed[(size_t)f] = c.lm_Q2_off[(size_t)f] >= 0 ? 1 : 0;
    any_mixed = any_mixed || mixed[(size_t)f] != 0;
  }
  std::vector<double> sume2, lam1, lamD, trM, froM;
  if (any_mixed) {
    sume2.assign(M * ncol, nan);
    lam1.assign(M * ncol, nan);
    lamD.assign(M * ncol, nan);
    trM.assign(M * ncol, nan);
    froM.assign(M * ncol, nan);
  }
  const int saved = ctx->precision;
  ctx->precision = PLAIDHIP_PRECISION_F64;
  int rc = [&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    plaidhip_geneset* gs = nullptr;
    PH_TRY(acquire_geneset(ctx, g, m, c.Gp, c.Gi, &gs));
    DevBuf dB, dS;
    PH_TRY(dB.alloc(B.size() * 8));
    PH_TRY(dS.alloc(S.size() * 8));
    PH_TRY(upload_host(ctx, dB.p, R * 8, B.data(), R * 8, (int64_t)(ncol + nfit)));
    PH_TRY(launch_spmm_dense_f64(ctx, gs, dB.as<double>(), g, (int32_t)(ncol + nfit), PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0,
                                 dS.as<double>(), m, nullptr));
    PH_HIP(hipMemcpyAsync(S.data(), dS.p, S.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    if (!any_mixed) return PLAIDHIP_OK;
    DevBuf dGp, dGi, drho, de, dC, db, da, dtr, dfro, dDk, dl1, dlD, dsw, dcv;
    PH_TRY(upload_pattern(ctx, c.Gp, c.Gi, m, dGp, dGi));
    std::vector<double> rhoT, eT, ha, htr, hfro, hl1, hlD;
    std::vector<int32_t> Dk, hcv;
    // the device buffers once, sized for the largest need of any fit under the cap (a set chunk holds at most 256 MiB of C)
    auto chunk_of = [&](int32_t d) {
      return (int32_t)std::max<int64_t>(1, std::min<int64_t>(m, ((int64_t)256 << 20) / ((int64_t)d * d * 8)));
    };
    size_t max_rho = 0, max_C = 0, max_b = 0, max_nq = 0;
    for (int32_t f = 0; f < nfit; ++f) {
      if (!mixed[(size_t)f]) continue;
      const int32_t d = (int32_t)(c.lm_nf[(size_t)f] - p);
      const size_t ch = (size_t)chunk_of(d);
      max_rho = std::max(max_rho, R * (size_t)d);
      max_C = std::max(max_C, ch * (size_t)d * d);
      max_b = std::max(max_b, ch * q * (size_t)d);
      max_nq = std::max(max_nq, ch * q);
    }
    PH_TRY(drho.alloc(max_rho * 8));
    PH_TRY(de.alloc(R * q * 8));
    PH_TRY(dC.alloc(max_C * 8));
    PH_TRY(db.alloc(max_b * 8));
    PH_TRY(da.alloc(max_nq * 8));
    PH_TRY(dtr.alloc(max_nq * 8));
    PH_TRY(dfro.alloc(max_nq * 8));
    PH_TRY(dDk.alloc(max_nq * 4));
    PH_TRY(dl1.alloc(max_nq * 8));
    PH_TRY(dlD.alloc(max_nq * 8));
    PH_TRY(dsw.alloc(max_nq * 4));
    PH_TRY(dcv.alloc(max_nq * 4));
    for (int32_t f = 0; f < nfit; ++f) {
      if (!mixed[(size_t)f]) continue;
      const int32_t d = (int32_t)(c.lm_nf[(size_t)f] - p);
      const double* rho = sh.fry.rho[(size_t)f].data();   // [d + 1][rows]; gene-major for the gather
      rhoT.resize(R * d);
      eT.resize(R * q);
      for (int32_t k = 0; k < d; ++k)
        for (size_t r = 0; r < R; ++r) rhoT[r * d + k] = rho[(size_t)k * R + r];
      for (int32_t j = 0; j < q; ++j)
        for (size_t r = 0; r < R; ++r) eT[r * q + j] = B[((size_t)f * q + j) * R + r];
      const int32_t chunk = chunk_of(d);
      const size_t nq = (size_t)chunk * q;
      PH_TRY(upload_host(ctx, drho.p, 1, rhoT.data(), 1, (int64_t)rhoT.size() * 8));
      PH_TRY(upload_host(ctx, de.p, 1, eT.data(), 1, (int64_t)eT.size() * 8));
      ha.resize(nq); htr.resize(nq); hfro.resize(nq); hl1.resize(nq); hlD.resize(nq); Dk.resize(nq); hcv.resize(nq);
      for (int32_t s0 = 0; s0 < m; s0 += chunk) {
        const int32_t ns = std::min(chunk, m - s0);
        const size_t np = (size_t)ns * q;
        for (int32_t s = 0; s < ns; ++s) {
          const double mm = S[(ncol + f) * M + s0 + s];
          for (int32_t j = 0; j < q; ++j) Dk[(size_t)s * q + j] = (int32_t)std::max(1.0, std::min(mm, (double)d + 1.0));
        }
        PH_HIP(hipMemcpyAsync(dDk.p, Dk.data(), np * 4, hipMemcpyHostToDevice, ctx->stream));
        PH_TRY(launch_fry_gram(ctx, drho.as<double>(), de.as<double>(), d, q, dGp.as<int32_t>(), dGi.as<int32_t>(), s0, ns,
                               dC.as<double>(), db.as<double>(), da.as<double>(), dtr.as<double>(), dfro.as<double>()));
        PH_TRY(launch_fry_eigen(ctx, nullptr, dC.as<double>(), db.as<double>(), da.as<double>(), d + 1, q, (int64_t)np,
                                dDk.as<int32_t>(), dl1.as<double>(), dlD.as<double>(), dsw.as<int32_t>(), dcv.as<int32_t>()));
        PH_HIP(hipMemcpyAsync(ha.data(), da.p, np * 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipMemcpyAsync(htr.data(), dtr.p, np * 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipMemcpyAsync(hfro.data(), dfro.p, np * 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipMemcpyAsync(hl1.data(), dl1.p, np * 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipMemcpyAsync(hlD.data(), dlD.p, np * 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipMemcpyAsync(hcv.data(), dcv.p, np * 4, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));
        for (int32_t s = 0; s < ns; ++s)
          for (int32_t j = 0; j < q; ++j) {
            const size_t src = (size_t)s * q + j, dst = ((size_t)f * q + j) * M + s0 + s;
            const bool okc = hcv[src] != 0;   // (a problem that did not converge has no eigenvalues: NaN in the mixed columns)
            sume2[dst] = ha[src];
            trM[dst] = htr[src];
            froM[dst] = hfro[src];
            lam1[dst] = okc ? hl1[src] : nan;
            lamD[dst] = okc ? hlD[src] : nan;
          }
      }
    }
    return PLAIDHIP_OK;
  }();
  ctx->precision = saved;
  if (rc != PLAIDHIP_OK) return rc;
  PH_TRY(plaidhip_fry_finish(m, nfit, q, dres.data(), S.data() + M * ncol, S.data(), sh.camera.ss.data(),
                             any_mixed ? sume2.data() : nullptr, any_mixed ? lam1.data() : nullptr,
                             any_mixed ? lamD.data() : nullptr, any_mixed ? trM.data() : nullptr,
                             any_mixed ? froM.data() : nullptr, any_mixed ? mixed.data() : nullptr, c.out));
  for (int32_t f = 0; f < nfit; ++f) {
    for (int h = 0; h < 4; ++h) c.hyper[7 * (size_t)f + h] = hyp[4 * (size_t)f + h];
    c.hyper[7 * (size_t)f + 4] = uni[(size_t)f];
    c.hyper[7 * (size_t)f + 5] = dres[(size_t)f] + 1.0;
    c.hyper[7 * (size_t)f + 6] = mixed[(size_t)f] ? 1.0 : 0.0;
  }
  return PLAIDHIP_OK;
}

// plaid.roast (include/plaidhip.h: plaidhip_roast).  The ROTATIONS are dealt to the shards in whole tiles of 64: shard k
// takes tiles [ntile k / ndev, ntile (k + 1) / ndev).  Every shard takes all of X and runs plaid.limma's two passes itself,
// with the operations and the order of the one-device call (a 0.0 seed, then the block partials ascending), so every shard
// holds the same effects, RSS, tables and observed statistics; no rendezvous.  Then, fit by fit: the raw residuals of all
// samples (kernels_fry.hip's pass with a divisor of 1.0) and, per contrast, the observed statistics, z of the shard's
// rotations in chunks of whole tiles and the counts against the observed statistics (kernels_roast.hip).  A z is made whole
// on one device by one chain, and the counts are integers added under the lock: every sharding has the one-device bits.
// Shard 0 also leaves the hyperparameters, the set sizes and the members beyond -+sqrt(2) for roast_tail.
int roast_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t g = c.g, m = c.m, nfit = c.nfit, q = c.nq, p = c.ncoef, n = c.n, nrot = c.nrot;
  const size_t R = (size_t)g, M = (size_t)m, ncol = (size_t)nfit * q;
  const int64_t ld = even_ld(g), W1 = (int64_t)nfit * (p + 1);
  const int64_t ntile = ((int64_t)nrot + 63) / 64, ldw = ((int64_t)nrot + 15) / 16 * 16;
  const int64_t t_lo = ntile * k / ndev, t_hi = ntile * (k + 1) / ndev;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    PH_HIP(hipSetDevice(ctx->device));
    if (t_hi == t_lo && k != 0) return PLAIDHIP_OK;   // (no tile: nothing to add; shard 0 still makes what the tail reads)
    // ---- plaid.limma's two passes over all samples, as the one-device call makes them ----
    CtxBuf dA{ctx, 0}, dR{ctx, 3}, dZ{ctx, 4};
    DevBuf dQ, duse, dinvn, dmask, dwt, dws, drows;
    PH_TRY(drows.alloc((size_t)W1 * R * 3 * 8));   // [a 0.0 seed | the effects | the RSS]
    double *d_seed = drows.as<double>(), *d_E = d_seed + W1 * R, *d_rss = d_E + W1 * R;
    PH_HIP(hipMemsetAsync(d_seed, 0, (size_t)W1 * R * 8, ctx->stream));
    PH_TRY(dQ.alloc(c.lm_Q.size() * 8));
    PH_HIP(hipMemcpyAsync(dQ.p, c.lm_Q.data(), c.lm_Q.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (c.use != nullptr) {
      PH_TRY(duse.alloc((size_t)n * nfit));
      PH_HIP(hipMemcpyAsync(duse.p, c.use, (size_t)n * nfit, hipMemcpyHostToDevice, ctx->stream));
    }
    PH_TRY(dinvn.alloc((size_t)nfit * 8));
    PH_HIP(hipMemcpyAsync(dinvn.p, c.lm_invn.data(), (size_t)nfit * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dmask.alloc((size_t)lmfit_mask_bytes(n, W1)));
    PH_TRY(dwt.alloc((size_t)lmfit_weight_bytes(n, W1)));
    PH_TRY(launch_lmfit_masks(ctx, dQ.as<double>(), c.use != nullptr ? duse.as<int8_t>() : nullptr, dinvn.as<double>(), n, p, nfit,
                              dmask.p, dwt.as<double>()));
    PH_TRY(dws.alloc((size_t)row_design_ws_doubles(g, n, W1) * 8));
    PH_TRY(dA.alloc((size_t)ld * n * 8));
    PH_TRY(upload_pipelined(ctx, dA.as<char>(), (size_t)ld * 8, reinterpret_cast<const char*>(c.X), R * 8, n, nullptr));
    PH_TRY(launch_row_design_effects(ctx, dA.as<double>(), ld, g, n, dmask.p, dwt.as<double>(), (int32_t)W1, dws.as<double>()));
    PH_TRY(launch_reduce_blocks_flat(ctx, dws.as<double>(), W1 * g, n, d_seed, d_E));
    PH_TRY(launch_row_design_rss(ctx, dA.as<double>(), ld, g, n, dQ.as<double>(), dmask.p, p, nfit, d_E, dws.as<double>()));
    PH_TRY(launch_reduce_blocks_flat(ctx, dws.as<double>(), (int64_t)nfit * g, n, d_seed, d_rss));
    std::vector<double> E((size_t)W1 * R), rss((size_t)nfit * R), tab(R * 6 * ncol), hyp((size_t)nfit * 4);
    PH_HIP(hipMemcpyAsync(E.data(), d_E, E.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(rss.data(), d_rss, rss.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    PH_TRY(plaidhip_limma_finish(g, p, nfit, q, E.data(), rss.data(), c.lm_nf.data(), c.lm_v.data(), c.lm_u.data(), tab.data(),
                                 hyp.data()));
    // ---- the universe of every fit, and the pattern of the members inside it ----
    std::vector<double> cg(R * nfit);
    std::vector<std::vector<int32_t>> Gpf((size_t)nfit), Gif((size_t)nfit);
    for (int32_t f = 0; f < nfit; ++f) {
      const double* sigma2 = tab.data() + ((size_t)f * q * 6 + 5) * R;   // (of the fit's first contrast: NaN = not ok)
      double uni = 0.0, capped = 0.0;
      for (size_t r = 0; r < R; ++r) {
        cg[R * f + r] = std::isnan(sigma2[r]) ? nan : 1.0;
        uni += std::isnan(sigma2[r]) ? 0.0 : 1.0;
      }
      std::vector<int32_t>& gp = Gpf[(size_t)f];
      std::vector<int32_t>& gi = Gif[(size_t)f];
      gp.assign(M + 1, 0);
      for (int32_t st = 0; st < m; ++st) {
        for (int32_t e = c.Gp[st]; e < c.Gp[st + 1]; ++e)
          if (!std::isnan(sigma2[c.Gi[e]])) gi.push_back(c.Gi[e]);
        gp[(size_t)st + 1] = (int32_t)gi.size();
        const int32_t ms = gp[(size_t)st + 1] - gp[(size_t)st];
        if (k == 0) sh.roast.msize[M * f + st] = (double)ms;
        if (c.set_statistic == PLAIDHIP_ROAST_STAT_MEAN50 && ms > PLAIDHIP_ROAST_MEAN50_MAX) capped = 1.0;
      }
      if (k == 0) {
        for (int h = 0; h < 4; ++h) sh.roast.hyper[7 * (size_t)f + h] = hyp[4 * (size_t)f + h];
        sh.roast.hyper[7 * (size_t)f + 4] = uni;
        sh.roast.hyper[7 * (size_t)f + 5] = (double)nrot;
        sh.roast.hyper[7 * (size_t)f + 6] = capped;
      }
    }
    // ---- the shard's tiles ----
    const int64_t mine = std::max<int64_t>(t_hi - t_lo, 1);
    const int64_t ctile = std::max<int64_t>(1, std::min<int64_t>(mine, PLAIDHIP_ROAST_Z_BYTES / ((int64_t)R * 64 * 8)));
    DevBuf dcg, dW, dGp, dGi, dsel, dbeta, dt, dZo, dobs, dcnt;
    PH_TRY(dR.alloc((size_t)ld * n * 8));
    PH_TRY(dZ.alloc((size_t)ctile * R * 64 * 8));
    PH_TRY(dcg.alloc(cg.size() * 8));
    PH_HIP(hipMemcpyAsync(dcg.p, cg.data(), cg.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dW.alloc((size_t)(n + 1) * ldw * 8));
    PH_HIP(hipMemsetAsync(dW.p, 0, (size_t)(n + 1) * ldw * 8, ctx->stream));
    PH_TRY(dGp.alloc((M + 1) * 4));
    PH_TRY(dGi.alloc(std::max<size_t>((size_t)c.Gp[m], 1) * 4));
    PH_TRY(dsel.alloc(M * 4));
    PH_TRY(dbeta.alloc(R * 8));
    PH_TRY(dt.alloc(R * 8));
    PH_TRY(dZo.alloc(R * 64 * 8));
    PH_TRY(dobs.alloc(M * 4 * 8));
    PH_TRY(dcnt.alloc(M * 4 * 4));
    std::vector<double> beta(R), zobs(R);
    std::vector<int32_t> sel(M), hcnt(M * 4);
    for (int32_t f = 0; f < nfit; ++f) {
      const std::vector<int32_t>& gp = Gpf[(size_t)f];
      const std::vector<int32_t>& gi = Gif[(size_t)f];
      PH_TRY(launch_fry_residuals(ctx, dA.as<double>(), ld, g, n, dQ.as<double>(), dmask.p, p, f, d_E, dcg.as<double>(),
                                  dR.as<double>(), ld));
      const double* Wh = c.rotations != nullptr ? c.rotations + (size_t)f * (n + 1) * nrot : sh.roast.W[(size_t)f].data();
      PH_HIP(hipMemcpy2DAsync(dW.p, (size_t)ldw * 8, Wh, (size_t)nrot * 8, (size_t)nrot * 8, (size_t)n + 1, hipMemcpyHostToDevice,
                              ctx->stream));
      PH_HIP(hipMemcpyAsync(dGp.p, gp.data(), (M + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
      if (!gi.empty()) PH_HIP(hipMemcpyAsync(dGi.p, gi.data(), gi.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      int32_t cls_cnt[3] = {0, 0, 0};
      if (c.set_statistic == PLAIDHIP_ROAST_STAT_MEAN50) {   // the sets, class after class
        size_t at = 0;
        for (int cls = 0; cls < 3; ++cls)
          for (int32_t st = 0; st < m; ++st)
            if (roast_mean50_class(gp[(size_t)st + 1] - gp[(size_t)st]) == cls) {
              sel[at++] = st;
              ++cls_cnt[cls];
            }
        PH_HIP(hipMemcpyAsync(dsel.p, sel.data(), M * 4, hipMemcpyHostToDevice, ctx->stream));
      }
      const RoastFit rf = roast_fit(hyp[4 * (size_t)f], hyp[4 * (size_t)f + 1], hyp[4 * (size_t)f + 2]);
      for (int32_t j = 0; j < q; ++j) {
        const size_t col = (size_t)f * q + j;
        const double* fc = tab.data() + col * 6 * R;
        const double uj = c.lm_u[col];
        for (size_t r = 0; r < R; ++r) beta[r] = cg[R * f + r] == 1.0 ? fc[r] / uj : nan;
        PH_HIP(hipMemcpyAsync(dbeta.p, beta.data(), R * 8, hipMemcpyHostToDevice, ctx->stream));
        PH_HIP(hipMemcpyAsync(dt.p, fc + 2 * R, R * 8, hipMemcpyHostToDevice, ctx->stream));
        PH_TRY(launch_roast_observed(ctx, dt.as<double>(), g, rf.nu, c.zscore, dZo.as<double>()));
        PH_TRY(launch_roast_stats(ctx, dZo.as<double>(), g, dGp.as<int32_t>(), dGi.as<int32_t>(), m, c.set_statistic, 0, 1, 1,
                                  dsel.as<int32_t>(), cls_cnt, dobs.as<double>(), nullptr, nullptr));
        PH_HIP(hipMemsetAsync(dcnt.p, 0, M * 4 * 4, ctx->stream));
        for (int64_t t0 = t_lo; t0 < t_hi; t0 += ctile) {
          const int32_t k0 = (int32_t)(t0 * 64), k1 = (int32_t)std::min<int64_t>(nrot, std::min(t0 + ctile, t_hi) * 64);
          PH_TRY(launch_roast_rotate(ctx, dR.as<double>(), ld, g, n, dbeta.as<double>(), d_rss + R * f, dW.as<double>(), ldw, k0,
                                     k1, rf, c.zscore, dZ.as<double>()));
          PH_TRY(launch_roast_stats(ctx, dZ.as<double>(), g, dGp.as<int32_t>(), dGi.as<int32_t>(), m, c.set_statistic, k0, k1, nrot,
                                    dsel.as<int32_t>(), cls_cnt, nullptr, dobs.as<double>(), dcnt.as<int32_t>()));
        }
        if (k == 0) PH_HIP(hipMemcpy2DAsync(zobs.data(), 8, dZo.p, 64 * 8, 8, R, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipMemcpyAsync(hcnt.data(), dcnt.p, M * 4 * 4, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));   // (beta and the lists above are the sources of this contrast's uploads)
        {
          std::lock_guard<std::mutex> lk(sh.mu);
          int32_t* tot = sh.roast.cnt.data() + col * 4 * M;
          for (size_t e = 0; e < 4 * M; ++e) tot[e] += hcnt[e];
        }
        if (k != 0) continue;
        const double cut = std::sqrt(2.0);
        for (size_t st = 0; st < M; ++st)
          for (int32_t e = gp[st]; e < gp[st + 1]; ++e) {
            const double z = zobs[(size_t)gi[(size_t)e]];
            sh.roast.ndown[col * M + st] += z < -cut ? 1.0 : 0.0;
            sh.roast.nup[col * M + st] += z > cut ? 1.0 : 0.0;
          }
      }
    }
    return PLAIDHIP_OK;
  });
  return s.finish();
}

// sizes plaid.roast's part of Shared; the generated rotations of every fit are made here, once, before the workers
void roast_prepare(Shared& sh, const Call& c, int) {
  const size_t M = (size_t)c.m, ncol = (size_t)c.nfit * c.nq;
  sh.roast.cnt.assign(4 * M * ncol, 0);
  sh.roast.ndown.assign(M * ncol, 0.0);
  sh.roast.nup.assign(M * ncol, 0.0);
  sh.roast.msize.assign(M * c.nfit, 0.0);
  sh.roast.hyper.assign((size_t)c.nfit * 7, 0.0);
  sh.roast.W.assign((size_t)c.nfit, std::vector<double>());
  if (c.rotations != nullptr) return;
  for (int32_t f = 0; f < c.nfit; ++f) {
    sh.roast.W[(size_t)f].resize((size_t)(c.n + 1) * c.nrot);
    roast_rotations(c.lm_Q.data() + (size_t)f * c.n * c.ncoef, c.n, c.ncoef, c.use != nullptr ? c.use + (size_t)f * c.n : nullptr, f,
                    c.nrot, c.roast_seed, sh.roast.W[(size_t)f].data());
  }
}

// plaid.roast after the workers: the tables from the summed counts (plaidhip_roast_finish), on the host
int roast_tail(plaidhip_ctx*, const Call& c, Shared& sh) {
  PH_TRY(plaidhip_roast_finish(c.m, c.nfit, c.nq, c.nrot, c.set_statistic, c.midp, sh.roast.cnt.data(), sh.roast.msize.data(),
                               sh.roast.ndown.data(), sh.roast.nup.data(), c.out));
  std::copy(sh.roast.hyper.begin(), sh.roast.hyper.end(), c.hyper);
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
