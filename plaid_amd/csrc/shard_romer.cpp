// plaid.romer on the sharded engine (shard.cpp).
#include "shard.h"
#include "romer.h"

namespace plaidhip {

namespace {
// the prepared collection of one fit's pattern inside the universe (the rank crossprod of mean and floormean)
struct GenesetGuard {
  plaidhip_geneset* gs = nullptr;
  ~GenesetGuard() { reset(); }
  void reset() {
    if (gs != nullptr) plaidhip_geneset_destroy(gs);
    gs = nullptr;
  }
};
}  // namespace

// plaid.romer (include/plaidhip.h: plaidhip_romer).  As roast_worker: the ROTATIONS are dealt to the shards in whole tiles of
// 64, shard k takes tiles [ntile k / ndev, ntile (k + 1) / ndev); every shard takes all of X, runs plaid.limma's two passes
// itself with the operations and the order of the one-device call, and makes the shrink factors on the host from the same
// bits; no rendezvous.  Then, per fit and contrast: the observed sides from a one-column key matrix, and chunk after chunk
// of whole tiles the rotated t (roast_rotate_kernel without a z-score), the keys over the universe, their average ranks and the
// counts against the observed sides (kernels_romer.hip; mean and floormean through the rank crossprod on a collection prepared
// from the fit's pattern inside the universe).  The sides are integers and the counts are added under the lock: every
// sharding has the one-device bits.  Shard 0 also leaves the hyperparameters and the set sizes for romer_tail.
int romer_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  s.force_f64();   // (the rank crossprod is exact integer sums in every mode; said so)
  const int32_t g = c.g, m = c.m, nfit = c.nfit, q = c.nq, p = c.ncoef, n = c.n, nrot = c.nrot, stat = c.set_statistic;
  const size_t R = (size_t)g, M = (size_t)m, ncol = (size_t)nfit * q, H = 8 + (size_t)q;
  const int64_t ld = even_ld(g), W1 = (int64_t)nfit * (p + 1);
  const int64_t ntile = ((int64_t)nrot + 63) / 64, ldw = ((int64_t)nrot + 15) / 16 * 16;
  const int64_t t_lo = ntile * k / ndev, t_hi = ntile * (k + 1) / ndev;
  const int nkeys = romer_nkeys(stat);
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
    // ---- the buffers of one fit; the chunk is sized for the largest universe there can be (all rows) ----
    const int64_t ldu_max = ((int64_t)g + 15) / 16 * 16;
    const bool cross = stat != PLAIDHIP_ROMER_STAT_MEAN50;   // the sides by the rank crossprod
    const int64_t per_rot = (int64_t)R * 8 + ldu_max * 16 * nkeys + (cross ? (int64_t)M * 8 * nkeys : 0);   // t, keys, ranks, sums
    const int64_t mine = std::max<int64_t>(t_hi - t_lo, 1);
    const int64_t ctile = std::max<int64_t>(1, std::min<int64_t>(mine, PLAIDHIP_ROAST_Z_BYTES / (64 * per_rot)));
    const size_t ckeys = (size_t)ctile * 64 * (size_t)ldu_max;   // entries of one key matrix of a chunk
    DevBuf dcg, dW, dGp, dGi, dsel, duidx, dbeta, dt, dZo, dK, dRd, dS, dKo, dRdo, dobs, dcnt, dflag;
    std::vector<double> cg(R * nfit);
    for (int32_t f = 0; f < nfit; ++f) {
      const double* sigma2 = tab.data() + ((size_t)f * q * 6 + 5) * R;   // (of the fit's first contrast: NaN = not ok)
      for (size_t r = 0; r < R; ++r) cg[R * f + r] = std::isnan(sigma2[r]) ? nan : 1.0;
    }
    PH_TRY(dR.alloc((size_t)ld * n * 8));
    PH_TRY(dZ.alloc((size_t)ctile * R * 64 * 8));
    PH_TRY(dcg.alloc(cg.size() * 8));
    PH_HIP(hipMemcpyAsync(dcg.p, cg.data(), cg.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dW.alloc((size_t)(n + 1) * ldw * 8));
    PH_HIP(hipMemsetAsync(dW.p, 0, (size_t)(n + 1) * ldw * 8, ctx->stream));
    PH_TRY(dGp.alloc((M + 1) * 4));
    PH_TRY(dGi.alloc(std::max<size_t>((size_t)c.Gp[m], 1) * 4));
    PH_TRY(dsel.alloc(M * 4));
    PH_TRY(duidx.alloc(R * 4));
    PH_TRY(dbeta.alloc(R * 8));
    PH_TRY(dt.alloc(R * 8));
    PH_TRY(dZo.alloc(R * 64 * 8));
    PH_TRY(dK.alloc(ckeys * 8 * nkeys));
    PH_TRY(dRd.alloc(ckeys * 8 * nkeys));
    PH_TRY(dS.alloc(std::max<size_t>(cross ? (size_t)ctile * 64 * M * nkeys : 0, 3 * M) * 8));
    PH_TRY(dKo.alloc((size_t)ldu_max * 8 * 3));
    PH_TRY(dRdo.alloc((size_t)ldu_max * 8 * 3));
    PH_TRY(dobs.alloc(M * 3 * 8));
    PH_TRY(dcnt.alloc(M * 3 * 4));
    PH_TRY(dflag.alloc(4));
    std::vector<double> beta(R), tu, cu;
    std::vector<int32_t> sel, hcnt(M * 3), uidx, pos(R), gp(M + 1), gi;
    for (int32_t f = 0; f < nfit; ++f) {
      // ---- the universe, and the pattern of the members inside it by their place there ----
      uidx.clear();
      for (size_t r = 0; r < R; ++r) {
        pos[r] = cg[R * f + r] == 1.0 ? (int32_t)uidx.size() : -1;
        if (pos[r] >= 0) uidx.push_back((int32_t)r);
      }
      const int32_t U = (int32_t)uidx.size();
      const int64_t ldu = ((int64_t)U + 15) / 16 * 16;
      gi.clear();
      gp[0] = 0;
      double capped = 0.0;
      for (int32_t st = 0; st < m; ++st) {
        for (int32_t e = c.Gp[st]; e < c.Gp[st + 1]; ++e)
          if (pos[(size_t)c.Gi[e]] >= 0) gi.push_back(pos[(size_t)c.Gi[e]]);
        gp[(size_t)st + 1] = (int32_t)gi.size();
        const int32_t ms = gp[(size_t)st + 1] - gp[(size_t)st];
        if (k == 0) sh.romer.msize[M * f + st] = U == 0 ? 0.0 : (double)ms;
        if (stat == PLAIDHIP_ROMER_STAT_MEAN50 && ms > PLAIDHIP_ROAST_MEAN50_MAX) capped = 1.0;
      }
      double* hy = sh.romer.hyper.data() + H * (size_t)f;
      if (k == 0) {
        for (int h = 0; h < 4; ++h) hy[h] = hyp[4 * (size_t)f + h];
        hy[4] = (double)U;
        hy[5] = (double)nrot;
        hy[6] = capped;   // (hy[7], the NaN flag, and pi of every contrast start at 0.0: romer_prepare)
      }
      if (U == 0) continue;   // (every count stays 0 and every set size 0: NaN rows but NGenes)
      GenesetGuard prepared;
      if (cross) PH_TRY(plaidhip_geneset_create(ctx, U, m, gp.data(), gi.data(), &prepared.gs));
      PH_TRY(launch_fry_residuals(ctx, dA.as<double>(), ld, g, n, dQ.as<double>(), dmask.p, p, f, d_E, dcg.as<double>(),
                                  dR.as<double>(), ld));
      const double* Wh = c.rotations != nullptr ? c.rotations + (size_t)f * (n + 1) * nrot : sh.roast.W[(size_t)f].data();
      PH_HIP(hipMemcpy2DAsync(dW.p, (size_t)ldw * 8, Wh, (size_t)nrot * 8, (size_t)nrot * 8, (size_t)n + 1, hipMemcpyHostToDevice,
                              ctx->stream));
      PH_HIP(hipMemcpyAsync(dGp.p, gp.data(), (M + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
      if (!gi.empty()) PH_HIP(hipMemcpyAsync(dGi.p, gi.data(), gi.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      PH_HIP(hipMemcpyAsync(duidx.p, uidx.data(), (size_t)U * 4, hipMemcpyHostToDevice, ctx->stream));
      PH_HIP(hipMemsetAsync(dflag.p, 0, 4, ctx->stream));
      int32_t cls_cnt[2] = {0, 0};
      if (stat == PLAIDHIP_ROMER_STAT_MEAN50) {
        romer_mean50_classes(gp.data(), m, sel, cls_cnt);
        if (!sel.empty()) PH_HIP(hipMemcpyAsync(dsel.p, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      }
      const RoastFit rf = roast_fit(hyp[4 * (size_t)f], hyp[4 * (size_t)f + 1], hyp[4 * (size_t)f + 2]);
      double* Ko = dKo.as<double>();
      double* Ro = dRdo.as<double>();
      double* Kc = dK.as<double>();
      double* Rc = dRd.as<double>();
      auto rank = [&](const double* key, int32_t nk, double* to) {
        return launch_colranks_dense_f64(ctx, key, ldu, U, nk, PLAIDHIP_TIES_AVERAGE, 0, 1.0, to, ldu, nullptr);
      };
      const size_t kst = ckeys;   // the stride between the chunk's key matrices
      for (int32_t j = 0; j < q; ++j) {
        const size_t col = (size_t)f * q + j;
        const double* fc = tab.data() + col * 6 * R;
        const double uj = c.lm_u[col];
        // ---- the shrink factors: the caller's, or from the universe's moderated t on the host, or 1.0 ----
        cu.assign((size_t)U, 1.0);
        if (c.shrink != nullptr) {
          for (int32_t i = 0; i < U; ++i) cu[(size_t)i] = c.shrink[col * R + (size_t)uidx[(size_t)i]];
        } else if (c.shrink_resid) {
          tu.resize((size_t)U);
          for (int32_t i = 0; i < U; ++i) tu[(size_t)i] = fc[2 * R + (size_t)uidx[(size_t)i]];
          double prop = 0.0;
          PH_TRY(plaidhip_romer_shrink(U, tu.data(), uj, rf.s02, rf.df0 + rf.d, cu.data(), &prop));
          if (k == 0) hy[8 + j] = prop;
        }
        for (size_t r = 0; r < R; ++r) beta[r] = pos[r] >= 0 ? fc[r] / uj * cu[(size_t)pos[r]] : nan;
        PH_HIP(hipMemcpyAsync(dbeta.p, beta.data(), R * 8, hipMemcpyHostToDevice, ctx->stream));
        PH_HIP(hipMemcpyAsync(dt.p, fc + 2 * R, R * 8, hipMemcpyHostToDevice, ctx->stream));
        // ---- the observed sides: plaid.limma's moderated t itself as a one-column key matrix ----
        PH_TRY(launch_roast_observed(ctx, dt.as<double>(), g, rf.nu, PLAIDHIP_ROAST_ZSCORE_NONE, dZo.as<double>()));
        PH_TRY(launch_romer_keys(ctx, dZo.as<double>(), g, duidx.as<int32_t>(), U, ldu, stat, 1, Ko, Ko + ldu_max, Ko + 2 * ldu_max,
                                 dflag.as<uint32_t>()));
        PH_TRY(rank(Ko, 1, Ro));
        if (nkeys == 3) PH_TRY(rank(Ko + ldu_max, 1, Ro + ldu_max));
        PH_TRY(rank(Ko + 2 * ldu_max, 1, Ro + 2 * ldu_max));
        PH_HIP(hipMemsetAsync(dobs.p, 0, M * 3 * 8, ctx->stream));
        PH_TRY(launch_romer_sides(ctx, prepared.gs, Ro, Ro + ldu_max, Ro + 2 * ldu_max, ldu, U, dGp.as<int32_t>(),
                                  dGi.as<int32_t>(), m, stat, 1, 0, 1, dsel.as<int32_t>(), cls_cnt, dS.as<double>(),
                                  dobs.as<int64_t>(), nullptr, nullptr));
        PH_HIP(hipMemsetAsync(dcnt.p, 0, M * 3 * 4, ctx->stream));
        // ---- the shard's tiles, chunk after chunk ----
        for (int64_t t0 = t_lo; t0 < t_hi; t0 += ctile) {
          const int32_t k0 = (int32_t)(t0 * 64), k1 = (int32_t)std::min<int64_t>(nrot, std::min(t0 + ctile, t_hi) * 64);
          const int32_t nk = k1 - k0;
          PH_TRY(launch_roast_rotate(ctx, dR.as<double>(), ld, g, n, dbeta.as<double>(), d_rss + R * f, dW.as<double>(), ldw, k0,
                                     k1, rf, PLAIDHIP_ROAST_ZSCORE_NONE, dZ.as<double>()));
          PH_TRY(launch_romer_keys(ctx, dZ.as<double>(), g, duidx.as<int32_t>(), U, ldu, stat, nk, Kc, Kc + kst, Kc + (nkeys - 1) * kst,
                                   dflag.as<uint32_t>()));
          for (int e = 0; e < nkeys; ++e) PH_TRY(rank(Kc + e * kst, nk, Rc + e * kst));
          PH_TRY(launch_romer_sides(ctx, prepared.gs, Rc, Rc + kst, Rc + (nkeys - 1) * kst, ldu, U, dGp.as<int32_t>(),
                                    dGi.as<int32_t>(), m, stat, nk, k0, nrot, dsel.as<int32_t>(), cls_cnt, dS.as<double>(), nullptr,
                                    dobs.as<int64_t>(), dcnt.as<int32_t>()));
        }
        PH_HIP(hipMemcpyAsync(hcnt.data(), dcnt.p, M * 3 * 4, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));   // (beta and the lists above are the sources of this contrast's uploads)
        std::lock_guard<std::mutex> lk(sh.mu);
        int32_t* tot = sh.romer.cnt.data() + col * 3 * M;
        for (size_t e = 0; e < 3 * M; ++e) tot[e] += hcnt[e];
      }
      uint32_t flag = 0;
      PH_HIP(hipMemcpy(&flag, dflag.p, 4, hipMemcpyDeviceToHost));
      if (flag != 0) {
        std::lock_guard<std::mutex> lk(sh.mu);
        hy[7] = 1.0;
      }
    }
    return PLAIDHIP_OK;
  });
  return s.finish();
}

// sizes plaid.romer's part of Shared; the generated rotations of every fit are made here, once, before the workers
void romer_prepare(Shared& sh, const Call& c, int) {
  const size_t M = (size_t)c.m, ncol = (size_t)c.nfit * c.nq;
  sh.romer.cnt.assign(3 * M * ncol, 0);
  sh.romer.msize.assign(M * c.nfit, 0.0);
  sh.romer.hyper.assign((size_t)c.nfit * (8 + (size_t)c.nq), 0.0);
  sh.roast.W.assign((size_t)c.nfit, std::vector<double>());
  if (c.rotations != nullptr) return;
  for (int32_t f = 0; f < c.nfit; ++f) {
    sh.roast.W[(size_t)f].resize((size_t)(c.n + 1) * c.nrot);
    roast_rotations(c.lm_Q.data() + (size_t)f * c.n * c.ncoef, c.n, c.ncoef, c.use != nullptr ? c.use + (size_t)f * c.n : nullptr, f,
                    c.nrot, c.roast_seed, sh.roast.W[(size_t)f].data());
  }
}

// plaid.romer after the workers: the tables from the summed counts (plaidhip_romer_finish), on the host
int romer_tail(plaidhip_ctx*, const Call& c, Shared& sh) {
  PH_TRY(plaidhip_romer_finish(c.m, c.nfit, c.nq, c.nrot, c.set_statistic, sh.romer.cnt.data(), sh.romer.msize.data(), c.out));
  std::copy(sh.romer.hyper.begin(), sh.romer.hyper.end(), c.hyper);
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
