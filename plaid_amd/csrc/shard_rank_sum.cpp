// plaid / replaid.sing / replaid.ssgsea on the sharded engine (shard.cpp).
#include "shard.h"

namespace plaidhip {

int shard_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
#ifdef PLAIDHIP_DIAG
  const auto t_trace0 = std::chrono::steady_clock::now();
#endif
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc;
  const int32_t g = c.g, m = c.m;
  const bool sparse = c.Xp != nullptr;
  const bool ranks = c.method != kPlaid;
  plaidhip_geneset* gs = nullptr;
  CtxBuf dX{ctx, 0}, dXp{ctx, 1}, dXi{ctx, 2}, dR{ctx, 3}, dS{ctx, 4}, dsmall{ctx, 5};
  // the caller's S is usually fresh, untouched memory (R: allocMatrix): its pages are made while the upload and the
  // kernels run, the copy home follows chunk by chunk (HomeBuffer, common.h)
  HomeBuffer home;
  const int64_t ldg = even_ld(g);
  uint32_t* d_flags = nullptr;
  double *d_red = nullptr, *d_med = nullptr, *d_colmax = nullptr, *d_gmax = nullptr;
  const int64_t zx = s.zx;
  int32_t max_nnz = 0;
  std::vector<int32_t> ploc;

  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    PH_TRY(acquire_geneset(ctx, g, m, c.Gp, c.Gi, &gs));
    PH_TRACE("geneset acquired");
    PH_TRY(dsmall.alloc(64 + (size_t)std::max(nloc, 1) * 16));
    d_flags = dsmall.as<uint32_t>();
    d_red = reinterpret_cast<double*>(dsmall.as<char>() + 16);
    d_gmax = d_red + 2;
    d_med = reinterpret_cast<double*>(dsmall.as<char>() + 64);
    d_colmax = d_med + std::max(nloc, 1);
    PH_HIP(hipMemsetAsync(dsmall.p, 0, 64, ctx->stream));
    PH_TRY(dS.alloc((size_t)m * std::max(nloc, 1) * 8));
    if (nloc == 0) return PLAIDHIP_OK;
    if (!sparse) {
      PH_TRY(dX.alloc((size_t)ldg * nloc * 8));
      if (ranks) PH_TRY(dR.alloc((size_t)ldg * nloc * 8));
      const double* Xh = c.X + (int64_t)lo * g;
      // the kernels of a column panel follow its DMA: the crossprod itself for plaid(), the ranks for the others
      // (their crossprod needs max(rX) of ALL columns first, R/plaid.R:251)
      auto on_panel = [&](int64_t c0, int64_t c1) -> int {
        const int32_t nc = (int32_t)(c1 - c0);
        const double* xp = dX.as<double>() + c0 * ldg;
        if (c.method == kPlaid)
          return launch_spmm_dense_f64(ctx, gs, xp, ldg, nc, c.stat, 1.0, nullptr, 0.0, dS.as<double>() + c0 * m, m, d_flags);
        return launch_colranks_dense_f64(ctx, xp, ldg, g, nc, c.method == kSing ? PLAIDHIP_TIES_MIN : PLAIDHIP_TIES_AVERAGE, 0,
                                         c.method == kSsgsea ? 1.0 + c.alpha : 1.0, dR.as<double>() + c0 * ldg, ldg,
                                         c.method == kSsgsea ? d_colmax + c0 : nullptr);
      };
      PH_TRACE("buffers ready");
      PH_TRY(upload_pipelined(ctx, dX.as<char>(), (size_t)ldg * 8, reinterpret_cast<const char*>(Xh), (size_t)g * 8, nloc,
                              on_panel));
      PH_TRACE("upload enqueued");
      // (the result's pages are made from here on, not earlier: eight threads faulting pages in next to the four feeder
      // threads cost the upload a quarter of its rate)
      home.prepare(c.S_out + (int64_t)lo * m, (size_t)m * nloc * 8);
    } else {
      PH_TRY(upload_csc_shard(s, ploc, dXp, dXi, dX, &max_nnz));
      // replaid.sing ranks the zeros too (colranks' sparse branch without keep.zero, R/plaid.R:602-609: a dense rank
      // matrix): built panel by panel from the ranks of the stored values, each panel multiplied at once
      int64_t panel = ((int64_t)2 << 30) / (ldg * 8);
      panel = std::min<int64_t>(std::max<int64_t>(panel & ~(int64_t)1, 2), nloc);
      if (c.method == kSing) PH_TRY(dR.alloc((size_t)(panel * ldg + zx) * 8));   // a panel of dense ranks | ranks of the stored values
      else if (ranks) PH_TRY(dR.alloc((size_t)zx * 8));
      home.prepare(c.S_out + (int64_t)lo * m, (size_t)m * nloc * 8);
      if (c.method == kSing) {
        double* dRd = dR.as<double>();
        double* dRx = dRd + panel * ldg;
        const bool by_stored = max_nnz <= max_sparse_rank_column();
        for (int64_t c0 = 0; c0 < nloc; c0 += panel) {
          const int32_t nc = (int32_t)std::min<int64_t>(panel, nloc - c0);
          const int32_t* xp = dXp.as<int32_t>() + c0;          // (absolute offsets into the shard's @i / @x)
          if (by_stored)
            PH_TRY(launch_colranks_csc_dense_nz_f64(ctx, xp, dXi.as<int32_t>(), dX.as<double>(), g, nc, max_nnz,
                                                    PLAIDHIP_TIES_MIN, 0, 1.0, dRx, dRd, ldg, nullptr));
          else   // a column with more stored values than one pass ranks: densify and rank
            PH_TRY(launch_colranks_csc_dense_f64(ctx, xp, dXi.as<int32_t>(), dX.as<double>(), g, nc, PLAIDHIP_TIES_MIN, 0, 1.0,
                                                 dRd, ldg, nullptr));
          PH_TRY(launch_spmm_dense_f64(ctx, gs, dRd, ldg, nc, PLAIDHIP_STAT_MEAN, 1.0 / (double)g, nullptr, -0.5,   // R/plaid.R:216
                                       dS.as<double>() + c0 * m, m, d_flags, PLAIDHIP_X_RANKS));
        }
      } else if (ranks)   // sparse_colranks: the stored values among themselves (R/plaid.R:600-601, 631-650)
        PH_TRY(launch_colranks_csc_f64(ctx, dXp.as<int32_t>(), dX.as<double>(), nloc, max_nnz,
                                       c.method == kSing ? PLAIDHIP_TIES_MIN : PLAIDHIP_TIES_AVERAGE, 0,
                                       c.method == kSsgsea ? 1.0 + c.alpha : 1.0, dR.as<double>(), c.method == kSsgsea ? d_colmax : nullptr));
    }
    return PLAIDHIP_OK;
  });

  // ---- max(rX) over every shard (replaid.ssgsea, R/plaid.R:251) ----------------------------------------------------
  double gmax = 0.0;
  if (c.method == kSsgsea) {
    double mine = sparse ? 0.0 : -INFINITY;      // a dgCMatrix has implicit zeros
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      PH_TRY(launch_max(ctx, d_colmax, nloc, d_gmax));
      PH_HIP(hipMemcpyAsync(&mine, d_gmax, 8, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      return PLAIDHIP_OK;
    });
    {
      std::lock_guard<std::mutex> lk(sh.mu);
      if (nloc > 0 && s.rc == PLAIDHIP_OK) {
        sh.gmax = sh.gmax_set ? std::max(sh.gmax, mine) : mine;
        sh.gmax_set = true;
      }
    }
    sh.rv.arrive_and_wait();
    gmax = sh.gmax;
  }

  // ---- crossprod of the rank-based callers (plaid() did it per panel) ------------------------------------------------
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (nloc == 0) return PLAIDHIP_OK;
    if (c.method == kPlaid && !sparse) return PLAIDHIP_OK;
    if (c.method == kSing && sparse) return PLAIDHIP_OK;   // done panel by panel above
    double a = 1.0, b = 0.0;
    int stat = c.stat;
    if (c.method == kSing) { a = 1.0 / (double)g; b = -0.5; stat = PLAIDHIP_STAT_MEAN; }       // R/plaid.R:216
    if (c.method == kSsgsea) { a = 1.0 / gmax; b = -0.5; stat = PLAIDHIP_STAT_MEAN; }            // R/plaid.R:251
    const double* vals = ranks ? dR.as<double>() : dX.as<double>();
    if (sparse) {
      // scatter or gather is chosen from the density of the WHOLE matrix, not of the shard: every sharding of the same
      // call takes the same kernel (the gather kernels are then bit-identical across shardings; the scatter kernel adds
      // in arrival order and agrees to the last bits only, as it does from run to run -- and its fixed-point grid, where
      // the column-sum bound picks it, follows the SHARD's largest column sum: 2^-40 relative across shardings)
      const int64_t nnz_choice = (int64_t)((double)c.Xp[c.n] / (double)c.n * (double)nloc);
      // replaid.ssgsea: the values are rank weights in [0, max(rX)] (the scatter kernel may sum them in fixed point)
      // (normalised results: the crossprod also classifies its scores for the medians below, launch_col_medians_resume)
      const bool will_norm = c.method == kSsgsea || (c.method == kPlaid && c.normalize);
      if (will_norm)
        return launch_spmm_csc_fused_f64(ctx, gs, dXp.as<int32_t>(), dXi.as<int32_t>(), vals, nloc, zx, stat, a, nullptr, b,
                                         dS.as<double>(), m, d_flags, /*bounded=*/c.method == kSsgsea, nullptr, gmax, nnz_choice);
      return launch_spmm_csc_f64(ctx, gs, dXp.as<int32_t>(), dXi.as<int32_t>(), vals, nloc, nnz_choice, stat, a, nullptr, b,
                                 dS.as<double>(), m, d_flags, /*bounded=*/c.method == kSsgsea, nullptr, gmax);
    }
    const int x_kind = (c.method == kSing || (c.method == kSsgsea && c.alpha == 0.0)) ? PLAIDHIP_X_RANKS : PLAIDHIP_X_ANY;
    // (normalised results on the fp64 pair kernel: the crossprod also classifies its scores for the medians below)
    if (c.method == kSsgsea || (c.method == kPlaid && c.normalize))
      return launch_spmm_dense_fused_f64(ctx, gs, vals, ldg, nloc, stat, a, nullptr, b, dS.as<double>(), m, d_flags, x_kind);
    return launch_spmm_dense_f64(ctx, gs, vals, ldg, nloc, stat, a, nullptr, b, dS.as<double>(), m, d_flags, x_kind);
  });

  // ---- normalize_medians (R/plaid.R:554-575): two more scalars --------------------------------------------------------
  const bool norm = c.method == kSsgsea || (c.method == kPlaid && c.normalize);
  if (norm) {
    const double mean_med = medians_and_their_mean(s, dS.as<double>(), d_flags, d_med);
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      return launch_shift_columns(ctx, dS.as<double>(), m, m, nloc, d_med, mean_med, nullptr);
    });
  }

  // ---- the score shard goes home (pageable destination: the runtime's own staging runs at ~53 GB/s) ---------------------
  PH_TRACE("normalise enqueued");
  s.step([&]() -> int {
    if (nloc > 0) PH_TRY(home.copy(ctx, dS.p));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    PH_TRACE("scores home");
    return PLAIDHIP_OK;
  });
  return s.finish();
}

}  // namespace plaidhip
