// The exact scorers on the sharded engine (shard.cpp): replaid.ssgsea.exact, replaid.sing.exact, replaid.ucell.exact and
// replaid.aucell.exact.
#include "shard.h"

namespace plaidhip {

// one device's part of replaid.ssgsea.exact (kSsgseaExact, kernels_walk.hip): the operands of its columns, the crossprods
// C = G'Q (the exact rank route) and, for alpha != 0, A = G'P and B = G'W (fp64), the pinned epilogue.  The only coupling
// between the shards is the range of all scores behind norm = TRUE, combined on the host.
// single = FALSE: the same operands, then the walk kernel of kernels_ks.hip in place of the crossprods and the epilogue
// (P's columns, which it has no use for, take the weights in walk order).
int ssgsea_exact_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc;
  const int32_t g = c.g, m = c.m;
  const bool sparse = c.Xp != nullptr;
  const bool need_w = c.alpha != 0.0;
  const int64_t ld = g;
  // the scores are fp64 in every mode: the crossprods stay on the fp64 kernels whatever precision the context was given
  s.force_f64();
  plaidhip_geneset* gs = nullptr;
  // the large buffers stay with the context between calls (ctx_buffer), as the other scorers' do: operands [Q | W | P |
  // rank scratch] in one, scores [S | A | B] in another
  CtxBuf dX{ctx, 0}, dXp{ctx, 1}, dXi{ctx, 2}, dops{ctx, 3}, dS{ctx, 4}, dsmall{ctx, 5};
  DevBuf dk, dpart, dGp, dGi;
  HomeBuffer home;
  const bool ks = c.single == 0;
  double *Q = nullptr, *W = nullptr, *P = nullptr, *scratch = nullptr, *A = nullptr, *B = nullptr;
  uint32_t* d_colnan = nullptr;
  double* d_range = nullptr;   // {min, max, any NaN} of the shard's scores
  std::vector<int32_t> kset((size_t)m), ploc;
  for (int32_t j = 0; j < m; ++j) kset[(size_t)j] = c.Gp[j + 1] - c.Gp[j];   // members after the alignment

  // ---- upload, operands ---------------------------------------------------------------------------------------------------
  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    PH_TRY(acquire_geneset(ctx, g, m, c.Gp, c.Gi, &gs));
    const size_t nl = (size_t)std::max(nloc, 1);
    PH_TRY(dsmall.alloc(64 + nl * 4));
    d_range = dsmall.as<double>();
    d_colnan = reinterpret_cast<uint32_t*>(dsmall.as<char>() + 64);
    const size_t nscores = (size_t)m * nl;
    PH_TRY(dS.alloc(nscores * 8 * (need_w && !ks ? 3 : 1)));
    if (nloc == 0) return PLAIDHIP_OK;
    if (ks) PH_TRY(upload_pattern(ctx, c.Gp, c.Gi, m, dGp, dGi));
    if (need_w && !ks) {
      A = dS.as<double>() + nscores;
      B = A + nscores;
    }
    PH_TRY(dk.alloc((size_t)m * 4));
    PH_HIP(hipMemcpyAsync(dk.p, kset.data(), (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dpart.alloc((size_t)score_part_blocks(ctx, (int64_t)m * nloc) * 24));
    const int64_t zx = s.zx;
    const size_t col = (size_t)ld * nloc;
    const size_t nscratch = sparse ? 3 * (size_t)std::max<int64_t>(zx, 1) : 2 * col;
    PH_TRY(dops.alloc((col * (need_w ? 3 : 1) + nscratch) * 8));
    Q = dops.as<double>();
    if (need_w) {
      W = Q + col;
      P = W + col;
    }
    scratch = Q + col * (need_w ? 3 : 1);
    if (!sparse) {
      PH_TRY(dX.alloc((size_t)ld * nloc * 8));
      PH_TRY(upload_pipelined(ctx, dX.as<char>(), (size_t)ld * 8, reinterpret_cast<const char*>(c.X + (int64_t)lo * g),
                              (size_t)g * 8, nloc, nullptr));
      PH_TRY(launch_ssgsea_exact_operands(ctx, dX.as<double>(), ld, nullptr, nullptr, g, nloc, 0, 0, c.alpha, Q, W, P, ld, scratch,
                                          d_colnan));
    } else {
      int32_t max_nnz = 0;
      PH_TRY(upload_csc_shard(s, ploc, dXp, dXi, dX, &max_nnz));
      PH_TRY(launch_ssgsea_exact_operands(ctx, dX.as<double>(), 0, dXp.as<int32_t>(), dXi.as<int32_t>(), g, nloc, max_nnz, zx,
                                          c.alpha, Q, W, P, ld, scratch, d_colnan));
    }
    home.prepare(c.S_out + (int64_t)lo * m, (size_t)m * nloc * 8);
    return PLAIDHIP_OK;
  });

  // ---- crossprods, epilogue ---------------------------------------------------------------------------------------------
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (nloc == 0) return PLAIDHIP_OK;
    if (ks) {
      PH_TRY(launch_gsea_ks(ctx, Q, W, P, ld, d_colnan, g, nloc, dGp.as<int32_t>(), dGi.as<int32_t>(), m, c.alpha, c.scale,
                            dS.as<double>(), m));
      return launch_score_range(ctx, dS.as<double>(), m, m, nloc, dpart.as<double>(), d_range);
    }
    // q holds integers in [1, N]: the rank route's u16 staging when 2 N fits, integer sums either way
    const int xk = 2 * (int64_t)g < 65536 ? PLAIDHIP_X_RANKS : PLAIDHIP_X_ANY;
    PH_TRY(launch_spmm_dense_f64(ctx, gs, Q, ld, nloc, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0, dS.as<double>(), m, nullptr, xk));
    if (need_w) {
      PH_TRY(launch_spmm_dense_f64(ctx, gs, P, ld, nloc, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0, A, m, nullptr));
      PH_TRY(launch_spmm_dense_f64(ctx, gs, W, ld, nloc, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0, B, m, nullptr));
    }
    return launch_ssgsea_exact_epilogue(ctx, A, B, dS.as<double>(), m, m, nloc, dk.as<int32_t>(), g, c.scale, d_colnan,
                                        dpart.as<double>(), d_range);
  });

  // ---- norm: es / diff(range(es)) over the whole m x n result; one NaN anywhere makes every score NaN -------------------
  if (c.normalize) {
    double mm[3] = {INFINITY, -INFINITY, 0.0};
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      PH_HIP(hipMemcpyAsync(mm, d_range, 24, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      return PLAIDHIP_OK;
    });
    merge_range(s, mm[0], mm[1], mm[2] != 0.0);
    sh.rv.arrive_and_wait();
    const double range = sh.es_nan ? std::numeric_limits<double>::quiet_NaN() : sh.xmax - sh.xmin;
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      return launch_ssgsea_exact_norm(ctx, dS.as<double>(), m, m, nloc, range);
    });
  }

  // ---- the score shard goes home ----------------------------------------------------------------------------------------
  s.step([&]() -> int {
    if (nloc > 0) PH_TRY(home.copy(ctx, dS.p));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    return PLAIDHIP_OK;
  });
  return s.finish();
}

// one device's part of replaid.sing.exact (kSingExact, kernels_sing.hip): the min ranks of its columns as replaid.sing takes
// them (a dgCMatrix: the dense rank matrix built on the device), the crossprods C = G'R on the exact rank route and the
// pinned epilogue; for the dispersions the last ranks (a second rank pass over a tie-free column made from the first),
// the ranks by position and the per-pair kernel, once per direction.  Nothing couples the shards.
int sing_exact_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc;
  const int32_t g = c.g, m = c.m;
  const bool sparse = c.Xp != nullptr;
  const bool down = c.Dp != nullptr;
  const bool want_score = c.sx_out[0] || c.sx_out[1] || c.sx_out[2];
  const bool want_disp = c.sx_out[3] || c.sx_out[4] || c.sx_out[5];
  const int64_t ld = even_ld(g);   // replaid.sing's layout: the pair crossprod takes the ranks as it takes them there
  s.force_f64();
  plaidhip_geneset *gs_up = nullptr, *gs_dn = nullptr;
  CtxBuf dX{ctx, 0}, dXp{ctx, 1}, dXi{ctx, 2}, dops{ctx, 3}, dS{ctx, 4}, dsmall{ctx, 5};
  DevBuf dk, dGp, dGi, dDp, dDi;
  HomeBuffer home[6];
  double *R = nullptr, *Y = nullptr, *Q = nullptr, *Rx = nullptr;
  uint32_t* d_colnan = nullptr;
  const size_t nscores = (size_t)m * (size_t)std::max(nloc, 1);
  auto part = [&](int o) { return dS.as<double>() + (size_t)o * nscores; };   // [total | up | down] scores, then dispersions
  std::vector<int32_t> kset((size_t)m * 2, 0), ploc;
  for (int32_t j = 0; j < m; ++j) {   // members after the alignment
    kset[(size_t)j] = c.Gp[j + 1] - c.Gp[j];
    if (down) kset[(size_t)m + j] = c.Dp[j + 1] - c.Dp[j];
  }

  // ---- upload, NaN flags, min ranks; last ranks and the ranks by position --------------------------------------------------
  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    if (want_score) {
      PH_TRY(acquire_geneset(ctx, g, m, c.Gp, c.Gi, &gs_up));
      if (down) PH_TRY(acquire_geneset(ctx, g, m, c.Dp, c.Di, &gs_dn));
    }
    PH_TRY(dsmall.alloc((size_t)std::max(nloc, 1) * 4));
    d_colnan = dsmall.as<uint32_t>();
    PH_TRY(dS.alloc(nscores * 6 * 8));
    if (nloc == 0) return PLAIDHIP_OK;
    PH_TRY(dk.alloc((size_t)m * 2 * 4));
    PH_HIP(hipMemcpyAsync(dk.p, kset.data(), (size_t)m * 2 * 4, hipMemcpyHostToDevice, ctx->stream));
    if (want_disp) {
      PH_TRY(upload_pattern(ctx, c.Gp, c.Gi, m, dGp, dGi));
      if (down) PH_TRY(upload_pattern(ctx, c.Dp, c.Di, m, dDp, dDi));
    }
    const int64_t zx = s.zx;
    const size_t col = (size_t)ld * nloc;
    // [R | Y (then the ranks by position, u32) | Q] for the dispersions, R alone without; a dgCMatrix: the ranks of its
    // stored values behind them
    PH_TRY(dops.alloc((col * (want_disp ? 3 : 1) + (size_t)std::max<int64_t>(zx, 1)) * 8));
    R = dops.as<double>();
    Y = R + col;
    Q = Y + col;
    Rx = R + col * (want_disp ? 3 : 1);
    if (!sparse) {
      PH_TRY(dX.alloc(col * 8));
      auto on_panel = [&](int64_t c0, int64_t c1) -> int {   // the ranks of a column panel follow its DMA, as replaid.sing's
        return launch_colranks_dense_f64(ctx, dX.as<double>() + c0 * ld, ld, g, (int32_t)(c1 - c0), PLAIDHIP_TIES_MIN, 0, 1.0,
                                         R + c0 * ld, ld, nullptr);
      };
      PH_TRY(upload_pipelined(ctx, dX.as<char>(), (size_t)ld * 8, reinterpret_cast<const char*>(c.X + (int64_t)lo * g),
                              (size_t)g * 8, nloc, on_panel));
      PH_TRY(launch_colnan(ctx, dX.as<double>(), ld, nullptr, g, nloc, 0, d_colnan));
    } else {
      int32_t max_nnz = 0;
      PH_TRY(upload_csc_shard(s, ploc, dXp, dXi, dX, &max_nnz));
      PH_TRY(launch_colnan(ctx, dX.as<double>(), 0, dXp.as<int32_t>(), g, nloc, max_nnz, d_colnan));
      // replaid.sing ranks the zeros too (shard_worker): the dense rank matrix from the ranks of the stored values, or, for
      // a column with more stored values than one pass ranks, densify and rank
      if (max_nnz <= max_sparse_rank_column())
        PH_TRY(launch_colranks_csc_dense_nz_f64(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), dX.as<double>(), g, nloc, max_nnz,
                                                PLAIDHIP_TIES_MIN, 0, 1.0, Rx, R, ld, nullptr));
      else
        PH_TRY(launch_colranks_csc_dense_f64(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), dX.as<double>(), g, nloc,
                                             PLAIDHIP_TIES_MIN, 0, 1.0, R, ld, nullptr));
    }
    if (want_disp) {
      PH_TRY(launch_last_ranks(ctx, dense_cols(g, nloc, ld), R, Y, Q));
      PH_TRY(launch_sing_rpos(ctx, R, Q, ld, d_colnan, g, nloc, reinterpret_cast<uint32_t*>(Y), ld));
    }
    for (int o = 0; o < 6; ++o)
      if (c.sx_out[o]) home[o].prepare(c.sx_out[o] + (int64_t)lo * m, (size_t)m * nloc * 8);
    return PLAIDHIP_OK;
  });

  // ---- scores: crossprods on the exact rank route, the pinned epilogue; dispersions: the per-pair kernel -----------------
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (nloc == 0) return PLAIDHIP_OK;
    if (want_score) {
      // r holds integers in [1, N]: the rank route's u16 staging when 2 N fits, integer sums either way
      const int xk = 2 * (int64_t)g < 65536 ? PLAIDHIP_X_RANKS : PLAIDHIP_X_ANY;
      PH_TRY(launch_spmm_dense_f64(ctx, gs_up, R, ld, nloc, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0, part(1), m, nullptr, xk));
      if (down)
        PH_TRY(launch_spmm_dense_f64(ctx, gs_dn, R, ld, nloc, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0, part(2), m, nullptr, xk));
      PH_TRY(launch_sing_score(ctx, part(1), down ? part(2) : nullptr, down ? part(0) : nullptr, m, m, nloc, dk.as<int32_t>(),
                               dk.as<int32_t>() + m, g, c.center, d_colnan));
    }
    if (want_disp) {
      const uint32_t* Rpos = reinterpret_cast<const uint32_t*>(Y);
      PH_TRY(launch_sing_mad(ctx, Q, ld, Rpos, ld, d_colnan, g, nloc, dGp.as<int32_t>(), dGi.as<int32_t>(), m, part(4), m));
      if (down) {
        // (the MAD of d = N + 1 - r is the MAD of r: a reflection)
        PH_TRY(launch_sing_mad(ctx, Q, ld, Rpos, ld, d_colnan, g, nloc, dDp.as<int32_t>(), dDi.as<int32_t>(), m, part(5), m));
        PH_TRY(launch_sing_add(ctx, part(4), part(5), part(3), m, m, nloc));
      }
    }
    return PLAIDHIP_OK;
  });

  // ---- the requested shards go home ---------------------------------------------------------------------------------------
  s.step([&]() -> int {
    if (nloc > 0)
      for (int o = 0; o < 6; ++o)
        if (c.sx_out[o]) PH_TRY(home[o].copy(ctx, part(o)));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    return PLAIDHIP_OK;
  });
  return s.finish();
}

// one device's part of replaid.ucell.exact / replaid.aucell.exact (kUcellExact, kAucellExact; kernels_trunc.hip): the
// truncated-rank stage turns the shard's columns into compressed columns of rank weights, panel by panel (a panel's slots
// stay below 2^27 entries and are sized by what its own columns can take), the sparse crossprod multiplies each panel with the prepared sets, and the pinned epilogue
// closes.  A dgCMatrix is never expanded: O(nnz + columns x T) on the device.  Nothing couples the shards, nothing is read
// back before the results.
int truncated_exact_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc;
  const int32_t g = c.g, m = c.m;
  const bool sparse = c.Xp != nullptr;
  const bool ucell = c.method == kUcellExact;
  const int mode = ucell ? PLAIDHIP_TRUNC_UCELL : PLAIDHIP_TRUNC_AUCELL;
  const int64_t T = (int64_t)c.max_rank;
  double* const outs[3] = {ucell ? c.sx_out[0] : nullptr, ucell ? c.sx_out[1] : c.S_out, ucell ? c.sx_out[2] : nullptr};
  const bool up = outs[0] || outs[1], down = outs[0] || outs[2];
  s.force_f64();
  plaidhip_geneset *gs_up = nullptr, *gs_dn = nullptr;
  CtxBuf dX{ctx, 0}, dXp{ctx, 1}, dXi{ctx, 2}, dops{ctx, 3}, dS{ctx, 4}, dsmall{ctx, 5};
  DevBuf dk, dK, dWi, dWx;
  HomeBuffer home[3];
  const size_t nl = (size_t)std::max(nloc, 1);
  const size_t nscores = (size_t)m * nl;
  auto part = [&](int o) { return dS.as<double>() + (size_t)o * nscores; };   // [total | up | down]
  std::vector<int32_t> kset((size_t)m * 2, 0), ploc;
  std::vector<double> kfull;
  for (int32_t j = 0; j < m; ++j) {   // members after the alignment
    kset[(size_t)j] = c.Gp[j + 1] - c.Gp[j];
    if (c.Dp != nullptr) kset[(size_t)m + j] = c.Dp[j + 1] - c.Dp[j];
  }
  if (c.k_full != nullptr) {
    kfull.assign((size_t)m * 2, 0.0);
    for (int32_t j = 0; j < m; ++j) {
      kfull[(size_t)j] = c.k_full[j];
      if (c.k_full_down != nullptr) kfull[(size_t)m + j] = c.k_full_down[j];
    }
  }
  double* d_u0 = nullptr;
  uint32_t* d_colnan = nullptr;
  int32_t *d_cnt = nullptr, *d_Wp = nullptr;
  int32_t max_nnz = 0;
  std::vector<int64_t> pcol{0}, pent;   // the panels' first columns, and the most entries each can take (its slots)
  int64_t wcap = 1, pmax = 1;            // the largest panel's entries and columns

  // ---- upload -----------------------------------------------------------------------------------------------------------------
  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    if (up) PH_TRY(acquire_geneset(ctx, g, m, c.Gp, c.Gi, &gs_up));
    if (down) PH_TRY(acquire_geneset(ctx, g, m, c.Dp, c.Di, &gs_dn));
    // [u0 | NaN flags | counts | slot pointers]
    PH_TRY(dsmall.alloc(nl * 8 + nl * 4 + nl * 4 + (nl + 1) * 4));
    d_u0 = dsmall.as<double>();
    d_colnan = reinterpret_cast<uint32_t*>(d_u0 + nl);
    d_cnt = reinterpret_cast<int32_t*>(d_colnan + nl);
    d_Wp = d_cnt + nl;
    PH_TRY(dS.alloc(nscores * 3 * 8));
    if (nloc == 0) return PLAIDHIP_OK;
    PH_TRY(dk.alloc((size_t)m * 2 * 4));
    PH_HIP(hipMemcpyAsync(dk.p, kset.data(), (size_t)m * 2 * 4, hipMemcpyHostToDevice, ctx->stream));
    if (!kfull.empty()) {
      PH_TRY(dK.alloc((size_t)m * 2 * 8));
      PH_HIP(hipMemcpyAsync(dK.p, kfull.data(), (size_t)m * 2 * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    if (!sparse) {
      PH_TRY(dX.alloc((size_t)g * nloc * 8));
      PH_TRY(upload_pipelined(ctx, dX.as<char>(), (size_t)g * 8, reinterpret_cast<const char*>(c.X + (int64_t)lo * g),
                              (size_t)g * 8, nloc, nullptr));
    } else {
      PH_TRY(upload_csc_shard(s, ploc, dXp, dXi, dX, &max_nnz));
    }
    // panels of columns whose slots stay below 2^27 entries, sized by what their own columns can take: a dgCMatrix in
    // UCell mode by its stored values (the sum over a panel is its nnz), everything else by the rank bound
    {
      int64_t sum = 0;
      for (int32_t j = 0; j < nloc; ++j) {
        const int64_t b = truncated_bound(mode, T, g, sparse ? ploc[(size_t)j + 1] - ploc[(size_t)j] : 0, sparse);
        if (sum + b > ((int64_t)1 << 27) && j > pcol.back()) {
          pent.push_back(sum);
          pcol.push_back(j);
          sum = 0;
        }
        sum += b;
      }
      pent.push_back(sum);
      pcol.push_back(nloc);
      for (size_t q = 0; q < pent.size(); ++q) {
        wcap = std::max(wcap, pent[q]);
        pmax = std::max(pmax, pcol[q + 1] - pcol[q]);
      }
    }
    // the ranks: a panel of dense columns, or of the stored values of the whole shard (and, for "last", the tie-free copy)
    PH_TRY(dops.alloc((sparse ? (size_t)std::max<int64_t>(s.zx, 1) * 2 : (size_t)g * (size_t)pmax) * 8));
    PH_TRY(dWi.alloc((size_t)wcap * 4));
    PH_TRY(dWx.alloc((size_t)wcap * 8));
    for (int o = 0; o < 3; ++o)
      if (outs[o]) home[o].prepare(outs[o] + (int64_t)lo * m, (size_t)m * nloc * 8);
    return PLAIDHIP_OK;
  });

  // ---- per panel: the truncated ranks as compressed columns, their crossprods; then the pinned epilogue ----------------------
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (nloc == 0) return PLAIDHIP_OK;
    for (size_t q = 0; q + 1 < pcol.size(); ++q) {
      const int64_t c0 = pcol[q];
      const int32_t nc = (int32_t)(pcol[q + 1] - c0);
      if (!sparse)
        PH_TRY(truncated_ranks_stage(ctx, mode, T, dX.as<double>() + c0 * g, g, nullptr, nullptr, g, nc, 0, 0, dops.as<double>(),
                                     d_colnan + c0, d_cnt, d_Wp, dWi.as<int32_t>(), dWx.as<double>(), wcap, nullptr));
      else   // (absolute offsets into the shard's @i / @x, and into the rank scratch)
        PH_TRY(truncated_ranks_stage(ctx, mode, T, dX.as<double>(), 0, dXp.as<int32_t>() + c0, dXi.as<int32_t>(), g, nc, max_nnz,
                                     s.zx, dops.as<double>(), d_colnan + c0, d_cnt, d_Wp, dWi.as<int32_t>(), dWx.as<double>(),
                                     wcap, d_u0 + c0));
      // The weights are half-integers (UCell; the shifted ones of any sign) or integers: every sum is exact on the fixed-point
      // and on the fp64 accumulators alike (a negative weight sends the scatter kernel to fp64, decided on the device), and on
      // the gather kernel; an estimate of the entries picks between scatter and gather
      const int64_t est = std::min<int64_t>(pent[q], (int64_t)nc * T);
      if (up)
        PH_TRY(launch_spmm_csc_f64(ctx, gs_up, d_Wp, dWi.as<int32_t>(), dWx.as<double>(), nc, est, PLAIDHIP_STAT_SUM, 1.0, nullptr,
                                   0.0, part(1) + c0 * m, m, nullptr));
      if (down)
        PH_TRY(launch_spmm_csc_f64(ctx, gs_dn, d_Wp, dWi.as<int32_t>(), dWx.as<double>(), nc, est, PLAIDHIP_STAT_SUM, 1.0, nullptr,
                                   0.0, part(2) + c0 * m, m, nullptr));
    }
    if (!ucell) return launch_aucell_exact(ctx, part(1), m, m, nloc, dk.as<int32_t>(), T, d_colnan);
    const double* K = kfull.empty() ? nullptr : dK.as<double>();
    return launch_ucell_exact(ctx, up ? part(1) : nullptr, down ? part(2) : nullptr, outs[0] ? part(0) : nullptr, m, m, nloc,
                              dk.as<int32_t>(), dk.as<int32_t>() + m, K, (K && c.k_full_down) ? K + m : nullptr,
                              sparse ? d_u0 : nullptr, T, c.w_neg, d_colnan);
  });

  // ---- the requested shards go home ---------------------------------------------------------------------------------------
  s.step([&]() -> int {
    if (nloc > 0)
      for (int o = 0; o < 3; ++o)
        if (outs[o]) PH_TRY(home[o].copy(ctx, part(o)));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    return PLAIDHIP_OK;
  });
  return s.finish();
}

}  // namespace plaidhip
