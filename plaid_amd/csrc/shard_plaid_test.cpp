// plaid.test and plaid.test.contrasts on the sharded engine (shard.cpp): one worker, one host tail.
#include "shard.h"

namespace plaidhip {

namespace {

// plaid.test is its own one contrast, with the group sizes of y
int32_t contrasts(const Call& c) { return c.method == kPlaidTestContrasts ? c.ncontrast : 1; }
int64_t group_size(const Call& c, int32_t j, int group) {
  if (c.method != kPlaidTestContrasts) return group ? c.n1 : c.n0;
  return group ? c.cn1[(size_t)j] : c.cn0[(size_t)j];
}

// the group means of [C][2][rows] chained sums, each contrast with its own group sizes: reduce_blocks_kernel's scale (a
// product with 1 / n_k, NaN for an empty group)
void scaled_group_means(const Call& c, const std::vector<double>& sums, int32_t rows, double* mean) {
  for (int32_t j = 0; j < contrasts(c); ++j) {
    const int64_t n0 = group_size(c, j, 0), n1 = group_size(c, j, 1);
    const double s0 = n0 > 0 ? 1.0 / (double)n0 : std::numeric_limits<double>::quiet_NaN();
    const double s1 = n1 > 0 ? 1.0 / (double)n1 : std::numeric_limits<double>::quiet_NaN();
    const size_t o = (size_t)j * 2 * rows;
    for (int32_t i = 0; i < rows; ++i) {
      mean[o + i] = sums[o + i] * s0;
      mean[o + rows + i] = sums[o + rows + i] * s1;
    }
  }
}

}  // namespace

// one device's part of a sharded plaid.test (kPlaidTest, R/plaid.R:392-474; one shard: plaidhip_plaid_test / _csc) or
// plaid.test.contrasts (kPlaidTestContrasts; include/plaidhip.h), with what couples the samples combined on the host in
// between -- everything plaid.test reduces is a row sum over the samples, so only O(genes + sets) numbers cross between the
// shards and the scores never leave their device.
//   logFC: dense X chains the two group sums of X from shard to shard (the one-device block order); a dgCMatrix sums each
//     shard's stored values per group, the host adds the shards.  Shard 0 alone then takes F = [fc, fc^2] and T = Gt F.
//   scores ("lm"): gsetX's columns uploaded, or plaid(X, G)'s sharded crossprod and medians (shard_worker), stopped
//     before the shift: the shard keeps the raw S, its medians and mean(medx).
//   Welch moments: the group sums of the score rows, shifted on load, chained; then, from the global means, the sums of
//     squared deviations, chained.  plaidhip_plaid_test_finish runs in plaid_test_tail.
// C label columns (cx): the same phases and rendezvous; what was [2][rows] is [C][2][rows], the labels get their masks, the
// row moments come from kernels_contrasts.hip (every read of X and of S shared by a tile of contrasts) and are chained all
// at once, plaid(X, G) and the medians run once, and shard 0 takes Gt [fc_j, fc_j^2] per contrast with plaid.test's crossprod
// call.  A contrast adds what plaid.test adds for its label column, in its order; plaid.test keeps kernels_stats.hip's kernels.
int plaid_test_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc;
  const int32_t g = c.g, m = c.m, n = c.n, C = contrasts(c);
  const bool cx = c.method == kPlaidTestContrasts;
  const bool sparse = c.Xp != nullptr;
  const bool lm = (c.tests & 4) != 0;
  const bool scores = lm && c.gsetX == nullptr;   // plaid(X, G) computed here (R/plaid.R:424-427), once
  const int64_t ldg = even_ld(g);
  const int64_t wide = std::max<int64_t>(g, m);
  const size_t nl = (size_t)std::max(nloc, 1);
  plaidhip_geneset* gs = nullptr;
  CtxBuf dX{ctx, 0}, dXp{ctx, 1}, dXi{ctx, 2}, dS{ctx, 4}, dsmall{ctx, 5};
  DevBuf dy, dmask, dws, drows, drp, dRj, dRx, dF, dT;
  uint32_t* d_flags = nullptr;
  double *d_med = nullptr, *d_seed = nullptr, *d_run = nullptr, *d_mean = nullptr;
  const int64_t zx = s.zx;
  std::vector<int32_t> ploc;
  // host sources of asynchronous uploads: they live until the worker's last synchronisation
  std::vector<double> x_mean, s_mean;

  // ---- what differs between the two methods: the kernels of the row moments and how their block partials are chained -------
  auto ws_doubles = [&](int32_t rows) { return cx ? row_contrast_ws_doubles(rows, nloc, C) : row_group_ws_doubles(rows, nloc); };
  auto s_partials = [&](const double* med, double add, const double* mean) -> int {   // the score rows, shifted on load
    if (cx) return launch_row_contrast_partials(ctx, dS.as<double>(), m, m, nloc, dmask.p, C, med, add, mean, dws.as<double>());
    return launch_row_group_shifted_partials(ctx, dS.as<double>(), m, m, nloc, dy.as<int32_t>(), med, add, mean, dws.as<double>());
  };
  auto chain = [&](std::vector<double>& run, int32_t rows) {   // ndev rendezvous
    if (cx) chain_flat_sums(s, run, dws.as<double>(), (int64_t)C * 2 * rows, d_seed, d_run);
    else chain_block_sums(s, run, dws.as<double>(), rows, 2, d_seed, d_run);
  };

  // ---- upload; the labels (and their masks); X's group sums of this shard; plaid()'s crossprod of dense X panel by panel -----
  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    if (k == 0 || scores) PH_TRY(acquire_geneset(ctx, g, m, c.Gp, c.Gi, &gs));
    PH_TRY(dsmall.alloc(64 + nl * 8));
    d_flags = dsmall.as<uint32_t>();
    d_med = reinterpret_cast<double*>(dsmall.as<char>() + 64);
    PH_HIP(hipMemsetAsync(dsmall.p, 0, 64, ctx->stream));
    PH_TRY(drows.alloc((size_t)wide * 6 * C * 8));   // [seed | running sums | means], [C][2][max(g, m)] each
    d_seed = drows.as<double>();
    d_run = d_seed + 2 * wide * C;
    d_mean = d_run + 2 * wide * C;
    if (lm) PH_TRY(dS.alloc((size_t)m * nl * 8));
    if (nloc == 0) return PLAIDHIP_OK;
    PH_TRY(dy.alloc((size_t)nloc * C * 4));   // the shard's rows of Y, nloc x C
    for (int32_t j = 0; j < C; ++j)
      PH_HIP(hipMemcpyAsync(dy.as<int32_t>() + (size_t)j * nloc, c.y + (size_t)j * n + lo, (size_t)nloc * 4,
                            hipMemcpyHostToDevice, ctx->stream));
    if (cx) {
      PH_TRY(dmask.alloc((size_t)contrast_mask_bytes(nloc, C)));
      PH_TRY(launch_contrast_masks(ctx, dy.as<int32_t>(), nloc, nloc, C, dmask.p));
    }
    PH_TRY(dws.alloc((size_t)std::max<int64_t>({sparse ? 0 : ws_doubles(g), lm ? ws_doubles(m) : 0, cx ? 1 : 0}) * 8));
    if (!sparse) {
      PH_TRY(dX.alloc((size_t)ldg * nloc * 8));
      auto on_panel = [&](int64_t c0, int64_t c1) -> int {   // (shard_worker's plaid())
        return launch_spmm_dense_f64(ctx, gs, dX.as<double>() + c0 * ldg, ldg, (int32_t)(c1 - c0), PLAIDHIP_STAT_MEAN, 1.0,
                                     nullptr, 0.0, dS.as<double>() + c0 * m, m, d_flags);
      };
      PH_TRY(upload_pipelined(ctx, dX.as<char>(), (size_t)ldg * 8, reinterpret_cast<const char*>(c.X + (int64_t)lo * g),
                              (size_t)g * 8, nloc, scores ? std::function<int(int64_t, int64_t)>(on_panel) : nullptr));
      if (!cx) return launch_row_group_partials(ctx, dX.as<double>(), ldg, g, nloc, dy.as<int32_t>(), nullptr, dws.as<double>());
      return launch_row_contrast_partials(ctx, dX.as<double>(), ldg, g, nloc, dmask.p, C, nullptr, 0.0, nullptr,
                                          dws.as<double>());
    }
    int32_t max_nnz = 0;
    PH_TRY(upload_csc_shard(s, ploc, dXp, dXi, dX, &max_nnz));
    const size_t zb = (size_t)std::max<int64_t>(zx, 1);
    // the shard's row view, built once, with its column indices (they look up y), and the unscaled group sums of its stored
    // values, per contrast
    PH_TRY(drp.alloc((size_t)(g + 2) * 4));
    PH_TRY(dRj.alloc(zb * 4));
    PH_TRY(dRx.alloc(zb * 8));
    PH_TRY(launch_csc_to_csr(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), dX.as<double>(), g, nloc, drp.as<int32_t>(),
                             dRj.as<int32_t>(), dRx.as<double>(), nullptr, drp.as<int32_t>() + g + 1));
    int32_t max_row = 0;
    PH_HIP(hipMemcpyAsync(&max_row, drp.as<int32_t>() + g + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    for (int32_t j = 0; j < C; ++j)
      PH_TRY(launch_csr_row_group_stored_sums(ctx, drp.as<int32_t>(), dRj.as<int32_t>(), dRx.as<double>(), g, max_row,
                                              dy.as<int32_t>() + (size_t)j * nloc, d_run + (size_t)j * 2 * g));
    std::vector<double> sums((size_t)g * 2 * C);
    PH_HIP(hipMemcpyAsync(sums.data(), d_run, sums.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    sh.pt.row_sum[(size_t)k] = std::move(sums);   // (each shard writes its own slot)
    return PLAIDHIP_OK;
  });

  // ---- logFC_j (R/plaid.R:407-409 on the contrast's samples); shard 0: Gt fc_j, Gt fc_j^2 (:478-479) ------------------------
  if (!sparse) chain(sh.pt.chain_x, g);
  else sh.rv.arrive_and_wait();   // every shard's stored-value sums are in sh.pt.row_sum
  s.step([&]() -> int {
    if (k != 0) return PLAIDHIP_OK;
    x_mean.resize((size_t)g * 2 * C);
    if (!sparse) {
      scaled_group_means(c, sh.pt.chain_x, g, x_mean.data());
    } else {   // the shards added in shard order, then csr_row_moments_kernel's true division (0 / 0 = NaN, empty group)
      for (int32_t j = 0; j < C; ++j) {
        const size_t o = (size_t)j * 2 * g;
        for (int32_t i = 0; i < g; ++i) {
          double s0 = 0.0, s1 = 0.0;
          for (int q = 0; q < ndev; ++q)
            if (!sh.pt.row_sum[(size_t)q].empty()) { s0 += sh.pt.row_sum[(size_t)q][o + i]; s1 += sh.pt.row_sum[(size_t)q][o + g + i]; }
          x_mean[o + i] = s0 / (double)group_size(c, j, 0);
          x_mean[o + g + i] = s1 / (double)group_size(c, j, 1);
        }
      }
    }
    PH_TRY(dF.alloc((size_t)ldg * 2 * C * 8));
    PH_TRY(dT.alloc((size_t)m * 2 * C * 8));
    PH_HIP(hipMemcpyAsync(d_mean, x_mean.data(), x_mean.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemsetAsync(dF.p, 0, (size_t)ldg * 2 * C * 8, ctx->stream));
    if (cx) PH_TRY(launch_fold_change_contrasts(ctx, d_mean, g, C, ldg, dF.as<double>()));
    else PH_TRY(launch_fold_change(ctx, d_mean, g, ldg, dF.as<double>()));
    for (int32_t j = 0; j < C; ++j)   // two columns per call, whatever C: the same crossprod call, so the same bits
      PH_TRY(launch_spmm_dense_f64(ctx, gs, dF.as<double>() + (size_t)j * 2 * ldg, ldg, 2, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0,
                                   dT.as<double>() + (size_t)j * 2 * m, m, nullptr));
    PH_HIP(hipMemcpyAsync(sh.pt.T.data(), dT.p, (size_t)m * 2 * C * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(sh.pt.F.data(), dF.p, (size_t)ldg * 2 * C * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    return PLAIDHIP_OK;
  });

  // ---- the scores, once: gsetX's columns, or plaid(X, G)'s crossprod of a dgCMatrix (dense X: done panel by panel above) ----
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (nloc == 0 || !lm) return PLAIDHIP_OK;
    if (!scores)
      return upload_pipelined(ctx, dS.as<char>(), (size_t)m * 8, reinterpret_cast<const char*>(c.gsetX + (int64_t)lo * m),
                              (size_t)m * 8, nloc, nullptr);
    if (!sparse) return PLAIDHIP_OK;
    // (after shard 0's Gt F above: another crossprod between this one and the medians would discard what it classified)
    const int64_t nnz_choice = (int64_t)((double)c.Xp[n] / (double)n * (double)nloc);   // (as shard_worker)
    return launch_spmm_csc_fused_f64(ctx, gs, dXp.as<int32_t>(), dXi.as<int32_t>(), dX.as<double>(), nloc, zx,
                                     PLAIDHIP_STAT_MEAN, 1.0, nullptr, 0.0, dS.as<double>(), m, d_flags, /*bounded=*/false,
                                     nullptr, 0.0, nnz_choice);
  });

  // ---- normalize_medians (R/plaid.R:554-575) over ALL samples, up to mean(medx): the shift is applied on load below ---------
  const double add = scores ? medians_and_their_mean(s, dS.as<double>(), d_flags, d_med) : 0.0;

  // ---- Welch moments of the score rows, every contrast per read of S (Rfast::ttests(t(gsetX), ina = y + 1), :429) -----------
  if (lm) {
    const double* med = scores ? d_med : nullptr;
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      return s_partials(med, add, nullptr);
    });
    chain(sh.pt.chain_s, m);
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      s_mean.resize((size_t)m * 2 * C);
      scaled_group_means(c, sh.pt.chain_s, m, s_mean.data());
      PH_HIP(hipMemcpyAsync(d_mean, s_mean.data(), s_mean.size() * 8, hipMemcpyHostToDevice, ctx->stream));
      return s_partials(med, add, d_mean);
    });
    chain(sh.pt.chain_q, m);
  }

  return s.finish();
}

bool plaid_test_empty(const Call& c) { return c.m == 0 || contrasts(c) == 0; }

void plaid_test_prepare(Shared& sh, const Call& c, int ndev) {
  const size_t C = (size_t)contrasts(c);
  sh.pt.chain_x.assign((size_t)c.g * 2 * C, 0.0);
  sh.pt.chain_s.assign((size_t)c.m * 2 * C, 0.0);
  sh.pt.chain_q.assign((size_t)c.m * 2 * C, 0.0);
  sh.pt.T.assign((size_t)c.m * 2 * C, 0.0);
  sh.pt.F.assign((size_t)even_ld(c.g) * 2 * C, 0.0);
  sh.pt.row_sum.resize((size_t)ndev);
}

// the host half of plaid.test (R/plaid.R:410-474), once per contrast with its group sizes
int plaid_test_tail(plaidhip_ctx*, const Call& c, Shared& sh) {
  const bool lm = (c.tests & 4) != 0;
  const int64_t ldg = even_ld(c.g);
  const size_t m = (size_t)c.m;
  std::vector<double> SM, means;   // SM: [group means | sums of squared deviations] of one contrast, [2][m] each
  if (lm) {
    SM.resize(m * 4);
    means.resize(m * 2 * (size_t)contrasts(c));
    scaled_group_means(c, sh.pt.chain_s, c.m, means.data());
  }
  for (int32_t j = 0; j < contrasts(c); ++j) {
    const double* F = sh.pt.F.data() + (size_t)j * 2 * ldg;
    double tot1 = 0.0, tot2 = 0.0;
    for (int32_t i = 0; i < c.g; ++i) { tot1 += F[(size_t)i]; tot2 += F[(size_t)ldg + i]; }
    if (lm) {
      std::copy(means.begin() + (size_t)j * 2 * m, means.begin() + (size_t)(j + 1) * 2 * m, SM.begin());
      std::copy(sh.pt.chain_q.begin() + (size_t)j * 2 * m, sh.pt.chain_q.begin() + (size_t)(j + 1) * 2 * m, SM.begin() + 2 * m);
    }
    PH_TRY(plaidhip_plaid_test_finish(c.g, c.m, c.Gp, sh.pt.T.data() + (size_t)j * 2 * m, tot1, tot2, lm ? SM.data() : nullptr,
                                      group_size(c, j, 0), group_size(c, j, 1), c.tests, c.metap_method,
                                      c.out + (size_t)j * 6 * m));
  }
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
