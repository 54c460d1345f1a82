// plaid.limma with weights on the sharded engine (shard.cpp; include/plaidhip.h: plaidhip_limma_w).
#include "shard.h"

namespace plaidhip {

// One device's part of the weighted fit (kernels_lmfit_w.hip).  The SAMPLES are shared out at multiples of 128 columns, as for
// plaid.limma: a shard takes its columns of A and of Wt, its entries of aw, and its rows of every Q_f and of use.  Round one
// chains the weighted sums [nfit Wc][rows] (H's triangle, b and M' of every pair) and the counts [2 nfit + 1][rows] from shard
// to shard; then shard 0 solves every (row, fit) and leaves gamma and AveExpr where plaid.limma leaves its effects, with every
// row's df.residual and u_j; round two chains the weighted residual sums of squares of the shards' own columns at gamma.  The
// block partials are added in the order of the one-device call, so every sharding has its bits.  3 ndev + 1 rendezvous.
int limma_w_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc, rows = c.g, n = c.n, p = c.ncoef, nfit = c.nfit, q = c.nq;
  const size_t R = (size_t)rows;
  const int64_t Wc = lmfit_w_columns(p), W = (int64_t)nfit * Wc, C = 2 * (int64_t)nfit + 1, W1 = (int64_t)nfit * (p + 1);
  const int64_t ld = even_ld(rows);
  CtxBuf dA{ctx, 0}, dWt{ctx, 3};
  DevBuf dQ, duse, dinvn, daw, dmask, dwt, dws, dcw, drows, dG;
  double *d_seed = nullptr, *d_run = nullptr;
  // host sources of asynchronous uploads: they live until the worker's last synchronisation
  std::vector<double> qloc;
  std::vector<int8_t> uloc;

  // ---- upload; the shard's rows of Q and use, the table of products; the block partials of the sums and of the counts ---------
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    PH_HIP(hipSetDevice(ctx->device));
    if (nloc == 0) return PLAIDHIP_OK;
    PH_TRY(drows.alloc((size_t)W * R * 2 * 8));   // [seed | running sums], [W][rows] each (W >= 2 nfit + 1 and W >= nfit)
    d_seed = drows.as<double>();
    d_run = d_seed + W * rows;
    PH_TRY(dG.alloc((size_t)W1 * R * 8));
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
    if (c.aw != nullptr) {
      PH_TRY(daw.alloc((size_t)nloc * 8));
      PH_HIP(hipMemcpyAsync(daw.p, c.aw + lo, (size_t)nloc * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    PH_TRY(dmask.alloc((size_t)lmfit_mask_bytes(nloc, W)));
    PH_TRY(dwt.alloc((size_t)lmfit_weight_bytes(nloc, W)));
    PH_TRY(launch_lmfit_w_table(ctx, dQ.as<double>(), c.use != nullptr ? duse.as<int8_t>() : nullptr, dinvn.as<double>(), nloc, p,
                                nfit, dmask.p, dwt.as<double>()));
    PH_TRY(dws.alloc((size_t)row_design_ws_doubles(rows, nloc, W) * 8));   // (W >= nfit: the RSS partials fit too)
    PH_TRY(dcw.alloc((size_t)row_design_ws_doubles(rows, nloc, C) * 8));
    PH_TRY(dA.alloc((size_t)ld * nloc * 8));
    PH_TRY(upload_pipelined(ctx, dA.as<char>(), (size_t)ld * 8, reinterpret_cast<const char*>(c.X + (int64_t)lo * rows), R * 8,
                            nloc, nullptr));
    if (c.Wt != nullptr) {
      PH_TRY(dWt.alloc((size_t)ld * nloc * 8));
      PH_TRY(upload_pipelined(ctx, dWt.as<char>(), (size_t)ld * 8, reinterpret_cast<const char*>(c.Wt + (int64_t)lo * rows),
                              R * 8, nloc, nullptr));
    }
    const double* wt = c.Wt != nullptr ? dWt.as<double>() : nullptr;
    const double* aw = c.aw != nullptr ? daw.as<double>() : nullptr;
    PH_TRY(launch_row_design_w_sums(ctx, dA.as<double>(), wt, aw, ld, rows, nloc, dmask.p, dwt.as<double>(), p, nfit,
                                    dws.as<double>()));
    return launch_lmfit_w_counts(ctx, dA.as<double>(), wt, aw, ld, rows, nloc, c.use != nullptr ? duse.as<int8_t>() : nullptr,
                                 nfit, dcw.as<double>());
  });
  chain_flat_sums(s, sh.limma.wsum, dws.as<double>(), W * rows, d_seed, d_run);
  chain_flat_sums(s, sh.limma.wcnt, dcw.as<double>(), C * rows, d_seed, d_run);

  // ---- shard 0: the solve of every (row, fit) from the sums of ALL samples ----------------------------------------------------
  if (k == 0)
    s.step([&]() -> int {
      std::vector<double> nfd((size_t)nfit);
      for (int32_t f = 0; f < nfit; ++f) nfd[(size_t)f] = (double)c.lm_nf[(size_t)f];
      sh.limma.na_d.assign(R * nfit, 0.0);
      sh.limma.na_u.assign(R * nfit * q, 0.0);
      // (the chained sums are whole on the host, and on a device only with one shard: they go up into the chain's two buffers,
      // which are free now, and gamma comes out where the RSS pass reads it)
      DevBuf dv, dnf, dd, du;
      if (nloc == 0) {
        PH_TRY(drows.alloc((size_t)W * R * 2 * 8));
        d_seed = drows.as<double>();
        d_run = d_seed + W * rows;
        PH_TRY(dG.alloc((size_t)W1 * R * 8));
      }
      auto up = [&](DevBuf& b, const void* src, size_t bytes) -> int {
        PH_TRY(b.alloc(bytes));
        PH_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return PLAIDHIP_OK;
      };
      PH_HIP(hipMemcpyAsync(d_seed, sh.limma.wsum.data(), sh.limma.wsum.size() * 8, hipMemcpyHostToDevice, ctx->stream));
      PH_HIP(hipMemcpyAsync(d_run, sh.limma.wcnt.data(), sh.limma.wcnt.size() * 8, hipMemcpyHostToDevice, ctx->stream));
      PH_TRY(up(dv, c.lm_v.data(), c.lm_v.size() * 8));
      PH_TRY(up(dnf, nfd.data(), nfd.size() * 8));
      PH_TRY(dd.alloc(R * nfit * 8));
      PH_TRY(du.alloc(R * nfit * q * 8));
      PH_TRY(launch_lmfit_w_solve(ctx, d_seed, d_run, dv.as<double>(), dnf.as<double>(), rows, n, p, nfit, q, c.max_na,
                                  dG.as<double>(), dd.as<double>(), du.as<double>()));
      PH_HIP(hipMemcpyAsync(sh.limma.effects.data(), dG.p, (size_t)W1 * R * 8, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipMemcpyAsync(sh.limma.na_d.data(), dd.p, R * nfit * 8, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipMemcpyAsync(sh.limma.na_u.data(), du.p, R * nfit * q * 8, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      return PLAIDHIP_OK;
    });
  sh.rv.arrive_and_wait();

  // ---- the weighted residual sums of squares of the shard's columns at gamma ----------------------------------------------------
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    if (k != 0) PH_HIP(hipMemcpyAsync(dG.p, sh.limma.effects.data(), (size_t)W1 * R * 8, hipMemcpyHostToDevice, ctx->stream));
    return launch_row_design_w_rss(ctx, dA.as<double>(), c.Wt != nullptr ? dWt.as<double>() : nullptr,
                                   c.aw != nullptr ? daw.as<double>() : nullptr, ld, rows, nloc, dQ.as<double>(), dmask.p, p, nfit,
                                   dG.as<double>(), dws.as<double>());
  });
  chain_flat_sums(s, sh.limma.rss, dws.as<double>(), (int64_t)nfit * rows, d_seed, d_run);
  return s.finish();
}

}  // namespace plaidhip
