// plaid.voom on the sharded engine (shard.cpp; include/plaidhip.h: plaidhip_voom).
#include "shard.h"
#include "lowess.h"

namespace plaidhip {

// Steps 4 - 6 of the header on the host: the trend points of the rows that are not all zero and have a finite s2, sorted by
// sx (ties in row order), lowess with delta = 0.01 (max - min), and the anchors of its last pass at unique x as the knots.
int voom_trend_knots(int32_t rows, const double* M, const double* s2, const double* rowsum, const double* lib, int32_t n,
                     double span, std::vector<double>& kx, std::vector<double>& ky) {
  double ml = 0.0;   // mean_c(log2(L_c + 1)): ascending c from 0.0, one division
  for (int32_t c = 0; c < n; ++c) ml = ml + log2(lib[c] + 1.0);
  ml = ml / (double)n;
  const double shift = ml - log2(1e6);
  std::vector<double> sx, sy;
  for (int32_t r = 0; r < rows; ++r) {
    if (rowsum[r] == 0.0 || !std::isfinite(s2[r])) continue;
    sx.push_back(M[r] + shift);
    sy.push_back(sqrt(sqrt(s2[r])));
  }
  const size_t m = sx.size();
  PH_REQUIRE(m >= 1, "voom: no row with a count and a finite variance to fit the trend on");
  for (size_t i = 0; i < m; ++i) PH_REQUIRE(std::isfinite(sx[i]), "voom: a row's mean log-CPM is not finite");
  std::vector<size_t> order(m);
  for (size_t i = 0; i < m; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return sx[a] < sx[b]; });
  std::vector<double> x(m), y(m), ys(m);
  std::vector<int8_t> anchor(m);
  for (size_t i = 0; i < m; ++i) {
    x[i] = sx[order[i]];
    y[i] = sy[order[i]];
  }
  lowess_run(x.data(), y.data(), (int64_t)m, span, 3, 0.01 * (x[m - 1] - x[0]), ys.data(), anchor.data());
  kx.clear();
  ky.clear();
  for (size_t i = 0; i < m; ++i)
    if (anchor[i] && (kx.empty() || x[i] != kx.back())) {
      kx.push_back(x[i]);
      ky.push_back(ys[i]);
    }
  PH_REQUIRE(kx.size() <= PLAIDHIP_VOOM_MAX_KNOTS, "voom: %lld knots (at most %d)", (long long)kx.size(), PLAIDHIP_VOOM_MAX_KNOTS);
  return PLAIDHIP_OK;
}

bool voom_empty(const Call& c) { return c.g == 0 || c.n == 0; }

void voom_prepare(Shared& sh, const Call& c, int) {
  sh.voom.colsum.assign((size_t)c.n, 0.0);
  sh.voom.rowsum.assign((size_t)c.g, 0.0);
  sh.limma.effects.assign((size_t)(c.ncoef + 1) * c.g, 0.0);
  sh.limma.rss.assign((size_t)c.g, 0.0);
}

// One device's part of plaid.voom (kernels_voom.hip, kernels_lmfit.hip).  The SAMPLES are shared out at multiples of 128
// columns.  Every pass is column-local but three: the check (a flag, or-ed), the row sums and the unweighted fit, whose block
// partials are chained from shard to shard in the order of the one-device call (chain_flat_sums), so every sharding has its
// bits.  Shard 0 fits the trend on the host between the fit and the weights pass.  Nothing is written to the caller's
// memory before the last step: a refused count or a failing shard leaves the outputs alone.
int voom_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc, rows = c.g, n = c.n, p = c.ncoef;
  const size_t R = (size_t)rows;
  const int64_t W1 = p + 1, ld = even_ld(rows);
  CtxBuf dA{ctx, 0}, dE{ctx, 3}, dW{ctx, 4};
  DevBuf dQ, dinvn, dmask, dwt, dws, drows, dcol, dbad, dlib, doff, dkx, dky;
  double *d_seed = nullptr, *d_run = nullptr, *d_eff = nullptr;
  std::vector<double> qloc, libloc, offloc;

  // ---- upload; the check with the column sums; the row sums' block partials -----------------------------------------------------
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    PH_HIP(hipSetDevice(ctx->device));
    if (nloc == 0) return PLAIDHIP_OK;
    PH_TRY(drows.alloc((size_t)W1 * R * 3 * 8));   // [seed | running sums | the effects of all samples], [p + 1][rows] each
    d_seed = drows.as<double>();
    d_run = d_seed + W1 * rows;
    d_eff = d_run + W1 * rows;
    PH_TRY(dws.alloc((size_t)row_design_ws_doubles(rows, nloc, W1) * 8));
    PH_TRY(dcol.alloc((size_t)nloc * 8));
    PH_TRY(dbad.alloc(4));
    PH_HIP(hipMemsetAsync(dbad.p, 0, 4, ctx->stream));
    PH_TRY(dA.alloc((size_t)ld * nloc * 8));
    PH_TRY(upload_pipelined(ctx, dA.as<char>(), (size_t)ld * 8, reinterpret_cast<const char*>(c.X + (int64_t)lo * rows), R * 8,
                            nloc, nullptr));
    PH_TRY(launch_voom_check(ctx, dA.as<double>(), ld, rows, nloc, dcol.as<double>(), dbad.as<uint32_t>()));
    PH_TRY(launch_voom_rowsum(ctx, dA.as<double>(), ld, rows, nloc, dws.as<double>()));
    uint32_t bad = 0;
    PH_HIP(hipMemcpyAsync(sh.voom.colsum.data() + lo, dcol.p, (size_t)nloc * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(&bad, dbad.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    std::lock_guard<std::mutex> lk(sh.mu);
    sh.voom.bad |= bad;
    return PLAIDHIP_OK;
  });
  chain_flat_sums(s, sh.voom.rowsum, dws.as<double>(), rows, d_seed, d_run);
  if (k == 0)
    s.step([&]() -> int {
      PH_REQUIRE(sh.voom.bad == 0, "voom: a count is NaN, negative or infinite (counts are finite and >= 0)");
      sh.voom.lib.resize((size_t)n);
      sh.voom.off.resize((size_t)n);
      const double l6 = log2(1e6);
      for (int32_t col = 0; col < n; ++col) {
        const double L = c.voom_lib != nullptr ? c.voom_lib[col] : sh.voom.colsum[(size_t)col];
        sh.voom.lib[(size_t)col] = L;
        sh.voom.off[(size_t)col] = log2(L + 1.0) - l6;
      }
      return PLAIDHIP_OK;
    });
  sh.rv.arrive_and_wait();

  // ---- log-CPM of the shard's columns; the unweighted fit's effects, then its RSS at the effects of ALL samples -----------------
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    libloc.assign(sh.voom.lib.begin() + lo, sh.voom.lib.begin() + lo + nloc);
    offloc.assign(sh.voom.off.begin() + lo, sh.voom.off.begin() + lo + nloc);
    PH_TRY(dlib.alloc((size_t)nloc * 8));
    PH_TRY(doff.alloc((size_t)nloc * 8));
    PH_HIP(hipMemcpyAsync(dlib.p, libloc.data(), (size_t)nloc * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemcpyAsync(doff.p, offloc.data(), (size_t)nloc * 8, hipMemcpyHostToDevice, ctx->stream));
    qloc.resize((size_t)nloc * p);
    for (int64_t col = 0; col < p; ++col)
      std::copy(c.lm_Q.begin() + col * n + lo, c.lm_Q.begin() + col * n + lo + nloc, qloc.begin() + col * nloc);
    PH_TRY(dQ.alloc(qloc.size() * 8));
    PH_HIP(hipMemcpyAsync(dQ.p, qloc.data(), qloc.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dinvn.alloc(8));
    PH_HIP(hipMemcpyAsync(dinvn.p, c.lm_invn.data(), 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dmask.alloc((size_t)lmfit_mask_bytes(nloc, W1)));
    PH_TRY(dwt.alloc((size_t)lmfit_weight_bytes(nloc, W1)));
    PH_TRY(launch_lmfit_masks(ctx, dQ.as<double>(), nullptr, dinvn.as<double>(), nloc, p, 1, dmask.p, dwt.as<double>()));
    PH_TRY(dE.alloc((size_t)ld * nloc * 8));
    PH_TRY(launch_voom_logcpm(ctx, dA.as<double>(), ld, rows, nloc, dlib.as<double>(), dE.as<double>(), ld));
    return launch_row_design_effects(ctx, dE.as<double>(), ld, rows, nloc, dmask.p, dwt.as<double>(), (int32_t)W1,
                                     dws.as<double>());
  });
  chain_flat_sums(s, sh.limma.effects, dws.as<double>(), W1 * rows, d_seed, d_run);
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    PH_HIP(hipMemcpyAsync(d_eff, sh.limma.effects.data(), (size_t)W1 * R * 8, hipMemcpyHostToDevice, ctx->stream));
    return launch_row_design_rss(ctx, dE.as<double>(), ld, rows, nloc, dQ.as<double>(), dmask.p, p, 1, d_eff, dws.as<double>());
  });
  chain_flat_sums(s, sh.limma.rss, dws.as<double>(), rows, d_seed, d_run);

  // ---- shard 0: the trend on the host -------------------------------------------------------------------------------------------
  if (k == 0)
    s.step([&]() -> int {
      std::vector<double> s2(R);
      const double d = (double)(n - p);
      for (size_t r = 0; r < R; ++r) s2[r] = sh.limma.rss[r] / d;
      return voom_trend_knots(rows, sh.limma.effects.data() + (size_t)p * R, s2.data(), sh.voom.rowsum.data(), sh.voom.lib.data(), n,
                              c.voom_span, sh.voom.kx, sh.voom.ky);
    });
  sh.rv.arrive_and_wait();

  // ---- the weights of the shard's columns; E and W go home ----------------------------------------------------------------------
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    const int32_t nk = (int32_t)sh.voom.kx.size();
    PH_TRY(dkx.alloc((size_t)nk * 8));
    PH_TRY(dky.alloc((size_t)nk * 8));
    PH_HIP(hipMemcpyAsync(dkx.p, sh.voom.kx.data(), (size_t)nk * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemcpyAsync(dky.p, sh.voom.ky.data(), (size_t)nk * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dW.alloc((size_t)ld * nloc * 8));
    PH_TRY(launch_voom_weights(ctx, dQ.as<double>(), doff.as<double>(), nloc, p, d_eff, rows, dkx.as<double>(), dky.as<double>(),
                               nk, dW.as<double>(), ld));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    return PLAIDHIP_OK;
  });
  sh.rv.arrive_and_wait();   // (every shard's passes are done: from here on the caller's memory is written)
  s.step([&]() -> int {
    if (nloc > 0) {
      PH_HIP(hipMemcpy2DAsync(c.voom_E + (size_t)lo * R, R * 8, dE.p, (size_t)ld * 8, R * 8, (size_t)nloc, hipMemcpyDeviceToHost,
                              ctx->stream));
      PH_HIP(hipMemcpy2DAsync(c.voom_W + (size_t)lo * R, R * 8, dW.p, (size_t)ld * 8, R * 8, (size_t)nloc, hipMemcpyDeviceToHost,
                              ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (k != 0) return PLAIDHIP_OK;
    const size_t nk = sh.voom.kx.size();
    std::copy(sh.voom.lib.begin(), sh.voom.lib.end(), c.voom_lib_out);
    std::copy(sh.voom.off.begin(), sh.voom.off.end(), c.voom_off);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t i = 0; i < PLAIDHIP_VOOM_MAX_KNOTS; ++i) {
      c.voom_kx[i] = i < nk ? sh.voom.kx[i] : nan;
      c.voom_ky[i] = i < nk ? sh.voom.ky[i] : nan;
    }
    *c.voom_nk = (int32_t)nk;
    return PLAIDHIP_OK;
  });
  return s.finish();
}

}  // namespace plaidhip
