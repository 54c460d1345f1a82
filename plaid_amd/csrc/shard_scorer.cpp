// replaid.ucell / aucell / scse / gsva and replaid.gsva.exact on the sharded engine (shard.cpp).
#include "shard.h"

namespace plaidhip {

// one device's part of replaid.ucell / aucell / scse / gsva (kUcell ... kGsva; one shard: plaidhip_ucell ... plaidhip_gsva_csc)
// and of replaid.gsva.exact (kGsvaExact).  The quantities that couple the samples are combined on the host between the
// phases: max(rX) (R/plaid.R:278, 306), the min / max behind removeLog2 = NULL (:160-161), the per-gene mean and sd of the
// z row transform (:341-343) and the medians' flags and mean(medx) (:554-575).
int scorer_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc;
  const int32_t g = c.g, m = c.m, n = c.n;
  const bool sparse = c.Xp != nullptr;
  const int method = c.method;
  const bool ranked = method == kUcell || method == kAucell;
  // replaid.gsva.exact (kGsvaExact): replaid.gsva's row transform (z, ecdf, or none: X as it is), then the last ranks of the
  // columns of v and the walk of kernels_ks.hip in place of the signed ranks, the crossprod and the medians
  const bool gx = method == kGsvaExact;
  const bool ztf = (method == kGsva || gx) && c.rowtf == 0;
  // "ecdf" ranks all samples of a gene together: one shard only (the argument checks see to it)
  const bool ecdf = (method == kGsva || gx) && c.rowtf == 1;
  // "gauss": GSVA's kernel CDF estimate (kernels_kcdf.hip).  Every V_ij needs its gene's whole row, so all of X goes to
  // every device, which computes the columns of its own shard: dX holds V, dense, whatever X was
  const bool gauss = gx && c.rowtf == 3;
  // leading dimension of the staged X and of the ranks: g, or even where the transposes and the pair crossprod of
  // replaid.gsva want their columns 16-byte aligned
  const int64_t ld = (ztf || ecdf) ? even_ld(g) : (int64_t)g;
  if (gx) s.force_f64();
  plaidhip_geneset* gs = nullptr;
  CtxBuf dX{ctx, 0}, dXp{ctx, 1}, dXi{ctx, 2}, dR{ctx, 3}, dS{ctx, 4}, dsmall{ctx, 5};
  DevBuf dscratch, dcsc, drp, drows, dy, dadd;
  DevBuf dops, dGp, dGi, dperm, dcolnan;   // gsva.exact: [Q | rank scratch | T], the pattern, the NaN flags
  size_t ops_t = 0;                        // where T starts in dops
  HomeBuffer home;
  uint32_t* d_flags = nullptr;
  double *d_gmax = nullptr, *d_mm = nullptr, *d_med = nullptr, *d_colmax = nullptr, *d_colsum = nullptr;
  double *d_mean = nullptr, *d_ssd = nullptr, *d_seed = nullptr, *d_run = nullptr;
  const int64_t zx = s.zx;
  int32_t max_row = 0, max_nnz = 0;
  std::vector<int32_t> ploc;
  // host sources of asynchronous uploads: they live until the worker's last synchronisation
  std::vector<double> host_mean, host_ssd, row_nnz, add;

  // ---- upload; the per-shard work up to the first coupling ------------------------------------------------------------
  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    PH_TRY(acquire_geneset(ctx, g, m, c.Gp, c.Gi, &gs));
    const size_t nl = (size_t)std::max(nloc, 1);
    PH_TRY(dsmall.alloc(64 + nl * 24));
    d_flags = dsmall.as<uint32_t>();
    d_gmax = reinterpret_cast<double*>(dsmall.as<char>() + 16);
    d_mm = d_gmax + 1;   // {min, max}
    d_med = reinterpret_cast<double*>(dsmall.as<char>() + 64);
    d_colmax = d_med + nl;
    d_colsum = d_colmax + nl;
    PH_HIP(hipMemsetAsync(dsmall.p, 0, 64, ctx->stream));
    PH_TRY(dS.alloc((size_t)m * nl * 8));
    if (ztf || ecdf) {   // [mean | group 1 (unused) | ssd | seed | running sums], g each
      PH_TRY(drows.alloc((size_t)g * 5 * 8));
      d_mean = drows.as<double>();
      d_ssd = d_mean + 2 * (size_t)g;
      d_seed = d_ssd + g;
      d_run = d_seed + g;
      PH_HIP(hipMemsetAsync(drows.p, 0, (size_t)g * 5 * 8, ctx->stream));
    }
    if (nloc == 0) return PLAIDHIP_OK;
    if (gx) {
      // Q, then the rank scratch (dense columns: 2 g nloc doubles; a dgCMatrix's stored values: 3 nnz), then T
      const int64_t nz = gauss ? 0 : zx;   // ("gauss" leaves a dense V)
      ops_t = (size_t)g * nloc + std::max((size_t)g * nloc * 2, (size_t)nz * 3);
      PH_TRY(dops.alloc((ops_t + (size_t)g) * 8));
      PH_TRY(dcolnan.alloc((size_t)nloc * 4));
      PH_TRY(upload_pattern(ctx, c.Gp, c.Gi, m, dGp, dGi));
    }
    if (gauss) {
      PH_TRY(dX.alloc((size_t)ld * nloc * 8));
      PH_TRY(gsva_kcdf_columns(ctx, c.Xp, c.Xi, c.X, g, n, lo, nloc, dX.as<double>()));
    } else if (!sparse) {
      PH_TRY(dX.alloc((size_t)ld * nloc * 8));
      if (method != kScse && !gx) PH_TRY(dR.alloc((size_t)ld * nloc * 8));
      // ucell / aucell: the average ranks of a column panel follow its DMA
      auto on_panel = [&](int64_t c0, int64_t c1) -> int {
        return launch_colranks_dense_f64(ctx, dX.as<double>() + c0 * ld, ld, g, (int32_t)(c1 - c0), PLAIDHIP_TIES_AVERAGE, 0,
                                         1.0, dR.as<double>() + c0 * ld, ld, d_colmax + c0);
      };
      PH_TRY(upload_pipelined(ctx, dX.as<char>(), (size_t)ld * 8, reinterpret_cast<const char*>(c.X + (int64_t)lo * g),
                              (size_t)g * 8, nloc, ranked ? std::function<int(int64_t, int64_t)>(on_panel) : nullptr));
      if (ecdf) {
        // zX = t(apply(X, 1, function(x) ecdf(x)(x))) (R/plaid.R:346): ecdf(x)(x_i) = #{x <= x_i} / n = rank(x, "max") / n
        // per gene.  Genes become columns (transpose), the column rank kernel ranks them, and the result goes back; the
        // factor 1 / n is dropped because only the per-sample ORDER of zX is used afterwards (:352)
        double* tmp = gx ? dops.as<double>() : dR.as<double>();
        PH_TRY(launch_transpose_f64(ctx, dX.as<double>(), ld, g, nloc, tmp, nloc));
        PH_TRY(launch_colranks_dense_f64(ctx, tmp, nloc, nloc, g, PLAIDHIP_TIES_MAX, 0, 1.0, dX.as<double>(), nloc, nullptr));
        PH_TRY(launch_transpose_f64(ctx, dX.as<double>(), nloc, nloc, g, tmp, ld));
        PH_HIP(hipMemcpyAsync(dX.p, tmp, (size_t)ld * nloc * 8, hipMemcpyDeviceToDevice, ctx->stream));
      }
      if (ztf) {   // zX, step 1: the block partials of the row sums (every sample in group 0)
        PH_TRY(dy.alloc((size_t)nloc * 4));
        PH_HIP(hipMemsetAsync(dy.p, 0, (size_t)nloc * 4, ctx->stream));
        PH_TRY(dscratch.alloc((size_t)row_group_ws_doubles(g, nloc) * 8));
        PH_TRY(launch_row_group_partials(ctx, dX.as<double>(), ld, g, nloc, dy.as<int32_t>(), nullptr, dscratch.as<double>()));
      }
    } else {
      // (a row transform builds a dense zX in dX: the slots' values go beside it)
      if (ztf || ecdf) PH_TRY(upload_csc_shard(s, ploc, dXp, dXi, dcsc, &max_nnz));
      else PH_TRY(upload_csc_shard(s, ploc, dXp, dXi, dX, &max_nnz));
      double* vals = (ztf || ecdf) ? dcsc.as<double>() : dX.as<double>();
      if (ranked) {
        // dense average ranks, zeros tie: from the ranks of the stored values (any nrow(X)) unless a column stores more
        // than one pass ranks -- then it is densified and ranked
        PH_TRY(dR.alloc((size_t)ld * nloc * 8));
        if (max_nnz <= max_sparse_rank_column()) {
          PH_TRY(dscratch.alloc((size_t)std::max<int64_t>(zx, 1) * 8));
          PH_TRY(launch_colranks_csc_dense_nz_f64(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), vals, g, nloc, max_nnz,
                                                  PLAIDHIP_TIES_AVERAGE, 0, 1.0, dscratch.as<double>(), dR.as<double>(), ld,
                                                  d_colmax));
        } else {
          PH_TRY(launch_colranks_csc_dense_f64(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), vals, g, nloc, PLAIDHIP_TIES_AVERAGE,
                                               0, 1.0, dR.as<double>(), ld, d_colmax));
        }
      } else if (ecdf) {
        // "ecdf" without the factor 1 / n, as for dense X: #{x <= x_i} per gene from the max ranks of its stored values and
        // its implicit zeros; the stored entries' values go back to CSC order (into the CSC value slot, no longer needed)
        // and are expanded with the rows' zero values
        PH_TRY(dX.alloc((size_t)ld * nloc * 8));
        if (!gx) PH_TRY(dR.alloc((size_t)ld * nloc * 8));   // (zx <= g nloc: checked with the arguments)
        PH_TRY(drp.alloc((size_t)(g + 2) * 4));
        PH_TRY(dscratch.alloc((size_t)std::max<int64_t>(zx, 1) * 8));
        PH_TRY(dperm.alloc((size_t)std::max<int64_t>(zx, 1) * 4));
        PH_TRY(launch_csc_to_csr(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), vals, g, nloc, drp.as<int32_t>(), nullptr,
                                 dscratch.as<double>(), dperm.as<int32_t>(), drp.as<int32_t>() + g + 1));
        PH_HIP(hipMemcpyAsync(&max_row, drp.as<int32_t>() + g + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));
        PH_TRY(launch_csr_row_ecdf(ctx, drp.as<int32_t>(), dscratch.as<double>(), g, nloc, max_row, dperm.as<int32_t>(),
                                   gx ? dops.as<double>() : dR.as<double>(), vals, drows.as<double>()));
        PH_TRY(launch_csc_expand(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), vals, g, nloc, ld, drows.as<double>(), nullptr,
                                 nullptr, dX.as<double>()));
      } else if (ztf) {
        // the shard's row view, and pass A of its row moments: the sums of the stored values
        PH_TRY(dX.alloc((size_t)ld * nloc * 8));
        if (!gx) PH_TRY(dR.alloc((size_t)ld * nloc * 8));
        PH_TRY(drp.alloc((size_t)(g + 2) * 4));
        PH_TRY(dscratch.alloc((size_t)std::max<int64_t>(zx, 1) * 8));
        PH_TRY(launch_csc_to_csr(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), vals, g, nloc, drp.as<int32_t>(), nullptr,
                                 dscratch.as<double>(), nullptr, drp.as<int32_t>() + g + 1));
        std::vector<int32_t> rp((size_t)g + 2);
        PH_HIP(hipMemcpyAsync(rp.data(), drp.p, (size_t)(g + 2) * 4, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));
        max_row = rp[(size_t)g + 1];
        // One shard: both passes in one kernel, the launch plaidhip_gsva_csc has always made.  Its division and its
        // q + z mu^2 run on the device, where the compiler may contract them differently from the host's below: the
        // one-device bits stay what they were.
        if (ndev == 1) {   // (group 1's unused sums land on d_seed, which is written later)
          PH_TRY(launch_csr_row_group_moments(ctx, drp.as<int32_t>(), nullptr, dscratch.as<double>(), g, max_row, nullptr, n, 0,
                                              d_mean, d_ssd));
        } else {
          PH_TRY(launch_csr_row_stored_moment(ctx, drp.as<int32_t>(), dscratch.as<double>(), g, max_row, nullptr, d_run));
          std::vector<double> sums((size_t)g);
          std::vector<int32_t> len((size_t)g);
          for (int32_t i = 0; i < g; ++i) len[(size_t)i] = rp[(size_t)i + 1] - rp[(size_t)i];
          PH_HIP(hipMemcpyAsync(sums.data(), d_run, (size_t)g * 8, hipMemcpyDeviceToHost, ctx->stream));
          PH_HIP(hipStreamSynchronize(ctx->stream));
          sh.gsva.row_sum[(size_t)k] = std::move(sums);   // (each shard writes its own slot)
          sh.gsva.row_len[(size_t)k] = std::move(len);
        }
      }
    }
    // (the result's pages are made from here on, as in shard_worker)
    home.prepare(c.S_out + (int64_t)lo * m, (size_t)m * nloc * 8);
    return PLAIDHIP_OK;
  });

  // ---- max over every shard of a device vector (launch_max, whose comparisons are repeated here) -------------------------
  double gmax = -INFINITY;   // (the host copy of d_gmax: lives until the stream has been synchronised)
  auto global_max = [&](const double* d_vec) {
    double mine = -INFINITY;
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      PH_TRY(launch_max(ctx, d_vec, nloc, d_gmax));
      PH_HIP(hipMemcpyAsync(&mine, d_gmax, 8, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      return PLAIDHIP_OK;
    });
    {
      std::lock_guard<std::mutex> lk(sh.mu);
      if (nloc > 0 && s.rc == PLAIDHIP_OK) {
        sh.gmax = (sh.gmax_set && !(mine > sh.gmax)) ? sh.gmax : mine;
        sh.gmax_set = true;
      }
    }
    sh.rv.arrive_and_wait();
    gmax = sh.gmax_set ? sh.gmax : -INFINITY;
    s.step([&]() -> int {   // every shard divides by / subtracts from the same device scalar
      if (nloc == 0) return PLAIDHIP_OK;
      PH_HIP(hipMemcpyAsync(d_gmax, &gmax, 8, hipMemcpyHostToDevice, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      return PLAIDHIP_OK;
    });
  };

  // ---- replaid.gsva, z row transform: rowMeans and rowSds of ALL samples -----------------------------------------------
  if (ztf && !sparse) {
    chain_block_sums(s, sh.gsva.chain_sum, dscratch.as<double>(), g, 1, d_seed, d_run);
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      host_mean.resize((size_t)g);
      // A true division, as rowMeans and the dgCMatrix branch below divide: sum * fl(1 / n) misses the mean of a constant
      // gene for some n (1.25 at n = 105), whose z then is -2e-8 instead of 0 and whose signed rank -1 instead of 0
      for (int32_t i = 0; i < g; ++i) host_mean[(size_t)i] = sh.gsva.chain_sum[(size_t)i] / (double)n;
      PH_HIP(hipMemcpyAsync(d_mean, host_mean.data(), (size_t)g * 8, hipMemcpyHostToDevice, ctx->stream));
      return launch_row_group_partials(ctx, dX.as<double>(), ld, g, nloc, dy.as<int32_t>(), d_mean, dscratch.as<double>());
    });
    chain_block_sums(s, sh.gsva.chain_ssd, dscratch.as<double>(), g, 1, d_seed, d_run);
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      PH_HIP(hipMemcpyAsync(d_ssd, sh.gsva.chain_ssd.data(), (size_t)g * 8, hipMemcpyHostToDevice, ctx->stream));
      PH_TRY(launch_row_ztransform_shard(ctx, dX.as<double>(), ld, g, nloc, n, d_mean, d_ssd));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      return PLAIDHIP_OK;
    });
  } else if (ztf) {
    // dgCMatrix: the shards' sums of stored values added in shard order, mean = s / n; then the same for the squared
    // deviations, plus (n - nnz) mean^2 for the implicit zeros, once (csr_row_moments_kernel's expression)
    host_mean.assign((size_t)g, 0.0);
    host_ssd.assign((size_t)g, 0.0);
    row_nnz.assign((size_t)g, 0.0);
    sh.rv.arrive_and_wait();
    if (s.live()) {
      for (int32_t i = 0; i < g; ++i) {
        double sum = 0.0, z = 0.0;
        for (int q = 0; q < ndev; ++q)
          if (!sh.gsva.row_sum[(size_t)q].empty()) { sum += sh.gsva.row_sum[(size_t)q][(size_t)i]; z += sh.gsva.row_len[(size_t)q][(size_t)i]; }
        host_mean[(size_t)i] = sum / (double)n;
        row_nnz[(size_t)i] = z;
      }
    }
    s.step([&]() -> int {
      if (nloc == 0 || ndev == 1) return PLAIDHIP_OK;
      PH_HIP(hipMemcpyAsync(d_mean, host_mean.data(), (size_t)g * 8, hipMemcpyHostToDevice, ctx->stream));
      PH_TRY(launch_csr_row_stored_moment(ctx, drp.as<int32_t>(), dscratch.as<double>(), g, max_row, d_mean, d_run));
      std::vector<double> q((size_t)g);
      PH_HIP(hipMemcpyAsync(q.data(), d_run, (size_t)g * 8, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      sh.gsva.row_ssd[(size_t)k] = std::move(q);
      return PLAIDHIP_OK;
    });
    sh.rv.arrive_and_wait();
    if (s.live()) {
      for (int32_t i = 0; i < g; ++i) {
        double q = 0.0;
        for (int r = 0; r < ndev; ++r)
          if (!sh.gsva.row_ssd[(size_t)r].empty()) q += sh.gsva.row_ssd[(size_t)r][(size_t)i];
        const double mu = host_mean[(size_t)i], z = (double)n - row_nnz[(size_t)i];
        host_ssd[(size_t)i] = z > 0.0 ? q + z * (mu * mu) : q;
      }
    }
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      if (ndev > 1) PH_HIP(hipMemcpyAsync(d_ssd, host_ssd.data(), (size_t)g * 8, hipMemcpyHostToDevice, ctx->stream));
      double* dflt = d_seed;
      PH_TRY(launch_row_z_defaults(ctx, d_mean, d_ssd, g, n, dflt));   // (n: the sd's divisor alone)
      PH_TRY(launch_csc_expand_shard(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), dcsc.as<double>(), g, nloc, n, ld, dflt, d_mean,
                                     d_ssd, dX.as<double>()));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      return PLAIDHIP_OK;
    });
  }
  if (method == kGsva) {
    // rX = colranks(zX, signed = TRUE, "average"); rX / max|rX|; sign * |rX|^(1 + tau) (R/plaid.R:352-358)
    //    = sign * rank^(1 + tau) / max(rank^(1 + tau)): the power is fused into the rank kernel, the division into the
    //    crossprod's epilogue (d_gmax below), by linearity of the mean statistic
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      return launch_colranks_dense_f64(ctx, dX.as<double>(), ld, g, nloc, PLAIDHIP_TIES_AVERAGE, 1,
                                       c.tau > 0.0 ? 1.0 + c.tau : 1.0, dR.as<double>(), ld, d_colmax);
    });
  }

  // ---- replaid.gsva.exact: q = rank(v, "last") of every column, then the walk ------------------------------------------------
  if (gx)
    s.step([&]() -> int {
      if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
      if (nloc == 0) return PLAIDHIP_OK;
      double* Q = dops.as<double>();
      double* scratch = Q + (size_t)g * nloc;
      double* T = Q + ops_t;
      uint32_t* d_colnan = dcolnan.as<uint32_t>();
      // (alpha = 0: the operand pass writes Q and the NaN flags only, no W or P)
      if (sparse && c.rowtf == 2)   // ("gauss" left its dense V in dX) the stored values are ranked, as replaid.ssgsea.exact ranks a dgCMatrix
        PH_TRY(launch_ssgsea_exact_operands(ctx, dX.as<double>(), 0, dXp.as<int32_t>(), dXi.as<int32_t>(), g, nloc,
                                            max_nnz, zx, 0.0, Q, nullptr, nullptr, g, scratch, d_colnan));
      else
        PH_TRY(launch_ssgsea_exact_operands(ctx, dX.as<double>(), ld, nullptr, nullptr, g, nloc, 0, 0, 0.0, Q, nullptr, nullptr, g,
                                            scratch, d_colnan));
      return launch_gsva_ks(ctx, Q, g, d_colnan, g, nloc, dGp.as<int32_t>(), dGi.as<int32_t>(), m, c.tau, c.max_diff, T,
                            dS.as<double>(), m);
    });

  // ---- max(rX) (ucell / aucell: R/plaid.R:278, 306; gsva: max|rX|, :354) --------------------------------------------------
  if (method != kScse && !gx) global_max(d_colmax);
  if (ranked)
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      return method == kUcell ? launch_map(ctx, dR.as<double>(), (int64_t)g * nloc, 0, c.rmax + 1.0, d_gmax)      // :278
                         : launch_map(ctx, dR.as<double>(), (int64_t)g * nloc, 1, c.auc_max_rank, d_gmax);   // :306
    });

  // ---- replaid.scse: removeLog2 = NULL decided once, from min / max of the whole matrix (R/plaid.R:160-161) -------------
  bool remove_log2 = c.remove_log2 > 0;
  if (method == kScse && c.remove_log2 < 0) {
    double mm[2] = {INFINITY, -INFINITY};
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      PH_TRY(launch_minmax(ctx, dX.as<double>(), sparse ? zx : (int64_t)g * nloc, d_mm));
      PH_HIP(hipMemcpyAsync(mm, d_mm, 16, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      return PLAIDHIP_OK;
    });
    merge_range(s, mm[0], mm[1]);
    sh.rv.arrive_and_wait();
    double mn = sh.xmin, mx = sh.xmax;
    if (sparse && (int64_t)c.Xp[n] < (int64_t)g * n) { mn = mn < 0.0 ? mn : 0.0; mx = mx > 0.0 ? mx : 0.0; }   // implicit zeros
    remove_log2 = mn == 0.0 && mx < 20.0;
  }
  if (method == kScse) {
    if (k == 0) sh.removed_log2 = remove_log2;
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      if (remove_log2) PH_TRY(launch_map(ctx, dX.as<double>(), sparse ? zx : (int64_t)g * nloc, sparse ? 3 : 2, 0.0, nullptr));
      return launch_col_abs_sums(ctx, dX.as<double>(), ld, g, sparse ? dXp.as<int32_t>() : nullptr, nloc, d_colsum);
    });
  }

  // ---- crossprod --------------------------------------------------------------------------------------------------------
  if (!gx) s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (nloc == 0) return PLAIDHIP_OK;
    if (method == kScse) {
      const int stat = c.score_mean ? PLAIDHIP_STAT_MEAN : PLAIDHIP_STAT_SUM;
      if (sparse) {
        // the kernel is chosen from the density of the whole matrix, as in shard_worker (one shard: the count itself, which
        // x / n * n may miss by one in its last place)
        const int64_t nnz_choice = ndev == 1 ? (int64_t)c.Xp[n] : (int64_t)((double)c.Xp[n] / (double)n * (double)nloc);
        return launch_spmm_csc_f64(ctx, gs, dXp.as<int32_t>(), dXi.as<int32_t>(), dX.as<double>(), nloc, nnz_choice, stat, 1.0,
                                   nullptr, 0.0, dS.as<double>(), m, nullptr);
      }
      return launch_spmm_dense_f64(ctx, gs, dX.as<double>(), ld, nloc, stat, 1.0, nullptr, 0.0, dS.as<double>(), m, nullptr);
    }
    int x_kind = PLAIDHIP_X_ANY;
    if (method == kUcell) {   // pmin(max(rX) - rX, rmax + 1) of average ranks: half-integers when rmax + 1 is one
      const double cap2 = 2.0 * (c.rmax + 1.0);
      x_kind = (cap2 == std::floor(cap2) && cap2 < 65536.0) ? PLAIDHIP_X_RANKS : PLAIDHIP_X_ANY;
    }
    if (method == kGsva) x_kind = c.tau > 0.0 ? PLAIDHIP_X_ANY : PLAIDHIP_X_EXACT_F32;   // signed average ranks
    return launch_spmm_dense_f64(ctx, gs, dR.as<double>(), ld, nloc, PLAIDHIP_STAT_MEAN, 1.0, method == kGsva ? d_gmax : nullptr,
                                 0.0, dS.as<double>(), m, d_flags, x_kind);
  });

  // ---- normalize_medians (R/plaid.R:554-575) -------------------------------------------------------------------------------
  if (method != kScse && !gx) {
    const double mean_med = medians_and_their_mean(s, dS.as<double>(), d_flags, d_med);
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      return launch_shift_columns(ctx, dS.as<double>(), m, m, nloc, d_med, mean_med, nullptr);
    });
  }

  // ---- the affine steps of replaid.ucell and replaid.scse ------------------------------------------------------------------
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    if (method == kUcell) {   // 1 - S / rmax + (k + 1) / (2 rmax)   (R/plaid.R:280)
      add.resize((size_t)m);
      for (int32_t j = 0; j < m; ++j) add[(size_t)j] = 1.0 + (c.k_full[j] + 1.0) / (2.0 * c.rmax);
      PH_TRY(dadd.alloc((size_t)m * 8));
      PH_HIP(hipMemcpyAsync(dadd.p, add.data(), (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
      return launch_affine(ctx, dS.as<double>(), m, m, nloc, -1.0 / c.rmax, nullptr, 1.0, dadd.as<double>(), 0.0);
    }
    if (method == kScse)   // mean: sX / (colMeans|X| + 1e-8) (:176-177); sum: sX / (colSums|X| + 1e-8) * 100 (:181-182)
      return launch_affine(ctx, dS.as<double>(), m, m, nloc, c.score_mean ? 1.0 : 100.0, d_colsum,
                           c.score_mean ? 1.0 / (double)g : 1.0, nullptr, 0.0);
    return PLAIDHIP_OK;
  });

  // ---- the score shard goes home ----------------------------------------------------------------------------------------
  s.step([&]() -> int {
    if (nloc > 0) PH_TRY(home.copy(ctx, dS.p));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    return PLAIDHIP_OK;
  });
  return s.finish();
}

void gsva_prepare(Shared& sh, const Call& c, int ndev) {
  sh.gsva.chain_sum.assign((size_t)c.g, 0.0);
  sh.gsva.chain_ssd.assign((size_t)c.g, 0.0);
  sh.gsva.row_sum.resize((size_t)ndev);
  sh.gsva.row_ssd.resize((size_t)ndev);
  sh.gsva.row_len.resize((size_t)ndev);
}

int scse_tail(plaidhip_ctx*, const Call& c, Shared& sh) {
  if (c.removed_log2 != nullptr) *c.removed_log2 = sh.removed_log2 ? 1 : 0;
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
