// plaid.fisher, plaid.rankcor and replaid.plage / replaid.zscore on the sharded engine (shard.cpp): the families that share
// out lists or columns and never meet.
#include "shard.h"

namespace plaidhip {

constexpr int kFisherBhThreads = 8;            // host threads of one shard's Benjamini-Hochberg columns, at most
constexpr int64_t kFisherBhWork = 1 << 16;     // p-values per thread below which another thread is not worth its start
// one device's part of plaid.fisher (kFisher, kernels_fisher.hip).  The lists are shared out (plaidhip_shard_bounds over c):
// a shard takes the columns of sig of its lists and all of G, and a list's results depend on that list alone, so every
// sharding has the one-shard bits.  Benjamini-Hochberg of the shard's own lists runs on the host, on the shard's thread and,
// for many lists, on a few more (every column is the same routine whichever thread runs it).  No rendezvous.
int fisher_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t g = c.g, m = c.m, l0 = s.lo, nl = s.nloc;
  const size_t nnz = (size_t)c.Gp[m];
  DevBuf dsig, dmask, dtot, dov, dGp, dGi, dout, dlen, didx;
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (nl <= 0) return PLAIDHIP_OK;
    PH_HIP(hipSetDevice(ctx->device));
    const int32_t ntile = (nl + PLAIDHIP_FISHER_LIST_TILE - 1) / PLAIDHIP_FISHER_LIST_TILE;
    PH_TRY(dsig.alloc((size_t)g * nl));
    PH_TRY(dmask.alloc((size_t)g * ntile * 2));
    PH_TRY(dtot.alloc((size_t)nl * 2 * 4));
    PH_TRY(dov.alloc((size_t)nl * 2 * m * 4));
    PH_TRY(dout.alloc((size_t)m * 12 * nl * 8));
    PH_TRY(upload_pattern(ctx, c.Gp, c.Gi, m, dGp, dGi));
    PH_TRY(upload_pipelined(ctx, dsig.as<char>(), (size_t)g, reinterpret_cast<const char*>(c.sig + (size_t)l0 * g), (size_t)g, nl,
                            nullptr));
    PH_TRY(launch_fisher_pack(ctx, dsig.as<int8_t>(), g, nl, dmask.as<uint16_t>(), dtot.as<int32_t>()));
    PH_TRY(launch_fisher_count(ctx, dmask.as<uint16_t>(), g, nl, dGp.as<int32_t>(), dGi.as<int32_t>(), m, dov.as<int32_t>()));
    PH_TRY(launch_fisher_tail(ctx, dtot.as<int32_t>(), dov.as<int32_t>(), dGp.as<int32_t>(), g, nl, m, dout.as<double>()));
    double* out = c.out + (size_t)l0 * 12 * m;
    std::vector<int32_t> tot((size_t)nl * 2);
    PH_HIP(hipMemcpyAsync(out, dout.p, (size_t)m * 12 * nl * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(tot.data(), dtot.p, (size_t)nl * 2 * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (c.le_len != nullptr) {
      PH_TRY(dlen.alloc((size_t)m * nl * 4));
      PH_TRY(didx.alloc(std::max<size_t>(nnz * nl, 1) * 4));
      PH_TRY(launch_fisher_overlap(ctx, dsig.as<int8_t>(), g, nl, dGp.as<int32_t>(), dGi.as<int32_t>(), m, dlen.as<int32_t>(),
                                   didx.as<int32_t>()));
      PH_HIP(hipMemcpyAsync(c.le_len + (size_t)l0 * m, dlen.p, (size_t)m * nl * 4, hipMemcpyDeviceToHost, ctx->stream));
      if (nnz != 0)
        PH_HIP(hipMemcpyAsync(c.le_idx + (size_t)l0 * nnz, didx.p, nnz * nl * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    PH_HIP(hipStreamSynchronize(ctx->stream));
    for (int32_t l = 0; l < nl; ++l) {
      c.tot_out[2 * (size_t)(l0 + l)] = (double)tot[2 * (size_t)l];
      c.tot_out[2 * (size_t)(l0 + l) + 1] = (double)tot[2 * (size_t)l + 1];
    }
    // Benjamini-Hochberg per (list, direction) over the sets that have a p-value: 3 nl independent sorts of m values, which
    // outweigh the kernels from a few lists on -- dealt to host threads when there is enough of them
    const int64_t ncol = 3 * (int64_t)nl;
    auto adjust = [&](int64_t q0, int64_t step) {
      for (int64_t q = q0; q < ncol; q += step) {
        double* o = out + (size_t)(q / 3) * 12 * m;
        p_adjust_fdr(o + (size_t)(3 + q % 3) * m, m, o + (size_t)(6 + q % 3) * m);
      }
    };
    const int64_t nth = std::min<int64_t>({(int64_t)kFisherBhThreads, ncol * m / kFisherBhWork, ncol});
    if (nth <= 1) {
      adjust(0, 1);
    } else {
      std::vector<std::thread> th;
      std::atomic<int> failed{0};
      for (int64_t t = 0; t < nth; ++t)
        th.emplace_back([&, t] {
          try { adjust(t, nth); } catch (...) { failed.store(1); }
        });
      for (auto& t : th) t.join();
      if (failed.load() != 0) { set_error("out of host memory"); return PLAIDHIP_ENOMEM; }
    }
    return PLAIDHIP_OK;
  });
  return s.finish();
}

constexpr int kRankcorThreads = 8;            // host threads of one shard's epilogues and Benjamini-Hochberg columns, at most
constexpr int64_t kRankcorWork = 1 << 16;     // (list, set) pairs per thread below which another thread is not worth its start
// one device's part of plaid.rankcor (kRankcor, kernels_rankcor.hip).  The lists are shared out (plaidhip_shard_bounds over
// c): a shard takes its columns of stat and all of G.  A list's ranks, sums and gathers depend on that list alone (the
// integer ones are exact, the fp64 ones run in an order the launch geometry fixes per list and per set), so every sharding
// has the one-shard bits.  The epilogue and Benjamini-Hochberg of the shard's lists run on the host.  No rendezvous.
int rankcor_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t g = c.g, m = c.m, l0 = s.lo, nl = s.nloc;
  DevBuf dX, dR, dtile, dmask, dsum, dk, dA, dGp, dGi;
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (nl <= 0) return PLAIDHIP_OK;
    PH_HIP(hipSetDevice(ctx->device));
    const int use_rank = c.use_rank;
    const int32_t ntile = (nl + PLAIDHIP_RANKCOR_LIST_TILE - 1) / PLAIDHIP_RANKCOR_LIST_TILE;
    const size_t cell = use_rank ? 4 : 8;
    PH_TRY(dX.alloc((size_t)g * nl * 8));
    PH_TRY(dR.alloc((size_t)g * nl * 8));
    PH_TRY(dtile.alloc((size_t)ntile * g * PLAIDHIP_RANKCOR_LIST_TILE * cell));
    if (!use_rank) PH_TRY(dmask.alloc((size_t)ntile * g));
    PH_TRY(dsum.alloc((size_t)nl * 4 * 8));   // ranks: [nl][3] u64; values: [nl][4] doubles
    PH_TRY(dk.alloc((size_t)nl * m * 4));
    PH_TRY(dA.alloc((size_t)nl * m * 8));
    PH_TRY(upload_pattern(ctx, c.Gp, c.Gi, m, dGp, dGi));
    PH_TRY(upload_pipelined(ctx, dX.as<char>(), (size_t)g * 8, reinterpret_cast<const char*>(c.X + (size_t)l0 * g), (size_t)g * 8,
                            nl, nullptr));
    if (use_rank)
      PH_TRY(launch_colranks_dense_f64(ctx, dX.as<double>(), g, g, nl, c.ties, 0, 1.0, dR.as<double>(), g, nullptr));
    else
      PH_TRY(launch_rankcor_center(ctx, dX.as<double>(), g, nl, dR.as<double>(), dsum.as<double>()));
    PH_TRY(launch_rankcor_pack(ctx, use_rank, dR.as<double>(), g, nl, dtile.p, dmask.as<uint8_t>(),
                               dsum.as<unsigned long long>()));
    PH_TRY(launch_rankcor_gather(ctx, use_rank, dtile.p, dmask.as<uint8_t>(), g, nl, dGp.as<int32_t>(), dGi.as<int32_t>(), m,
                                 dk.as<int32_t>(), dA.p));
    std::vector<int32_t> hk((size_t)nl * m);
    std::vector<int64_t> hA((size_t)nl * m), hsum((size_t)nl * 4);   // (hA, hsum: int64 or the bits of doubles)
    PH_HIP(hipMemcpyAsync(hk.data(), dk.p, hk.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(hA.data(), dA.p, hA.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(hsum.data(), dsum.p, (size_t)nl * (use_rank ? 3 : 4) * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    auto as_double = [](int64_t bits) { double d; std::memcpy(&d, &bits, 8); return d; };
    // the epilogue and Benjamini-Hochberg of every list: nl independent columns of m tails and one sort of m values, which
    // outweigh the kernels from a few lists on -- dealt to host threads when there is enough of them (a list is the same
    // routine whichever thread runs it)
    auto finish_lists = [&](int64_t q0, int64_t step) {
      for (int64_t l = q0; l < nl; l += step) {
        double* o = c.out + (size_t)(l0 + l) * 5 * m;
        const int64_t n = use_rank ? hsum[3 * (size_t)l] : (int64_t)as_double(hsum[4 * (size_t)l]);
        c.tot_out[(size_t)(l0 + l)] = (double)n;
        for (int32_t j = 0; j < m; ++j) {
          const size_t e = (size_t)l * m + j;
          double r[3];
          if (use_rank)
            rankcor_rank_epilogue(n, hsum[3 * (size_t)l + 1], hsum[3 * (size_t)l + 2], hk[e], hA[e], r);
          else
            rankcor_value_epilogue(n, as_double(hsum[4 * (size_t)l + 1]), as_double(hsum[4 * (size_t)l + 2]),
                                   (int)as_double(hsum[4 * (size_t)l + 3]), hk[e], as_double(hA[e]), r);
          o[j] = (double)hk[e];
          o[(size_t)m + j] = r[0];
          o[2 * (size_t)m + j] = r[1];
          o[3 * (size_t)m + j] = r[2];
        }
        p_adjust_fdr(o + 3 * (size_t)m, m, o + 4 * (size_t)m);
      }
    };
    const int64_t nth = std::min<int64_t>({(int64_t)kRankcorThreads, (int64_t)nl * m / kRankcorWork, (int64_t)nl});
    if (nth <= 1) {
      finish_lists(0, 1);
    } else {
      std::vector<std::thread> th;
      std::atomic<int> failed{0};
      for (int64_t t = 0; t < nth; ++t)
        th.emplace_back([&, t] {
          try { finish_lists(t, nth); } catch (...) { failed.store(1); }
        });
      for (auto& t : th) t.join();
      if (failed.load() != 0) { set_error("out of host memory"); return PLAIDHIP_ENOMEM; }
    }
    return PLAIDHIP_OK;
  });
  return s.finish();
}

// one device's part of replaid.plage and replaid.zscore (kPlage, kZscore; kernels_plage.hip).  A gene's moments need all its
// samples and a set's eigenvector all of its rows, so every shard takes all of X (a dgCMatrix as its slots, expanded on the
// device into the dense form, as rowtf = "gauss" does), standardizes, and -- for plage -- forms C and u of EVERY set: the
// same code in the same order on every device, hence the same bits.  The shard then projects (plage) or sums (zscore: the
// crossprod with stat = sum on Z, then the epilogue) its own sample columns.  Shard 0 brings home what does not depend on
// the columns: the per-set statistics and the loadings, or the effective sizes.  No rendezvous.
int plage_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t g = c.g, n = c.n, m = c.m, lo = s.lo, nloc = s.nloc;
  const bool plage = c.method == kPlage;
  const bool writer = k == 0;
  const bool idle = nloc <= 0 && !writer;
  const size_t z = (size_t)std::max<int32_t>(c.Gp[m], 1);
  const int64_t ldz = plage ? plage_row_ld(n) : (int64_t)g;
  s.force_f64();   // (zscore's crossprod stays on the fp64 kernels whatever precision the context was given)
  plaidhip_geneset* gs = nullptr;
  DevBuf dfull, dp, di, dx, ddflt, dmom, dflag, dGp, dGi, dCi, dCpos, dkf, dZ, dU, dstats, dL, dS;
  HomeBuffer home;
  std::vector<int32_t> hk;

  // ---- all of X, the moments, the kept members, Z --------------------------------------------------------------------------
  s.step([&]() -> int {
    if (idle) return PLAIDHIP_OK;
    PH_HIP(hipSetDevice(ctx->device));
    PH_TRY(dfull.alloc((size_t)g * n * 8));
    if (c.Xp == nullptr) {
      PH_TRY(upload_host(ctx, dfull.p, (size_t)g * 8, c.X, (size_t)g * 8, n));
    } else {
      const int64_t zx = c.Xp[n];
      PH_TRY(dp.alloc((size_t)(n + 1) * 4));
      PH_TRY(di.alloc((size_t)std::max<int64_t>(zx, 1) * 4));
      PH_TRY(dx.alloc((size_t)std::max<int64_t>(zx, 1) * 8));
      PH_TRY(ddflt.alloc((size_t)g * 8));
      PH_HIP(hipMemcpyAsync(dp.p, c.Xp, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
      PH_TRY(upload_host(ctx, di.p, 1, c.Xi, 1, zx * 4));
      PH_TRY(upload_host(ctx, dx.p, 1, c.X, 1, zx * 8));
      PH_HIP(hipMemsetAsync(ddflt.p, 0, (size_t)g * 8, ctx->stream));   // (the rows' default: a zero)
      PH_TRY(launch_csc_expand(ctx, dp.as<int32_t>(), di.as<int32_t>(), dx.as<double>(), g, n, g, ddflt.as<double>(), nullptr,
                               nullptr, dfull.as<double>()));
    }
    PH_TRY(dmom.alloc((size_t)g * 2 * 8));
    PH_TRY(dflag.alloc((size_t)g * 4));
    double* d_mean = dmom.as<double>();
    double* d_sd = d_mean + g;
    PH_TRY(launch_plage_moments(ctx, dfull.as<double>(), g, g, n, d_mean, d_sd, dflag.as<int32_t>()));
    PH_TRY(upload_pattern(ctx, c.Gp, c.Gi, m, dGp, dGi));
    PH_TRY(dCi.alloc(z * 4));
    PH_TRY(dCpos.alloc(z * 4));
    PH_TRY(dkf.alloc((size_t)m * 2 * 4));   // [keff | nanflag]
    PH_TRY(launch_plage_compact(ctx, dGp.as<int32_t>(), dGi.as<int32_t>(), m, dflag.as<int32_t>(), dCi.as<int32_t>(),
                                dCpos.as<int32_t>(), dkf.as<int32_t>(), dkf.as<int32_t>() + m));
    PH_TRY(dS.alloc((size_t)m * std::max(nloc, 1) * 8));
    if (plage) {
      PH_TRY(dZ.alloc((size_t)g * ldz * 8));
      PH_TRY(launch_plage_standardize_rows(ctx, dfull.as<double>(), g, g, n, d_mean, d_sd, dflag.as<int32_t>(), dZ.as<double>(),
                                           ldz));
    } else if (nloc > 0) {
      PH_TRY(acquire_geneset(ctx, g, m, c.Gp, c.Gi, &gs));
      PH_TRY(dZ.alloc((size_t)g * nloc * 8));
      PH_TRY(launch_plage_standardize_columns(ctx, dfull.as<double>(), g, g, lo, nloc, d_mean, d_sd, dflag.as<int32_t>(),
                                              dZ.as<double>(), ldz));
    }
    if (nloc > 0) home.prepare(c.S_out + (int64_t)lo * m, (size_t)m * nloc * 8);
    return PLAIDHIP_OK;
  });

  // ---- plage: C, u and the projection; zscore: the crossprod and its epilogue -----------------------------------------------
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (idle) return PLAIDHIP_OK;
    const int32_t* d_keff = dkf.as<int32_t>();
    const int32_t* d_nan = d_keff + m;
    if (plage) {
      PH_TRY(dU.alloc(z * 8));
      PH_TRY(dstats.alloc((size_t)m * 6 * 8));
      if (writer && c.load_out != nullptr) PH_TRY(dL.alloc(z * 8));
      PH_TRY(launch_plage_sets(ctx, dZ.as<double>(), ldz, c.Gp, dGp.as<int32_t>(), dCi.as<int32_t>(), dCpos.as<int32_t>(), d_keff,
                               d_nan, m, c.tol, c.maxit, dU.as<double>(), dstats.as<double>(), dL.as<double>()));
      return launch_plage_project(ctx, dZ.as<double>(), ldz, dGp.as<int32_t>(), dCi.as<int32_t>(), d_keff, d_nan, dU.as<double>(),
                                  dstats.as<double>(), m, lo, nloc, dS.as<double>(), m);
    }
    if (nloc <= 0) return PLAIDHIP_OK;
    PH_TRY(launch_spmm_dense_f64(ctx, gs, dZ.as<double>(), ldz, nloc, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0, dS.as<double>(), m,
                                 nullptr));
    return launch_zscore_epilogue(ctx, dS.as<double>(), m, m, nloc, d_keff, d_nan);
  });

  // ---- the score shard goes home; shard 0 brings the per-set results ----------------------------------------------------------
  s.step([&]() -> int {
    if (idle) return PLAIDHIP_OK;
    if (nloc > 0) PH_TRY(home.copy(ctx, dS.p));
    if (writer && plage && c.out != nullptr)
      PH_HIP(hipMemcpyAsync(c.out, dstats.p, (size_t)m * 6 * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (writer && plage && c.load_out != nullptr && c.Gp[m] > 0)
      PH_HIP(hipMemcpyAsync(c.load_out, dL.p, (size_t)c.Gp[m] * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (writer && !plage && c.out != nullptr) {
      hk.resize((size_t)m);
      PH_HIP(hipMemcpyAsync(hk.data(), dkf.p, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    PH_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t j = 0; j < hk.size(); ++j) c.out[j] = (double)hk[j];
    return PLAIDHIP_OK;
  });
  return s.finish();
}

}  // namespace plaidhip
