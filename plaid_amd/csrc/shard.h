// The sharded engine's scaffold (shard.cpp) and what its worker families (shard_*.cpp) share: the rendezvous, the
// cross-shard state, one shard's columns and status, the shared blocks, and every family's worker, prepare and tail.
// Host only, private to shard.cpp, shard_*.cpp and multi.cpp.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "call.h"

#define PH_TRY(expr)                      \
  do {                                    \
    int rc_ = (expr);                     \
    if (rc_ != PLAIDHIP_OK) return rc_;   \
  } while (0)

#ifdef PLAIDHIP_DIAG
#define PH_TRACE(tag)                                                                                              \
  do {                                                                                                             \
    if (getenv("PLAIDHIP_TRACE"))                                                                                  \
      fprintf(stderr, "[trace] %-22s %8.2f ms\n", tag,                                                             \
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_trace0).count());     \
  } while (0)
#else
#define PH_TRACE(tag) do { } while (0)
#endif

namespace plaidhip {

// all threads of a sharded call meet here between phases; a thread that failed keeps arriving (doing nothing in
// between), so nobody waits forever
class Rendezvous {
 public:
  explicit Rendezvous(int n) : n_(n) {}
  void arrive_and_wait() {
    std::unique_lock<std::mutex> lk(mu_);
    const int gen = gen_;
    if (++count_ == n_) {
      count_ = 0;
      ++gen_;
      cv_.notify_all();
    } else {
      cv_.wait(lk, [&] { return gen_ != gen; });
    }
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  int n_, count_ = 0, gen_ = 0;
};

// What the shards of one call share.  The scaffold's own fields first; then one struct per family, sized by that family's
// prepare (route, shard.cpp) and touched by nobody else.
struct Shared {
  explicit Shared(int n) : rv(n) {}
  Rendezvous rv;
  std::mutex mu;
  std::atomic<int> abort{0};
  double gmax = 0.0;               // max(rX) over all shards
  bool gmax_set = false;
  uint32_t flags[4] = {0, 0, 0, 0};
  std::vector<double> med_all;     // medx of every sample column, global column order (each shard writes its block)
  // replaid.scse: min / max of X over all shards, in the comparisons of minmax_final_kernel (kernels_norm.hip)
  double xmin = INFINITY, xmax = -INFINITY;
  bool removed_log2 = false;
  // replaid.ssgsea.exact with norm: a NaN among the scores of any shard (its min / max go to xmin / xmax)
  bool es_nan = false;
  // replaid.gsva's z row transform.  Dense X: the running row sums (then sums of squared deviations) handed from shard to
  // shard; a dgCMatrix: every shard's row sums of stored values, then of squared deviations, and row lengths
  struct Gsva {
    std::vector<double> chain_sum, chain_ssd;
    std::vector<std::vector<double>> row_sum, row_ssd;
    std::vector<std::vector<int32_t>> row_len;
  } gsva;
  // plaid.test and plaid.test.contrasts ([C] of each): the chained two-group sums ([2][rows]) of X (dense), of the score rows
  // and of their squared deviations; a dgCMatrix's per-shard stored-value sums; shard 0's T = Gt [fc, fc^2] and
  // F = [fc, fc^2] (leading dimension even_ld(g))
  struct PlaidTest {
    std::vector<double> chain_x, chain_s, chain_q, T, F;
    std::vector<std::vector<double>> row_sum;
  } pt;
  // plaid.limma and plaid.camera: the chained effects [W][rows] and residual sums of squares [nfit][rows].  na = "fit": every
  // shard's NaN per row and their (global) columns, row after row; the NaN of every (fit, row) inside the fit's used samples,
  // added over the shards; then, from shard 0, df.residual [nfit][rows] (NaN: not fitted) and u [nfit q][rows]
  struct Limma {
    std::vector<double> effects, rss;
    std::vector<std::vector<int32_t>> na_cnt, na_list;
    std::vector<int32_t> na_pair;
    std::vector<double> na_d, na_u;
    // with weights: the chained weighted sums [nfit Wc][rows] and counts [2 nfit + 1][rows]; shard 0's solve then fills
    // effects (gamma and AveExpr), na_d and na_u
    std::vector<double> wsum, wcnt;
  } limma;
  // plaid.voom: a count that is not finite and >= 0 on any shard; every column's sum (each shard writes its block); the chained
  // row sums [rows]; the library sizes used and the offsets; shard 0's knots (limma.effects / limma.rss take the unweighted fit)
  struct Voom {
    uint32_t bad = 0;
    std::vector<double> colsum, rowsum, lib, off, kx, ky;
  } voom;
  // plaid.camera: the chained sums over the samples of T^2, [nfit][m] (T = G'Z of every fit)
  struct Camera { std::vector<double> ss; } camera;
  // plaid.fry: the divisors [nfit][rows] (shard 0 makes them after the RSS chain); the chained residual effects of every
  // fit under the cap, [d + 1][rows] each (camera.ss takes the sums of T^2)
  struct Fry {
    std::vector<double> cg;
    std::vector<std::vector<double>> rho;
  } fry;
  // plaid.roast: the generated rotations of every fit ((n + 1) x nrot; empty: the caller's), the counts added over the shards
  // ([nfit q][m][4]), and from shard 0 the set sizes, the members beyond -+sqrt(2) and the hyperparameters
  struct Roast {
    std::vector<std::vector<double>> W;
    std::vector<int32_t> cnt;
    std::vector<double> msize, ndown, nup, hyper;
  } roast;
  // plaid.romer (roast.W takes the generated rotations): the counts added over the shards ([nfit q][m][3]), and from shard 0
  // the set sizes and the hyperparameters ([nfit][8 + q])
  struct Romer {
    std::vector<int32_t> cnt;
    std::vector<double> msize, hyper;
  } romer;
  // plaid.gsea: the block partials [nblk][c][6][m] of all permutation blocks, each shard writing its own blocks; multilevel:
  // (qhat, log2err, stage, status) of every (list, set), NaN without a ruler, each shard writing the sets of its own rulers
  struct Gsea { std::vector<double> part, ml; } gsea;
};

// columns [lo, lo + nloc) of shard k: cut at multiples of kRowColBlock (row_pair.h, 128 columns) for the methods whose
// chained row reductions add the block partials of the one-device call in the same order (route's block_cut); everything
// else takes plaidhip_shard_bounds.
void shard_columns(const Call& c, int ndev, int k, int32_t* lo, int32_t* nloc);

inline int64_t even_ld(int32_t g) { return (int64_t)g + (g & 1); }

// device buffers that live in the context between calls (ctx_buffer); same interface as DevBuf
struct CtxBuf {
  plaidhip_ctx* ctx;
  int slot;
  void* p = nullptr;
  int alloc(size_t bytes) { return ctx_buffer(ctx, slot, bytes, &p); }
  template <typename T> T* as() { return static_cast<T*>(p); }
};

// What every worker runs on: shard k of ndev, its columns, its status.  Every `step` is skipped once this shard or
// any other has failed; the rendezvous points between the steps are always reached.
struct Shard {
  plaidhip_ctx* ctx;
  const Call& c;
  int ndev, k;
  Shared& sh;
  int32_t lo = 0, nloc = 0;
  int64_t zx = 0;             // a dgCMatrix: the stored values of the shard's columns
  int rc = PLAIDHIP_OK;
  int saved_precision = -1;   // >= 0: the context's precision, given back by finish()

  Shard(plaidhip_ctx* ctx_, const Call& c_, int ndev_, int k_, Shared& sh_) : ctx(ctx_), c(c_), ndev(ndev_), k(k_), sh(sh_) {
    shard_columns(c, ndev, k, &lo, &nloc);
    if (c.Xp != nullptr) zx = (int64_t)c.Xp[lo + nloc] - c.Xp[lo];
  }
  bool live() const { return rc == PLAIDHIP_OK && sh.abort.load() == 0; }
  template <typename Fn> void step(Fn&& fn) {
    if (!live()) return;
    try {
      rc = fn();
    } catch (...) {   // (a worker thread has no function-try-block above it; the rendezvous points must still be reached)
      rc = on_exception();
    }
    if (rc != PLAIDHIP_OK) sh.abort.store(1);
  }
  // the exact scorers are fp64 and integers in every mode: their crossprods stay on the fp64 kernels
  void force_f64() {
    saved_precision = ctx->precision;
    ctx->precision = PLAIDHIP_PRECISION_F64;
  }
  int finish() {
    if (saved_precision >= 0) ctx->precision = saved_precision;
    if (rc == PLAIDHIP_OK && sh.abort.load() != 0) {
      hipStreamSynchronize(ctx->stream);
      return PLAIDHIP_EHIP;   // another shard failed; its error text is reported
    }
    if (rc != PLAIDHIP_OK) hipStreamSynchronize(ctx->stream);
    return rc;
  }
};

// ---- the shared blocks (shard.cpp) ---------------------------------------------------------------------------------------
// pageable host -> device through the context's pinned ring; on_panel(c0, c1) (may be empty) enqueues what consumes a panel
int upload_pipelined(plaidhip_ctx* ctx, char* dst, size_t ldd_bytes, const char* src, size_t row_bytes, int64_t cols,
                     const std::function<int(int64_t, int64_t)>& on_panel);

// The CSC slots of the shard's columns go to the device: @p rebased to the shard (ploc, which the caller keeps until its
// last synchronisation), @i and the values through the pinned ring.  *max_nnz: the shard's longest column.  dXx: a CtxBuf
// or a DevBuf.
template <typename Buf>
int upload_csc_shard(const Shard& s, std::vector<int32_t>& ploc, CtxBuf& dXp, CtxBuf& dXi, Buf& dXx, int32_t* max_nnz) {
  const Call& c = s.c;
  const int64_t z0 = c.Xp[s.lo];
  ploc.resize((size_t)s.nloc + 1);
  for (int32_t j = 0; j <= s.nloc; ++j) ploc[(size_t)j] = (int32_t)(c.Xp[s.lo + j] - z0);
  *max_nnz = host_max_col_nnz(ploc.data(), s.nloc);
  const size_t zb = (size_t)std::max<int64_t>(s.zx, 1);
  PH_TRY(dXp.alloc((size_t)(s.nloc + 1) * 4));
  PH_TRY(dXi.alloc(zb * 4));
  PH_TRY(dXx.alloc(zb * 8));
  PH_HIP(hipMemcpyAsync(dXp.p, ploc.data(), (size_t)(s.nloc + 1) * 4, hipMemcpyHostToDevice, s.ctx->stream));
  PH_TRY(upload_pipelined(s.ctx, dXi.template as<char>(), 1, reinterpret_cast<const char*>(c.Xi + z0), 1, s.zx * 4, nullptr));
  return upload_pipelined(s.ctx, dXx.template as<char>(), 1, reinterpret_cast<const char*>(c.X + z0), 1, s.zx * 8, nullptr);
}

// the pattern of a set collection (aligned to X's rows) for the kernels that walk it
int upload_pattern(plaidhip_ctx* ctx, const int32_t* Gp, const int32_t* Gi, int32_t m, DevBuf& dGp, DevBuf& dGi);
// this shard's {min, max} (and "a NaN among them") into the range over all shards
void merge_range(Shard& s, double mn, double mx, bool any_nan = false);
// normalize_medians up to mean(medx): the shard's medians (left in d_med) and the mean over ALL columns.  Two rendezvous.
double medians_and_their_mean(Shard& s, double* dS, const uint32_t* d_flags, double* d_med);
// chained, ordered reduction over the samples of [nblk][groups][rows] block partials, group by group.  ndev rendezvous.
void chain_block_sums(Shard& s, std::vector<double>& run, const double* ws, int32_t rows, int groups, double* d_seed,
                      double* d_run);
// the same for any [nblk][len] partials at once (launch_reduce_blocks_flat).  ndev rendezvous.
void chain_flat_sums(Shard& s, std::vector<double>& run, const double* ws, int64_t len, double* d_seed, double* d_run);
// {sum, count} of the non-NaN entries of v in exactly the order of sum_kernel (kernels_norm.hip)
double mean_like_device_sum(const double* v, int64_t count);

// ---- the families: one device's part of a call, what sizes their part of Shared, their host half after the workers --------
int shard_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);              // shard_rank_sum.cpp
int scorer_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);             // shard_scorer.cpp
void gsva_prepare(Shared& sh, const Call& c, int ndev);
int scse_tail(plaidhip_ctx* first, const Call& c, Shared& sh);
int ssgsea_exact_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);       // shard_exact.cpp
int sing_exact_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);
int truncated_exact_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);
int plaid_test_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);         // shard_plaid_test.cpp
bool plaid_test_empty(const Call& c);
void plaid_test_prepare(Shared& sh, const Call& c, int ndev);
int plaid_test_tail(plaidhip_ctx* first, const Call& c, Shared& sh);
int gsea_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);               // shard_gsea.cpp
int gsea_ruler_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);
void gsea_prepare(Shared& sh, const Call& c, int ndev);
int fisher_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);             // shard_lists.cpp
int rankcor_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);
int plage_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);
int limma_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);              // shard_limma.cpp
int limma_w_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);            // shard_limma_w.cpp
int voom_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);               // shard_voom.cpp
bool voom_empty(const Call& c);
void voom_prepare(Shared& sh, const Call& c, int ndev);
// the trend of plaid.voom on the host (include/plaidhip.h, steps 4 - 6): the knots from M, s2 and the row sums; EINVAL
// without a row to fit it on
int voom_trend_knots(int32_t rows, const double* M, const double* s2, const double* rowsum, const double* lib, int32_t n,
                     double span, std::vector<double>& kx, std::vector<double>& ky);
bool limma_empty(const Call& c);
void limma_prepare(Shared& sh, const Call& c, int ndev);
int limma_tail(plaidhip_ctx* first, const Call& c, Shared& sh);
int camera_tail(plaidhip_ctx* first, const Call& c, Shared& sh);
int fry_tail(plaidhip_ctx* first, const Call& c, Shared& sh);
int roast_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);
void roast_prepare(Shared& sh, const Call& c, int ndev);
int roast_tail(plaidhip_ctx* first, const Call& c, Shared& sh);
int romer_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh);              // shard_romer.cpp
void romer_prepare(Shared& sh, const Call& c, int ndev);
int romer_tail(plaidhip_ctx* first, const Call& c, Shared& sh);

// ---- what the engine knows about a method on the run side (shard.cpp) --------------------------------------------------------
struct Route {
  bool block_cut;                                              // shards cut at multiples of 128 columns
  bool (*empty)(const Call&);                                  // no result to compute: return before a device is touched
  void (*prepare)(Shared&, const Call&, int ndev);             // sizes the family's part of Shared (may be null)
  int (*worker)(plaidhip_ctx*, const Call&, int ndev, int k, Shared&);
  int (*tail)(plaidhip_ctx* first, const Call&, Shared&);      // the host half after the workers (may be null)
};
Route route(const Call& c);
// every shard on a thread of its own (one shard: the calling thread); the first failure's text is reported
int run_call(plaidhip_ctx* const* ctxs, int ndev, const Call& c);

}  // namespace plaidhip
