// Host-buffer pipelines for one or several GPUs of a node, driven from ONE host process.
//
// The reference is a single R process (no process-per-GPU runtime to lean on), so the multi-GPU form of the host entry
// points is a thread per device inside the library: the sample columns are cut into contiguous shards
// (plaidhip_shard_bounds: ceil(n / ndev) columns each, R's column-major layout makes a shard one byte range of X and of
// S), every device moves its shard over its own PCIe link, and the three scalars that couple the samples -- max(rX)
// (R/plaid.R:251), min(x) == 0 (R/plaid.R:556-557) and mean(medx) (R/plaid.R:572) -- are combined on the host between
// the phases.  No RCCL: nothing but those scalars crosses between devices.  (One process per GPU over RCCL is the
// other form, plaid_amd/sharded.py.)  The single-device entry points of api.cpp run the same code with one shard:
// there is one implementation per scorer, and a context entry is its one-shard case.
// replaid.ucell / aucell / scse / gsva (scorer_worker) add their own couplings: the min / max behind removeLog2 = NULL and
// the per-gene mean and sd of gsva's z transform (g values each, chained from shard to shard for dense X).  plaid.test
// (plaid_test_worker) reduces nothing but row sums over the samples: its scores stay on the devices.  The workers are
// plain functions over one scaffold (Shard: the columns, `step`, the common exit) and a few shared blocks (the CSC
// upload, the medians' coupling, the chained row reductions).
//
// Uploads are pipelined: R hands over pageable memory, which the HIP runtime copies at ~21 GB/s; staged through
// pinned buffers by a few feeder threads (memcpy at ~75 GB/s with four threads, tools/ubench/pcie.cpp) the DMA
// runs at the link rate (~57 GB/s) and the kernels of a column panel start as soon as the panel has landed.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <chrono>
#include <thread>
#include <vector>

#include <sys/mman.h>

#include "call.h"

using namespace plaidhip;

#define PH_TRY(expr)                      \
  do {                                    \
    int rc_ = (expr);                     \
    if (rc_ != PLAIDHIP_OK) return rc_;   \
  } while (0)

extern "C" int plaidhip_shard_bounds(int64_t n, int ndev, int k, int64_t* lo, int64_t* hi) try {
  PH_REQUIRE(n >= 0 && ndev > 0 && k >= 0 && k < ndev && lo && hi, "shard_bounds: bad arguments n=%lld ndev=%d k=%d",
             (long long)n, ndev, k);
  const int64_t per = (n + ndev - 1) / ndev;
  *lo = std::min(n, (int64_t)k * per);
  *hi = std::min(n, *lo + per);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

namespace plaidhip {

// ---- HomeBuffer ---------------------------------------------------------------------------------------------------------
struct HomeBuffer::State {
  char* dst = nullptr;
  size_t bytes = 0, nchunk = 0;
  std::vector<std::atomic<int>> done;
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  explicit State(size_t n) : done(n) {}
};
namespace {
constexpr size_t kHomeChunk = (size_t)64 << 20;
constexpr size_t kHomeMin = (size_t)16 << 20;   // below this one plain copy (a few thousand page faults)
constexpr int kHomeThreads = 8;                 // touching 4.9 GB of huge pages: 29 ms with 8 threads, 68 with 4 (ubench)
}  // namespace

void HomeBuffer::prepare(void* dst, size_t bytes) {
  finish();
  const size_t nchunk = bytes >= kHomeMin ? (bytes + kHomeChunk - 1) / kHomeChunk : 0;
  st_ = new State(nchunk);
  st_->dst = static_cast<char*>(dst);
  st_->bytes = bytes;
  st_->nchunk = nchunk;
  if (nchunk == 0) return;
  for (auto& d : st_->done) d.store(0, std::memory_order_relaxed);
  {
    const uintptr_t b = ((uintptr_t)dst + 4095) & ~(uintptr_t)4095, e = ((uintptr_t)dst + bytes) & ~(uintptr_t)4095;
    if (e > b) (void)madvise(reinterpret_cast<void*>(b), e - b, MADV_HUGEPAGE);
  }
  unsigned hw = std::thread::hardware_concurrency();
  const int nt = (int)std::max<size_t>(1, std::min<size_t>({(size_t)kHomeThreads, nchunk, hw > 1 ? hw / 2 : 1}));
  State* st = st_;
  auto spawn = [&](auto&& body) {   // (a thread the system refuses is one helper less, not an exception through a C ABI)
    try {
      st_->th.emplace_back(body);
    } catch (...) {
    }
  };
  for (int t = 0; t < nt; ++t)
    spawn([st] {
      for (;;) {
        const size_t k = st->next.fetch_add(1);
        if (k >= st->nchunk) return;
        const size_t b = k * kHomeChunk, e = std::min(st->bytes, b + kHomeChunk);
        // one write per 4 KiB page, at the page's first byte inside the buffer
        for (size_t o = b; o < e; o = ((((uintptr_t)st->dst + o) | 4095) + 1) - (uintptr_t)st->dst)
          *reinterpret_cast<volatile char*>(st->dst + o) = 0;
        st->done[k].store(1, std::memory_order_release);
      }
    });
  if (st_->th.empty()) st_->nchunk = 0;   // no helper at all: one plain copy (copy() below)
}

int HomeBuffer::copy(plaidhip_ctx* ctx, const void* src_dev) {
  PH_REQUIRE(st_ != nullptr, "HomeBuffer::copy before prepare");
  if (st_->bytes == 0) return PLAIDHIP_OK;
  if (st_->nchunk == 0) {
    PH_HIP(hipMemcpyAsync(st_->dst, src_dev, st_->bytes, hipMemcpyDeviceToHost, ctx->stream));
    return PLAIDHIP_OK;
  }
  for (size_t k = 0; k < st_->nchunk; ++k) {
    while (st_->done[k].load(std::memory_order_acquire) == 0) std::this_thread::yield();
    const size_t b = k * kHomeChunk, len = std::min(kHomeChunk, st_->bytes - b);
    PH_HIP(hipMemcpyAsync(st_->dst + b, static_cast<const char*>(src_dev) + b, len, hipMemcpyDeviceToHost, ctx->stream));
  }
  return PLAIDHIP_OK;
}

void HomeBuffer::finish() {
  if (st_ == nullptr) return;
  for (auto& t : st_->th) t.join();
  delete st_;
  st_ = nullptr;
}

int copy_home(plaidhip_ctx* ctx, void* dst, const void* src_dev, size_t bytes) {
  HomeBuffer hb;
  hb.prepare(dst, bytes);
  const int rc = hb.copy(ctx, src_dev);
  hb.finish();
  return rc;
}

}  // namespace plaidhip

namespace {

constexpr size_t kPanelBytes = (size_t)48 << 20;   // pinned staging buffer: 2 per feeder thread

int ensure_pinned(plaidhip_ctx* ctx) {
  if (ctx->pin_bytes >= kPanelBytes) return PLAIDHIP_OK;
  // whatever a partial failure leaves behind stays recorded in the context (null-checked here, freed by plaidhip_finalize)
  for (int t = 0; t < plaidhip_ctx::kFeeders; ++t) {
    for (int b = 0; b < 2; ++b)
      if (ctx->pin[t][b] == nullptr) PH_HIP(hipHostMalloc(&ctx->pin[t][b], kPanelBytes, hipHostMallocDefault));
    if (ctx->copy_stream[t] == nullptr) PH_HIP(hipStreamCreateWithFlags(&ctx->copy_stream[t], hipStreamNonBlocking));
  }
  ctx->pin_bytes = kPanelBytes;
  return PLAIDHIP_OK;
}

// Host (pageable) -> device copy of `rows x cols` column-major doubles (or of a flat byte array: rows = bytes per
// "column") with destination leading dimension ldd, pipelined through the context's pinned buffers.  `on_panel(c0, c1)`
// (may be empty) is called on the calling thread, in column order, after the compute stream has been made to wait for
// the panel's DMA: it enqueues whatever consumes columns [c0, c1).
int upload_pipelined(plaidhip_ctx* ctx, char* dst, size_t ldd_bytes, const char* src, size_t row_bytes, int64_t cols,
                     const std::function<int(int64_t, int64_t)>& on_panel) {
  if (cols == 0 || row_bytes == 0) return PLAIDHIP_OK;
  if (row_bytes * (size_t)cols < ((size_t)8 << 20) || 2 * ldd_bytes > kPanelBytes) {
    // small input, or columns so long that a panel of two (the least the pair kernel takes) overflows a staging
    // buffer: one plain copy
    if (ldd_bytes == row_bytes) {
      PH_HIP(hipMemcpyAsync(dst, src, row_bytes * (size_t)cols, hipMemcpyHostToDevice, ctx->stream));
    } else {
      PH_HIP(hipMemcpy2DAsync(dst, ldd_bytes, src, row_bytes, row_bytes, (size_t)cols, hipMemcpyHostToDevice, ctx->stream));
    }
    return on_panel ? on_panel(0, cols) : PLAIDHIP_OK;
  }
  PH_TRY(ensure_pinned(ctx));
  constexpr int T = plaidhip_ctx::kFeeders;
  const int64_t pcols = std::max<int64_t>(1, (int64_t)(kPanelBytes / ldd_bytes));
  // panel boundaries: the first round of panels (one per feeder) is an eighth of the size, the second a half -- the
  // bus starts after a fraction of a millisecond of staging instead of after a whole 48 MB memcpy (measured: 3.3 ms
  // of fill in front of the first DMA with equal panels)
  std::vector<int64_t> pb{0};
  for (int64_t r = 0; pb.back() < cols; ++r) {
    int64_t w = r < T ? pcols / 8 : (r < 2 * T ? pcols / 2 : pcols);
    w = std::max<int64_t>(2, w & ~(int64_t)1);   // even: the pair kernel takes two columns per pass
    pb.push_back(std::min(cols, pb.back() + w));
  }
  const int64_t npan = (int64_t)pb.size() - 1;
  struct Events {   // destroyed on every exit path
    std::vector<hipEvent_t> v;
    ~Events() { for (hipEvent_t e : v) if (e) hipEventDestroy(e); }
    hipEvent_t& operator[](size_t i) { return v[i]; }
  } done;
  done.v.assign((size_t)npan, nullptr);
  for (auto& e : done.v) PH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  std::vector<std::atomic<int>> ready((size_t)npan);
  for (auto& r : ready) r.store(0, std::memory_order_relaxed);
  std::atomic<int> failed{0};
  const int device = ctx->device;
  auto feeder = [&](int t) {
    if (hipSetDevice(device) != hipSuccess) { failed.store(1); }
    hipEvent_t freeb[2] = {nullptr, nullptr};
    for (int64_t p = t, it = 0; p < npan; p += T, ++it) {
      const int b = (int)(it & 1);
      const int64_t c0 = pb[(size_t)p], c1 = pb[(size_t)p + 1];
      bool ok = failed.load() == 0;
      if (ok && freeb[b] != nullptr) ok = hipEventSynchronize(freeb[b]) == hipSuccess;   // the DMA that last read this buffer
      if (ok) {
        char* stage = static_cast<char*>(ctx->pin[t][b]);
        if (ldd_bytes == row_bytes) {
          memcpy(stage, src + (size_t)c0 * row_bytes, (size_t)(c1 - c0) * row_bytes);
        } else {
          for (int64_t c = c0; c < c1; ++c) memcpy(stage + (size_t)(c - c0) * ldd_bytes, src + (size_t)c * row_bytes, row_bytes);
        }
        ok = hipMemcpyAsync(dst + (size_t)c0 * ldd_bytes, stage, (size_t)(c1 - c0) * ldd_bytes, hipMemcpyHostToDevice,
                            ctx->copy_stream[t]) == hipSuccess;
        if (ok) ok = hipEventRecord(done[(size_t)p], ctx->copy_stream[t]) == hipSuccess;
        if (ok) {
          if (freeb[b] == nullptr) ok = hipEventCreateWithFlags(&freeb[b], hipEventDisableTiming) == hipSuccess;
          if (ok) ok = hipEventRecord(freeb[b], ctx->copy_stream[t]) == hipSuccess;
        }
      }
      if (!ok) failed.store(1);
      ready[(size_t)p].store(1, std::memory_order_release);
    }
    for (int b = 0; b < 2; ++b)
      if (freeb[b] != nullptr) { hipEventSynchronize(freeb[b]); hipEventDestroy(freeb[b]); }
  };
  std::vector<std::thread> th;
  th.reserve((size_t)T);
  for (int t = 0; t < T && t < npan; ++t) {
    try {
      th.emplace_back(feeder, t);
    } catch (...) {   // (a thread the system refuses: its panels are staged by this thread, before the loop below waits)
      feeder(t);
    }
  }
  int rc = PLAIDHIP_OK;
  try {
    for (int64_t p = 0; p < npan; ++p) {
      while (ready[(size_t)p].load(std::memory_order_acquire) == 0) std::this_thread::yield();
      if (failed.load() != 0 || rc != PLAIDHIP_OK) continue;
      if (hipStreamWaitEvent(ctx->stream, done[(size_t)p], 0) != hipSuccess) { failed.store(1); continue; }
      if (on_panel) rc = on_panel(pb[(size_t)p], pb[(size_t)p + 1]);
    }
  } catch (...) {   // (the feeders hold references into this frame: they are joined before anything unwinds)
    failed.store(1);
    for (auto& t : th) t.join();
    throw;
  }
  for (auto& t : th) t.join();
  if (failed.load() != 0 && rc == PLAIDHIP_OK) {
    set_error("pipelined host-to-device copy failed (%s)", hipGetErrorString(hipGetLastError()));
    rc = PLAIDHIP_EHIP;
  }
  return rc;
}

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

struct Shared {
  explicit Shared(int n) : rv(n) {}
  Rendezvous rv;
  std::mutex mu;
  double gmax = 0.0;               // max(rX) over all shards
  bool gmax_set = false;
  uint32_t flags[4] = {0, 0, 0, 0};
  std::vector<double> med_all;     // medx of every sample column, global column order (each shard writes its block)
  std::atomic<int> abort{0};
  // replaid.scse: min / max of X over all shards, in the comparisons of minmax_final_kernel (kernels_norm.hip)
  double xmin = INFINITY, xmax = -INFINITY;
  bool removed_log2 = false;
  // replaid.gsva, dense X: the running row sums (then sums of squared deviations) handed from shard to shard
  std::vector<double> chain_sum, chain_ssd;
  // replaid.gsva, dgCMatrix: every shard's row sums of stored values, then of squared deviations, and row lengths
  std::vector<std::vector<double>> row_sum, row_ssd;
  std::vector<std::vector<int32_t>> row_len;
  // plaid.test: the chained two-group sums ([2][rows]) of X (dense), of the score rows and of their squared deviations;
  // shard 0's T = Gt [fc, fc^2] and F = [fc, fc^2] (leading dimension even_ld(g)); a dgCMatrix's per-shard stored-value
  // sums go to row_sum
  // plaid.limma: chain_x is the chained effects [W][rows], chain_q the chained residual sums of squares [nfit][rows]
  std::vector<double> chain_x, chain_s, chain_q, pt_T, pt_F;
  // plaid.limma with na = "fit": every shard's NaN per row and their (global) columns, row after row; the NaN of every
  // (fit, row) inside the fit's used samples, added over the shards; then, from shard 0, df.residual [nfit][rows] (NaN: not
  // fitted) and u [nfit q][rows]
  std::vector<std::vector<int32_t>> na_cnt, na_list;
  std::vector<int32_t> na_pair;
  std::vector<double> na_d, na_u;
  // plaid.camera: the chained sums over the samples of T^2, [nfit][m] (T = G'Z of every fit)
  std::vector<double> cam_ss;
  // replaid.ssgsea.exact with norm: a NaN among the scores of any shard (its min / max go to xmin / xmax)
  bool es_nan = false;
  // plaid.gsea: the block partials [nblk][c][6][m] of all permutation blocks, each shard writing its own blocks
  std::vector<double> gsea_part;
  // plaid.gsea's multilevel p-values: (qhat, log2err, stage, status) of every (list, set), NaN without a ruler; each shard
  // writes the sets of its own rulers
  std::vector<double> gsea_ml;
};

// columns [lo, lo + nloc) of shard k.  Dense replaid.gsva and plaid.test (dense or not: its score rows are chained too)
// (and replaid.gsva.exact with its z transform) cut at multiples of kColBlock (kernels_stats.hip, 128 columns) so that their chained row reductions add the block
// partials of the one-device call in the same order; everything else takes plaidhip_shard_bounds.
void shard_columns(const Call& c, int ndev, int k, int32_t* lo, int32_t* nloc) {
  int64_t lo64 = 0, hi64 = 0;
  if (((c.method == kGsva || (c.method == kGsvaExact && c.rowtf == 0)) && c.Xp == nullptr) || c.method == kPlaidTest ||
      c.method == kPlaidTestContrasts || c.method == kLimma || c.method == kCamera) {
    constexpr int64_t kBlock = 128;
    const int64_t per = kBlock * (((c.n + kBlock - 1) / kBlock + ndev - 1) / ndev);
    lo64 = std::min<int64_t>(c.n, (int64_t)k * per);
    hi64 = std::min<int64_t>(c.n, lo64 + per);
  } else {
    plaidhip_shard_bounds(c.n, ndev, k, &lo64, &hi64);
  }
  *lo = (int32_t)lo64;
  *nloc = (int32_t)(hi64 - lo64);
}

inline int64_t even_ld(int32_t g) { return (int64_t)g + (g & 1); }

// device buffers that live in the context between calls (ctx_buffer); same interface as DevBuf
struct CtxBuf {
  plaidhip_ctx* ctx;
  int slot;
  void* p = nullptr;
  int alloc(size_t bytes) { return ctx_buffer(ctx, slot, bytes, &p); }
  template <typename T> T* as() { return static_cast<T*>(p); }
};

// one device's part of a sharded call.  Returns a status; `sh` carries the cross-shard scalars.
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

// {sum, count} of the non-NaN entries of v in exactly the order of sum_kernel (kernels_norm.hip): 1,024 strided partial
// sums, then a halving tree -- IEEE additions in the same order give the same bits on the host
double mean_like_device_sum(const double* v, int64_t count) {
  std::vector<double> s(1024, 0.0), cnt(1024, 0.0);
  for (int t = 0; t < 1024; ++t)
    for (int64_t i = t; i < count; i += 1024) {
      const double x = v[i];
      if (x == x) { s[(size_t)t] += x; cnt[(size_t)t] += 1.0; }
    }
  for (int h = 512; h >= 1; h >>= 1)
    for (int t = 0; t < h; ++t) { s[(size_t)t] += s[(size_t)(t + h)]; cnt[(size_t)t] += cnt[(size_t)(t + h)]; }
  return s[0] / cnt[0];
}

// What every worker below runs on: shard k of ndev, its columns, its status.  Every `step` is skipped once this shard or
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
int upload_pattern(plaidhip_ctx* ctx, const int32_t* Gp, const int32_t* Gi, int32_t m, DevBuf& dGp, DevBuf& dGi) {
  const size_t z = (size_t)Gp[m];
  PH_TRY(dGp.alloc((size_t)(m + 1) * 4));
  PH_TRY(dGi.alloc(std::max<size_t>(z, 1) * 4));
  PH_HIP(hipMemcpyAsync(dGp.p, Gp, (size_t)(m + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  if (z > 0) PH_HIP(hipMemcpyAsync(dGi.p, Gi, z * 4, hipMemcpyHostToDevice, ctx->stream));
  return PLAIDHIP_OK;
}

// this shard's {min, max} (and "a NaN among them") into the range over all shards, in the comparisons of
// minmax_final_kernel; a shard without columns brings {inf, -inf, false}, which change nothing
void merge_range(Shard& s, double mn, double mx, bool any_nan = false) {
  std::lock_guard<std::mutex> lk(s.sh.mu);
  if (s.rc != PLAIDHIP_OK) return;
  s.sh.xmin = mn < s.sh.xmin ? mn : s.sh.xmin;
  s.sh.xmax = mx > s.sh.xmax ? mx : s.sh.xmax;
  s.sh.es_nan = s.sh.es_nan || any_nan;
}

// normalize_medians (R/plaid.R:554-575) up to mean(medx), for the m x nloc scores dS whose crossprod classified them
// (d_flags): min(x) == 0 over ALL shards decides ignore.zero (:556-557), every shard takes its columns' medians (left in
// d_med), and mean(medx, na.rm = TRUE) (:572) is taken over ALL columns in the summation order of the device's sum kernel
// (launch_sum) -- it does not depend on how the columns were sharded, so every sharding, one device included, normalises
// with the same bits.  Two rendezvous.  The caller shifts the columns, or keeps the shift for later.
double medians_and_their_mean(Shard& s, double* dS, const uint32_t* d_flags, double* d_med) {
  const int32_t m = s.c.m, nloc = s.nloc;
  plaidhip_ctx* ctx = s.ctx;
  uint32_t fl[4] = {0, 0, 0, 0};
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    PH_HIP(hipMemcpyAsync(fl, d_flags, 16, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    return PLAIDHIP_OK;
  });
  {
    std::lock_guard<std::mutex> lk(s.sh.mu);
    for (int q = 0; q < 4; ++q) s.sh.flags[q] |= fl[q];
  }
  s.sh.rv.arrive_and_wait();
  const int ignore_zero = (s.sh.flags[1] != 0 && s.sh.flags[0] == 0) ? 1 : 0;
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    PH_TRY(launch_col_medians_resume(ctx, dS, m, m, nloc, ignore_zero, nullptr, d_med));
    PH_HIP(hipMemcpyAsync(s.sh.med_all.data() + s.lo, d_med, (size_t)nloc * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    return PLAIDHIP_OK;
  });
  s.sh.rv.arrive_and_wait();
  return s.live() ? mean_like_device_sum(s.sh.med_all.data(), s.c.n) : 0.0;
}

// Chained, ordered reduction over the samples of the [nblk][groups][rows] block partials in ws: in round r only shard r
// works, continuing shard r - 1's running sums (`run`, [groups][rows], on the host) block by block -- the additions of the
// one-device call in their order.  ndev rendezvous.  d_seed, d_run: groups x rows doubles each.
void chain_block_sums(Shard& s, std::vector<double>& run, const double* ws, int32_t rows, int groups, double* d_seed,
                      double* d_run) {
  plaidhip_ctx* ctx = s.ctx;
  const size_t bytes = (size_t)rows * groups * 8;
  for (int r = 0; r < s.ndev; ++r) {
    if (r == s.k)
      s.step([&]() -> int {
        if (s.nloc == 0) return PLAIDHIP_OK;
        PH_HIP(hipMemcpyAsync(d_seed, run.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        for (int q = 0; q < groups; ++q)
          PH_TRY(launch_reduce_blocks_seeded(ctx, ws + (size_t)q * rows, rows, s.nloc, d_seed + (size_t)q * rows,
                                             d_run + (size_t)q * rows));
        PH_HIP(hipMemcpyAsync(run.data(), d_run, bytes, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));
        return PLAIDHIP_OK;
      });
    s.sh.rv.arrive_and_wait();
  }
}

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

// one device's part of replaid.ucell / aucell / scse / gsva (kUcell ... kGsva; one shard: plaidhip_ucell ... plaidhip_gsva_csc)
// and of replaid.gsva.exact (kGsvaExact).  The quantities that couple the samples are combined on the host between the
// phases: max(rX) (R/plaid.R:278, 306), the min / max behind removeLog2 = NULL (:160-161), the per-gene mean and sd of the
// z row transform (:341-343) and the medians' flags and mean(medx) (:554-575).
int scorer_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  if (c.method == kSsgseaExact) return ssgsea_exact_worker(ctx, c, ndev, k, sh);
  if (c.method == kSingExact) return sing_exact_worker(ctx, c, ndev, k, sh);
  if (c.method == kUcellExact || c.method == kAucellExact) return truncated_exact_worker(ctx, c, ndev, k, sh);
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
          sh.row_sum[(size_t)k] = std::move(sums);   // (each shard writes its own slot)
          sh.row_len[(size_t)k] = std::move(len);
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
    chain_block_sums(s, sh.chain_sum, dscratch.as<double>(), g, 1, d_seed, d_run);
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      host_mean.resize((size_t)g);
      // A true division, as rowMeans and the dgCMatrix branch below divide: sum * fl(1 / n) misses the mean of a constant
      // gene for some n (1.25 at n = 105), whose z then is -2e-8 instead of 0 and whose signed rank -1 instead of 0
      for (int32_t i = 0; i < g; ++i) host_mean[(size_t)i] = sh.chain_sum[(size_t)i] / (double)n;
      PH_HIP(hipMemcpyAsync(d_mean, host_mean.data(), (size_t)g * 8, hipMemcpyHostToDevice, ctx->stream));
      return launch_row_group_partials(ctx, dX.as<double>(), ld, g, nloc, dy.as<int32_t>(), d_mean, dscratch.as<double>());
    });
    chain_block_sums(s, sh.chain_ssd, dscratch.as<double>(), g, 1, d_seed, d_run);
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      PH_HIP(hipMemcpyAsync(d_ssd, sh.chain_ssd.data(), (size_t)g * 8, hipMemcpyHostToDevice, ctx->stream));
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
          if (!sh.row_sum[(size_t)q].empty()) { sum += sh.row_sum[(size_t)q][(size_t)i]; z += sh.row_len[(size_t)q][(size_t)i]; }
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
      sh.row_ssd[(size_t)k] = std::move(q);
      return PLAIDHIP_OK;
    });
    sh.rv.arrive_and_wait();
    if (s.live()) {
      for (int32_t i = 0; i < g; ++i) {
        double q = 0.0;
        for (int r = 0; r < ndev; ++r)
          if (!sh.row_ssd[(size_t)r].empty()) q += sh.row_ssd[(size_t)r][(size_t)i];
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

// the group means of [2][rows] chained sums: reduce_blocks_kernel's scale (a product with 1 / n_k, NaN for an empty group)
void scaled_group_means(const std::vector<double>& sums, int32_t rows, int64_t n0, int64_t n1, double* mean) {
  const double s0 = n0 > 0 ? 1.0 / (double)n0 : std::numeric_limits<double>::quiet_NaN();
  const double s1 = n1 > 0 ? 1.0 / (double)n1 : std::numeric_limits<double>::quiet_NaN();
  for (int32_t i = 0; i < rows; ++i) {
    mean[i] = sums[(size_t)i] * s0;
    mean[(size_t)rows + i] = sums[(size_t)rows + i] * s1;
  }
}

// one device's part of a sharded plaid.test (kPlaidTest, R/plaid.R:392-474; one shard: plaidhip_plaid_test / _csc), with what
// couples the samples combined on the host in between -- everything plaid.test reduces is a row sum over the samples,
// so only O(genes + sets) numbers cross between the shards and the scores never leave their device.
//   logFC: dense X chains the two group sums of X from shard to shard (the one-device block order); a dgCMatrix sums
//     each shard's stored values per group, the host adds the shards.  Shard 0 alone then takes F = [fc, fc^2] and
//     T = Gt F.
//   scores ("lm"): gsetX's columns uploaded, or plaid(X, G)'s sharded crossprod and medians (shard_worker), stopped
//     before the shift: the shard keeps the raw S, its medians and mean(medx).
//   Welch moments: the group sums of the score rows, shifted on load (launch_row_group_shifted_partials), chained; then,
//     from the global means, the sums of squared deviations, chained.  plaidhip_plaid_test_finish runs in run_call.
int plaid_test_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc;
  const int32_t g = c.g, m = c.m, n = c.n;
  const bool sparse = c.Xp != nullptr;
  const bool lm = (c.tests & 4) != 0;
  const bool scores = lm && c.gsetX == nullptr;   // plaid(X, G) computed here (R/plaid.R:424-427)
  const int64_t ldg = even_ld(g);
  const int64_t wide = std::max<int64_t>(g, m);
  const size_t nl = (size_t)std::max(nloc, 1);
  plaidhip_geneset* gs = nullptr;
  CtxBuf dX{ctx, 0}, dXp{ctx, 1}, dXi{ctx, 2}, dS{ctx, 4}, dsmall{ctx, 5};
  DevBuf dy, dws, drows, drp, dRj, dRx, dF, dT;
  uint32_t* d_flags = nullptr;
  double *d_med = nullptr, *d_seed = nullptr, *d_run = nullptr, *d_mean = nullptr;
  const int64_t zx = s.zx;
  std::vector<int32_t> ploc;
  // host sources of asynchronous uploads: they live until the worker's last synchronisation
  std::vector<double> x_mean, s_mean;

  // ---- upload; X's group sums of this shard; plaid()'s crossprod of dense X panel by panel --------------------------------
  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    if (k == 0 || scores) PH_TRY(acquire_geneset(ctx, g, m, c.Gp, c.Gi, &gs));
    PH_TRY(dsmall.alloc(64 + nl * 8));
    d_flags = dsmall.as<uint32_t>();
    d_med = reinterpret_cast<double*>(dsmall.as<char>() + 64);
    PH_HIP(hipMemsetAsync(dsmall.p, 0, 64, ctx->stream));
    PH_TRY(drows.alloc((size_t)wide * 6 * 8));   // [seed | running sums | means], [2][max(g, m)] each
    d_seed = drows.as<double>();
    d_run = d_seed + 2 * wide;
    d_mean = d_run + 2 * wide;
    if (lm) PH_TRY(dS.alloc((size_t)m * nl * 8));
    if (nloc == 0) return PLAIDHIP_OK;
    PH_TRY(dy.alloc((size_t)nloc * 4));
    PH_HIP(hipMemcpyAsync(dy.p, c.y + lo, (size_t)nloc * 4, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dws.alloc((size_t)std::max(sparse ? 0 : row_group_ws_doubles(g, nloc), lm ? row_group_ws_doubles(m, nloc) : 0) * 8));
    if (!sparse) {
      PH_TRY(dX.alloc((size_t)ldg * nloc * 8));
      auto on_panel = [&](int64_t c0, int64_t c1) -> int {   // (shard_worker's plaid())
        return launch_spmm_dense_f64(ctx, gs, dX.as<double>() + c0 * ldg, ldg, (int32_t)(c1 - c0), PLAIDHIP_STAT_MEAN, 1.0,
                                     nullptr, 0.0, dS.as<double>() + c0 * m, m, d_flags);
      };
      PH_TRY(upload_pipelined(ctx, dX.as<char>(), (size_t)ldg * 8, reinterpret_cast<const char*>(c.X + (int64_t)lo * g),
                              (size_t)g * 8, nloc, scores ? std::function<int(int64_t, int64_t)>(on_panel) : nullptr));
      return launch_row_group_partials(ctx, dX.as<double>(), ldg, g, nloc, dy.as<int32_t>(), nullptr, dws.as<double>());
    }
    int32_t max_nnz = 0;
    PH_TRY(upload_csc_shard(s, ploc, dXp, dXi, dX, &max_nnz));
    const size_t zb = (size_t)std::max<int64_t>(zx, 1);
    // the shard's row view, with its column indices (they look up y), and the unscaled group sums of its stored values
    PH_TRY(drp.alloc((size_t)(g + 2) * 4));
    PH_TRY(dRj.alloc(zb * 4));
    PH_TRY(dRx.alloc(zb * 8));
    PH_TRY(launch_csc_to_csr(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), dX.as<double>(), g, nloc, drp.as<int32_t>(),
                             dRj.as<int32_t>(), dRx.as<double>(), nullptr, drp.as<int32_t>() + g + 1));
    int32_t max_row = 0;
    PH_HIP(hipMemcpyAsync(&max_row, drp.as<int32_t>() + g + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    PH_TRY(launch_csr_row_group_stored_sums(ctx, drp.as<int32_t>(), dRj.as<int32_t>(), dRx.as<double>(), g, max_row,
                                            dy.as<int32_t>(), d_run));
    std::vector<double> sums((size_t)g * 2);
    PH_HIP(hipMemcpyAsync(sums.data(), d_run, (size_t)g * 2 * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    sh.row_sum[(size_t)k] = std::move(sums);   // (each shard writes its own slot)
    return PLAIDHIP_OK;
  });

  // ---- logFC = rowMeans(X[, y == 1]) - rowMeans(X[, y == 0]) (R/plaid.R:407-409); shard 0: Gt fc, Gt fc^2 (:478-479) -----
  if (!sparse) chain_block_sums(s, sh.chain_x, dws.as<double>(), g, 2, d_seed, d_run);
  else sh.rv.arrive_and_wait();   // every shard's stored-value sums are in sh.row_sum
  s.step([&]() -> int {
    if (k != 0) return PLAIDHIP_OK;
    x_mean.resize((size_t)g * 2);
    if (!sparse) {
      scaled_group_means(sh.chain_x, g, c.n0, c.n1, x_mean.data());
    } else {   // the shards added in shard order, then csr_row_moments_kernel's true division (0 / 0 = NaN, empty group)
      for (int32_t i = 0; i < g; ++i) {
        double s0 = 0.0, s1 = 0.0;
        for (int q = 0; q < ndev; ++q)
          if (!sh.row_sum[(size_t)q].empty()) { s0 += sh.row_sum[(size_t)q][(size_t)i]; s1 += sh.row_sum[(size_t)q][(size_t)g + i]; }
        x_mean[(size_t)i] = s0 / (double)c.n0;
        x_mean[(size_t)g + i] = s1 / (double)c.n1;
      }
    }
    PH_TRY(dF.alloc((size_t)ldg * 2 * 8));
    PH_TRY(dT.alloc((size_t)m * 2 * 8));
    PH_HIP(hipMemcpyAsync(d_mean, x_mean.data(), (size_t)g * 2 * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemsetAsync(dF.p, 0, (size_t)ldg * 2 * 8, ctx->stream));
    PH_TRY(launch_fold_change(ctx, d_mean, g, ldg, dF.as<double>()));
    PH_TRY(launch_spmm_dense_f64(ctx, gs, dF.as<double>(), ldg, 2, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0, dT.as<double>(), m,
                                 nullptr));
    PH_HIP(hipMemcpyAsync(sh.pt_T.data(), dT.p, (size_t)m * 2 * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(sh.pt_F.data(), dF.p, (size_t)ldg * 2 * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    return PLAIDHIP_OK;
  });

  // ---- the scores: gsetX's columns, or plaid(X, G)'s crossprod of a dgCMatrix (dense X: done panel by panel above) ---------
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

  // ---- normalize_medians (R/plaid.R:554-575) up to mean(medx): the shift is applied on load below ----------------------------
  const double add = scores ? medians_and_their_mean(s, dS.as<double>(), d_flags, d_med) : 0.0;

  // ---- Welch moments of the score rows (Rfast::ttests(t(gsetX), ina = y + 1), :429) --------------------------------------
  if (lm) {
    const double* med = scores ? d_med : nullptr;
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      return launch_row_group_shifted_partials(ctx, dS.as<double>(), m, m, nloc, dy.as<int32_t>(), med, add, nullptr,
                                               dws.as<double>());
    });
    chain_block_sums(s, sh.chain_s, dws.as<double>(), m, 2, d_seed, d_run);
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      s_mean.resize((size_t)m * 2);
      scaled_group_means(sh.chain_s, m, c.n0, c.n1, s_mean.data());
      PH_HIP(hipMemcpyAsync(d_mean, s_mean.data(), (size_t)m * 2 * 8, hipMemcpyHostToDevice, ctx->stream));
      return launch_row_group_shifted_partials(ctx, dS.as<double>(), m, m, nloc, dy.as<int32_t>(), med, add, d_mean,
                                               dws.as<double>());
    });
    chain_block_sums(s, sh.chain_q, dws.as<double>(), m, 2, d_seed, d_run);
  }

  return s.finish();
}

// chain_block_sums for the [nblk][C][2][rows] partials of launch_row_contrast_partials: every contrast and group at once
// (launch_reduce_blocks_flat); run, d_seed, d_run: [C][2][rows].  ndev rendezvous.
void chain_contrast_sums(Shard& s, std::vector<double>& run, const double* ws, int32_t rows, int32_t C, double* d_seed,
                         double* d_run) {
  plaidhip_ctx* ctx = s.ctx;
  const int64_t len = (int64_t)C * 2 * rows;
  for (int r = 0; r < s.ndev; ++r) {
    if (r == s.k)
      s.step([&]() -> int {
        if (s.nloc == 0) return PLAIDHIP_OK;
        PH_HIP(hipMemcpyAsync(d_seed, run.data(), (size_t)len * 8, hipMemcpyHostToDevice, ctx->stream));
        PH_TRY(launch_reduce_blocks_flat(ctx, ws, len, s.nloc, d_seed, d_run));
        PH_HIP(hipMemcpyAsync(run.data(), d_run, (size_t)len * 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));
        return PLAIDHIP_OK;
      });
    s.sh.rv.arrive_and_wait();
  }
}

// scaled_group_means for every contrast of [C][2][rows] chained sums, each with its own group sizes
void scaled_contrast_means(const Call& c, const std::vector<double>& sums, int32_t rows, double* mean) {
  for (int32_t j = 0; j < c.ncontrast; ++j) {
    const int64_t n0 = c.cn0[(size_t)j], n1 = c.cn1[(size_t)j];
    const double s0 = n0 > 0 ? 1.0 / (double)n0 : std::numeric_limits<double>::quiet_NaN();
    const double s1 = n1 > 0 ? 1.0 / (double)n1 : std::numeric_limits<double>::quiet_NaN();
    const size_t o = (size_t)j * 2 * rows;
    for (int32_t i = 0; i < rows; ++i) {
      mean[o + i] = sums[o + i] * s0;
      mean[o + rows + i] = sums[o + rows + i] * s1;
    }
  }
}

// one device's part of plaid.test.contrasts (kPlaidTestContrasts; include/plaidhip.h: plaidhip_plaid_test_contrasts):
// plaid_test_worker with C label columns.  The same phases and rendezvous; what was [2][rows] is [C][2][rows], the row
// moments come from kernels_contrasts.hip (every read of X and of S shared by a tile of contrasts), plaid(X, G) and the
// medians run once, and shard 0 takes Gt [fc_j, fc_j^2] per contrast with the crossprod call of plaid_test_worker.  A
// contrast adds what plaid_test_worker adds for its label column, in its order.
int plaid_test_contrasts_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t lo = s.lo, nloc = s.nloc;
  const int32_t g = c.g, m = c.m, n = c.n, C = c.ncontrast;
  const bool sparse = c.Xp != nullptr;
  const bool lm = (c.tests & 4) != 0;
  const bool scores = lm && c.gsetX == nullptr;   // plaid(X, G) computed here (R/plaid.R:424-427), once
  const int64_t ldg = even_ld(g);
  const int64_t wide = std::max<int64_t>(g, m);
  const size_t nl = (size_t)std::max(nloc, 1);
  plaidhip_geneset* gs = nullptr;
  CtxBuf dX{ctx, 0}, dXp{ctx, 1}, dXi{ctx, 2}, dS{ctx, 4}, dsmall{ctx, 5};
  DevBuf dY, dmask, dws, drows, drp, dRj, dRx, dF, dT;
  uint32_t* d_flags = nullptr;
  double *d_med = nullptr, *d_seed = nullptr, *d_run = nullptr, *d_mean = nullptr;
  const int64_t zx = s.zx;
  std::vector<int32_t> ploc;
  // host sources of asynchronous uploads: they live until the worker's last synchronisation
  std::vector<double> x_mean, s_mean;

  // ---- upload; the labels and their masks; X's group sums of this shard; plaid()'s crossprod of dense X ---------------------
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
    PH_TRY(dY.alloc((size_t)nloc * C * 4));   // the shard's rows of Y, nloc x C
    for (int32_t j = 0; j < C; ++j)
      PH_HIP(hipMemcpyAsync(dY.as<int32_t>() + (size_t)j * nloc, c.y + (size_t)j * n + lo, (size_t)nloc * 4,
                            hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(dmask.alloc((size_t)contrast_mask_bytes(nloc, C)));
    PH_TRY(launch_contrast_masks(ctx, dY.as<int32_t>(), nloc, nloc, C, dmask.p));
    PH_TRY(dws.alloc((size_t)std::max<int64_t>(
        {sparse ? 0 : row_contrast_ws_doubles(g, nloc, C), lm ? row_contrast_ws_doubles(m, nloc, C) : 0, 1}) * 8));
    if (!sparse) {
      PH_TRY(dX.alloc((size_t)ldg * nloc * 8));
      auto on_panel = [&](int64_t c0, int64_t c1) -> int {   // (shard_worker's plaid())
        return launch_spmm_dense_f64(ctx, gs, dX.as<double>() + c0 * ldg, ldg, (int32_t)(c1 - c0), PLAIDHIP_STAT_MEAN, 1.0,
                                     nullptr, 0.0, dS.as<double>() + c0 * m, m, d_flags);
      };
      PH_TRY(upload_pipelined(ctx, dX.as<char>(), (size_t)ldg * 8, reinterpret_cast<const char*>(c.X + (int64_t)lo * g),
                              (size_t)g * 8, nloc, scores ? std::function<int(int64_t, int64_t)>(on_panel) : nullptr));
      return launch_row_contrast_partials(ctx, dX.as<double>(), ldg, g, nloc, dmask.p, C, nullptr, 0.0, nullptr,
                                          dws.as<double>());
    }
    int32_t max_nnz = 0;
    PH_TRY(upload_csc_shard(s, ploc, dXp, dXi, dX, &max_nnz));
    const size_t zb = (size_t)std::max<int64_t>(zx, 1);
    // the shard's row view, built once; the unscaled group sums of its stored values, per contrast
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
                                              dY.as<int32_t>() + (size_t)j * nloc, d_run + (size_t)j * 2 * g));
    std::vector<double> sums((size_t)g * 2 * C);
    PH_HIP(hipMemcpyAsync(sums.data(), d_run, sums.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    sh.row_sum[(size_t)k] = std::move(sums);   // (each shard writes its own slot)
    return PLAIDHIP_OK;
  });

  // ---- logFC_j (R/plaid.R:407-409 on the contrast's samples); shard 0: Gt fc_j, Gt fc_j^2 (:478-479) ------------------------
  if (!sparse) chain_contrast_sums(s, sh.chain_x, dws.as<double>(), g, C, d_seed, d_run);
  else sh.rv.arrive_and_wait();   // every shard's stored-value sums are in sh.row_sum
  s.step([&]() -> int {
    if (k != 0) return PLAIDHIP_OK;
    x_mean.resize((size_t)g * 2 * C);
    if (!sparse) {
      scaled_contrast_means(c, sh.chain_x, g, x_mean.data());
    } else {   // the shards added in shard order, then csr_row_moments_kernel's true division (0 / 0 = NaN, empty group)
      for (int32_t j = 0; j < C; ++j) {
        const size_t o = (size_t)j * 2 * g;
        for (int32_t i = 0; i < g; ++i) {
          double s0 = 0.0, s1 = 0.0;
          for (int q = 0; q < ndev; ++q)
            if (!sh.row_sum[(size_t)q].empty()) { s0 += sh.row_sum[(size_t)q][o + i]; s1 += sh.row_sum[(size_t)q][o + g + i]; }
          x_mean[o + i] = s0 / (double)c.cn0[(size_t)j];
          x_mean[o + g + i] = s1 / (double)c.cn1[(size_t)j];
        }
      }
    }
    PH_TRY(dF.alloc((size_t)ldg * 2 * C * 8));
    PH_TRY(dT.alloc((size_t)m * 2 * C * 8));
    PH_HIP(hipMemcpyAsync(d_mean, x_mean.data(), x_mean.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemsetAsync(dF.p, 0, (size_t)ldg * 2 * C * 8, ctx->stream));
    PH_TRY(launch_fold_change_contrasts(ctx, d_mean, g, C, ldg, dF.as<double>()));
    for (int32_t j = 0; j < C; ++j)   // two columns per call: the crossprod call of plaid_test_worker, so its bits
      PH_TRY(launch_spmm_dense_f64(ctx, gs, dF.as<double>() + (size_t)j * 2 * ldg, ldg, 2, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0,
                                   dT.as<double>() + (size_t)j * 2 * m, m, nullptr));
    PH_HIP(hipMemcpyAsync(sh.pt_T.data(), dT.p, (size_t)m * 2 * C * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(sh.pt_F.data(), dF.p, (size_t)ldg * 2 * C * 8, hipMemcpyDeviceToHost, ctx->stream));
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
      return launch_row_contrast_partials(ctx, dS.as<double>(), m, m, nloc, dmask.p, C, med, add, nullptr, dws.as<double>());
    });
    chain_contrast_sums(s, sh.chain_s, dws.as<double>(), m, C, d_seed, d_run);
    s.step([&]() -> int {
      if (nloc == 0) return PLAIDHIP_OK;
      s_mean.resize((size_t)m * 2 * C);
      scaled_contrast_means(c, sh.chain_s, m, s_mean.data());
      PH_HIP(hipMemcpyAsync(d_mean, s_mean.data(), s_mean.size() * 8, hipMemcpyHostToDevice, ctx->stream));
      return launch_row_contrast_partials(ctx, dS.as<double>(), m, m, nloc, dmask.p, C, med, add, d_mean, dws.as<double>());
    });
    chain_contrast_sums(s, sh.chain_q, dws.as<double>(), m, C, d_seed, d_run);
  }

  return s.finish();
}

// ---- plaid.gsea's multilevel chains (kernels_gsea_ml.hip; include/plaidhip.h: plaidhip_gsea_multilevel) -------------------------
// what the rulers leave: per set (in the rulers' set order) the read-off stage, count and status; per ruler its stages, end
// status and the trace of counts and levels ([ruler][PLAIDHIP_GSEA_ML_MAX_STAGES])
struct GseaMlResult {
  std::vector<int32_t> lstar, cnt, est, s_trace, nstages, end;
  std::vector<double> m_trace;
};

constexpr size_t kGseaMlBatchBytes = (size_t)1 << 30;   // ruler state one batch of rulers keeps on the device, at most

// Runs `rulers` (their set0 / nset index `gamma`) to their ends, batch by batch; a host loop advances a batch one stage per
// launch pair and reads one counter back, so no launch outlasts one stage.  h_out (nullable, one ruler): every stage's scores.
int gsea_ml_run(plaidhip_ctx* ctx, int weighted, int score_type, const double* dWpos, int32_t g,
                const std::vector<GseaMlRuler>& rulers, const std::vector<double>& gamma, int32_t n, int32_t sweeps, double eps,
                uint64_t seed, double* h_out, GseaMlResult& res) {
  constexpr int32_t S = PLAIDHIP_GSEA_ML_MAX_STAGES;
  const size_t nr_all = rulers.size(), nset_all = gamma.size();
  res.lstar.assign(nset_all, -1);
  res.cnt.assign(nset_all, 0);
  res.est.assign(nset_all, 0);
  res.s_trace.assign(nr_all * S, 0);
  res.m_trace.assign(nr_all * S, 0.0);
  res.nstages.assign(nr_all, 0);
  res.end.assign(nr_all, 0);
  if (nr_all == 0) return PLAIDHIP_OK;
  const int32_t nwg = gsea_ml_map_words(g);
  const size_t per_ruler = (size_t)n * nwg * 8 + (size_t)n * 8 + (size_t)S * 12 + sizeof(GseaMlState) + sizeof(GseaMlRuler);
  const size_t batch = std::max<size_t>(1, std::min<size_t>(nr_all, kGseaMlBatchBytes / per_ruler));
  DevBuf dru, dst, dmaps, dH, dstr, dmtr, dhtr, dgam, dls, dcn, des, dcount;
  PH_TRY(dru.alloc(batch * sizeof(GseaMlRuler)));
  PH_TRY(dst.alloc(batch * sizeof(GseaMlState)));
  PH_TRY(dmaps.alloc(batch * n * nwg * 8));
  PH_TRY(dH.alloc(batch * n * 8));
  PH_TRY(dstr.alloc(batch * S * 4));
  PH_TRY(dmtr.alloc(batch * S * 8));
  if (h_out != nullptr) PH_TRY(dhtr.alloc(batch * S * n * 8));
  PH_TRY(dcount.alloc(4));
  size_t max_nq = 1;   // the sets of the largest batch
  for (size_t r0 = 0; r0 < nr_all; r0 += batch) {
    const size_t r1 = std::min(nr_all, r0 + batch);
    max_nq = std::max(max_nq, (size_t)(rulers[r1 - 1].set0 + rulers[r1 - 1].nset - rulers[r0].set0));
  }
  PH_TRY(dgam.alloc(max_nq * 8));
  PH_TRY(dls.alloc(max_nq * 4));
  PH_TRY(dcn.alloc(max_nq * 4));
  PH_TRY(des.alloc(max_nq * 4));
  std::vector<GseaMlRuler> hr;
  std::vector<GseaMlState> hs;
  for (size_t r0 = 0; r0 < nr_all; r0 += batch) {
    const size_t r1 = std::min(nr_all, r0 + batch);
    const int32_t nr = (int32_t)(r1 - r0);
    const int32_t q0 = rulers[r0].set0, q1 = rulers[r1 - 1].set0 + rulers[r1 - 1].nset, nq = q1 - q0;
    hr.assign(rulers.begin() + (ptrdiff_t)r0, rulers.begin() + (ptrdiff_t)r1);
    for (GseaMlRuler& r : hr) r.set0 -= q0;
    GseaMlState fresh{};
    fresh.P = 1.0;
    hs.assign((size_t)nr, fresh);
    PH_HIP(hipMemcpyAsync(dru.p, hr.data(), (size_t)nr * sizeof(GseaMlRuler), hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemcpyAsync(dst.p, hs.data(), (size_t)nr * sizeof(GseaMlState), hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemcpyAsync(dgam.p, gamma.data() + q0, (size_t)nq * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemsetAsync(dls.p, 0xff, (size_t)nq * 4, ctx->stream));
    PH_HIP(hipMemsetAsync(dcn.p, 0, (size_t)nq * 4, ctx->stream));
    PH_HIP(hipMemsetAsync(des.p, 0, (size_t)nq * 4, ctx->stream));
    PH_HIP(hipMemsetAsync(dstr.p, 0, (size_t)nr * S * 4, ctx->stream));
    PH_HIP(hipMemsetAsync(dmtr.p, 0, (size_t)nr * S * 8, ctx->stream));
    if (h_out != nullptr) PH_HIP(hipMemsetAsync(dhtr.p, 0, (size_t)nr * S * n * 8, ctx->stream));
    PH_TRY(launch_gsea_ml_init(ctx, weighted, score_type, dru.as<GseaMlRuler>(), nr, n, g, dWpos, seed,
                               dmaps.as<unsigned long long>(), dH.as<double>()));
    for (int32_t stage = 0; stage < S; ++stage) {
      uint32_t unfinished = 0u;
      PH_HIP(hipMemsetAsync(dcount.p, 0, 4, ctx->stream));
      PH_TRY(launch_gsea_ml_stage(ctx, dru.as<GseaMlRuler>(), dst.as<GseaMlState>(), nr, n, g, eps,
                                  dmaps.as<unsigned long long>(), dH.as<double>(), dstr.as<int32_t>(), dmtr.as<double>(),
                                  h_out != nullptr ? dhtr.as<double>() : nullptr, dgam.as<double>(), dls.as<int32_t>(),
                                  dcn.as<int32_t>(), des.as<int32_t>(), dcount.as<uint32_t>()));
      PH_HIP(hipMemcpyAsync(&unfinished, dcount.p, 4, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
      if (unfinished == 0u) break;
      PH_TRY(launch_gsea_ml_mutate(ctx, weighted, score_type, dru.as<GseaMlRuler>(), dst.as<GseaMlState>(), nr, n, g, dWpos, seed,
                                   sweeps, dmaps.as<unsigned long long>(), dH.as<double>()));
    }
    PH_HIP(hipMemcpyAsync(hs.data(), dst.p, (size_t)nr * sizeof(GseaMlState), hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(res.s_trace.data() + r0 * S, dstr.p, (size_t)nr * S * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(res.m_trace.data() + r0 * S, dmtr.p, (size_t)nr * S * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(res.lstar.data() + q0, dls.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(res.cnt.data() + q0, dcn.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipMemcpyAsync(res.est.data() + q0, des.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (h_out != nullptr) PH_HIP(hipMemcpyAsync(h_out, dhtr.p, (size_t)S * n * 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    for (int32_t r = 0; r < nr; ++r) {
      PH_REQUIRE(hs[(size_t)r].ended != 0, "gsea_multilevel: a ruler did not end within %d stages", S);
      res.nstages[r0 + (size_t)r] = hs[(size_t)r].stage;
      res.end[r0 + (size_t)r] = hs[(size_t)r].status;
    }
  }
  return PLAIDHIP_OK;
}

// qhat and log2err of a set read off at stage lstar with count cnt, from its ruler's counts (include/plaidhip.h: the order of
// the operations is part of the pinned form)
void gsea_ml_readoff(const int32_t* s_trace, int32_t n, int32_t lstar, int32_t cnt, double* qhat, double* log2err) {
  double P = 1.0, sum = 0.0;
  for (int32_t j = 0; j < lstar; ++j) {
    const int32_t s = s_trace[j];
    P = P * ((double)s / (double)n);
    sum += (double)(n - s) / ((double)n * (double)s);
  }
  const int32_t c1 = cnt > 1 ? cnt : 1;
  *qhat = P * ((double)c1 / (double)n);
  sum += (double)(n - c1) / ((double)n * (double)c1);
  *log2err = std::sqrt(sum) / 0.6931471805599453;   // ln 2
}

// the observed placement and walk-order weights of nl lists already on the device (dstat, dw: g x nl)
int gsea_observed_operands(plaidhip_ctx* ctx, const double* dstat, const double* dw, const uint32_t* dnan, int32_t g, int32_t nl,
                           double* dR, double* dY, double* dQ, int32_t* dpos, double* dWpos) {
  const size_t col = (size_t)g * nl;
  PH_HIP(hipMemsetAsync(dWpos, 0, col * 8, ctx->stream));
  PH_HIP(hipMemsetAsync(dpos, 0, col * 4, ctx->stream));
  PH_TRY(launch_colranks_dense_f64(ctx, dstat, g, g, nl, PLAIDHIP_TIES_MIN, 0, 1.0, dR, g, nullptr));
  PH_TRY(launch_last_ranks(ctx, dense_cols(g, nl, g), dR, dY, dQ));
  return launch_gsea_operands(ctx, dQ, dw, g, dnan, g, nl, dpos, dWpos);
}

// plaidhip_gsea_ruler: one ruler of one list to the caller's target, and its trace
int gsea_ruler_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    const int32_t g = c.g;
    DevBuf dstat, dw, dR, dY, dQ, dWpos, dpos, dnan;
    for (DevBuf* b : {&dstat, &dw, &dR, &dY, &dQ, &dWpos}) PH_TRY(b->alloc((size_t)g * 8));
    PH_TRY(dpos.alloc((size_t)g * 4));
    PH_TRY(dnan.alloc(4));
    PH_HIP(hipMemcpyAsync(dstat.p, c.X, (size_t)g * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemcpyAsync(dw.p, c.weight, (size_t)g * 8, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipMemsetAsync(dnan.p, 0, 4, ctx->stream));
    PH_TRY(gsea_observed_operands(ctx, dstat.as<double>(), dw.as<double>(), dnan.as<uint32_t>(), g, 1, dR.as<double>(),
                                  dY.as<double>(), dQ.as<double>(), dpos.as<int32_t>(), dWpos.as<double>()));
    const std::vector<GseaMlRuler> rulers(1, GseaMlRuler{0, c.ml_l, c.ml_side, c.ml_k, 0, 1, c.ml_gamma});
    const std::vector<double> gamma(1, c.ml_gamma);
    GseaMlResult res;
    PH_TRY(gsea_ml_run(ctx, c.gsea_weighted, c.score_type, dWpos.as<double>(), g, rulers, gamma, c.ml_sample, c.ml_sweeps,
                       c.ml_eps, c.seed, c.ml_h, res));
    *c.ml_nstages = res.nstages[0];
    *c.ml_end = res.end[0];
    std::copy(res.m_trace.begin(), res.m_trace.end(), c.ml_m);
    std::copy(res.s_trace.begin(), res.s_trace.end(), c.ml_s);
    return PLAIDHIP_OK;
  });
  return s.finish();
}

// the side of a pair's ruler: 0 positive, 1 negative, -1 none (a NaN pair; std with ES == 0)
inline int gsea_ml_side(int score_type, double es) {
  if (es != es) return -1;
  if (score_type == PLAIDHIP_GSEA_POS) return 0;
  if (score_type == PLAIDHIP_GSEA_NEG) return 1;
  return es > 0.0 ? 0 : (es < 0.0 ? 1 : -1);
}

// This shard's rulers of plaid.gsea's multilevel p-values: the ruler list (sorted by list, side and size; the same on every
// shard, from the same observed scores) is shared out in whole rulers, and every set's (qhat, log2err, stage, status) goes
// to sh.gsea_ml[4 (l m + j) ..], which holds NaN for a pair without a ruler.
int gsea_ml_shard(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh, const double* dES, const double* dWpos) {
  const int32_t m = c.m, nl = c.n, n = c.ml_sample;
  std::vector<double> es((size_t)m * nl);
  PH_HIP(hipMemcpyAsync(es.data(), dES, es.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  struct Entry { int32_t l, side, k, j; };
  std::vector<Entry> ent;
  for (int32_t l = 0; l < nl; ++l)
    for (int32_t j = 0; j < m; ++j) {
      const int side = gsea_ml_side(c.score_type, es[(size_t)l * m + j]);
      if (side >= 0) ent.push_back(Entry{l, side, c.Gp[j + 1] - c.Gp[j], j});
    }
  std::stable_sort(ent.begin(), ent.end(), [](const Entry& a, const Entry& b) {
    return a.l != b.l ? a.l < b.l : (a.side != b.side ? a.side < b.side : a.k < b.k);
  });
  std::vector<GseaMlRuler> all;
  for (size_t q = 0; q < ent.size(); ++q) {
    const Entry& e = ent[q];
    const double ga = std::fabs(es[(size_t)e.l * m + e.j]);
    if (all.empty() || all.back().l != e.l || all.back().side != e.side || all.back().k != e.k)
      all.push_back(GseaMlRuler{e.l, e.l, e.side, e.k, (int32_t)q, 0, ga});
    all.back().nset += 1;
    all.back().gmax = std::max(all.back().gmax, ga);
  }
  int64_t lo = 0, hi = 0;
  plaidhip_shard_bounds((int64_t)all.size(), ndev, k, &lo, &hi);
  if (hi <= lo) return PLAIDHIP_OK;
  const int32_t q0 = all[(size_t)lo].set0, q1 = all[(size_t)hi - 1].set0 + all[(size_t)hi - 1].nset;
  std::vector<GseaMlRuler> mine(all.begin() + lo, all.begin() + hi);
  std::vector<double> gamma((size_t)(q1 - q0));
  for (GseaMlRuler& r : mine) r.set0 -= q0;
  for (int32_t q = q0; q < q1; ++q) gamma[(size_t)(q - q0)] = std::fabs(es[(size_t)ent[(size_t)q].l * m + ent[(size_t)q].j]);
  GseaMlResult res;
  PH_TRY(gsea_ml_run(ctx, c.gsea_weighted, c.score_type, dWpos, c.g, mine, gamma, n, c.ml_sweeps, c.ml_eps, c.seed, nullptr, res));
  for (size_t r = 0; r < mine.size(); ++r)
    for (int32_t q = mine[r].set0; q < mine[r].set0 + mine[r].nset; ++q) {
      const Entry& e = ent[(size_t)(q0 + q)];
      PH_REQUIRE(res.lstar[(size_t)q] >= 0, "gsea_multilevel: set %d of list %d was not read off", e.j, e.l);
      double* o = sh.gsea_ml.data() + 4 * ((size_t)e.l * m + e.j);
      gsea_ml_readoff(res.s_trace.data() + r * PLAIDHIP_GSEA_ML_MAX_STAGES, n, res.lstar[(size_t)q], res.cnt[(size_t)q], &o[0], &o[1]);
      o[2] = (double)res.lstar[(size_t)q];
      o[3] = (double)res.est[(size_t)q];
    }
  return PLAIDHIP_OK;
}

// one device's part of plaid.gsea (kGsea, kernels_gsea.hip).  Every shard holds stat, weight and G and forms the observed
// placements and scores itself (the same bits everywhere); the permutation blocks are shared out in whole blocks
// (plaidhip_shard_bounds over the blocks) and walked slab by slab; the block partials meet on the host in block order and
// shard 0 reduces them once, so every sharding has the one-shard bits.  One rendezvous.
int gsea_worker(plaidhip_ctx* ctx, const Call& c, int ndev, int k, Shared& sh) {
  Shard s(ctx, c, ndev, k, sh);
  const int32_t g = c.g, nl = c.n, m = c.m, B = c.nperm;
  const int32_t nblk = (B + PLAIDHIP_GSEA_PERM_BLOCK - 1) / PLAIDHIP_GSEA_PERM_BLOCK;
  int64_t blo = 0, bhi = 0;
  plaidhip_shard_bounds(nblk, ndev, k, &blo, &bhi);
  const int64_t p_lo = blo * PLAIDHIP_GSEA_PERM_BLOCK, p_hi = std::min<int64_t>(B, bhi * PLAIDHIP_GSEA_PERM_BLOCK);
  const size_t col = (size_t)g * nl, blk_doubles = (size_t)nl * 6 * m;
  DevBuf dstat, dw, dR, dY, dQ, dWpos, dpos, dnan, dGp, dGi, dES, dpart, dslabY, dslabR, dP, dbad, dnull, dout, dall, dlen, didx;
  const int32_t slab = gsea_slab_perms(g);

  // ---- upload, the observed placements and scores -------------------------------------------------------------------------
  s.step([&]() -> int {
    PH_HIP(hipSetDevice(ctx->device));
    PH_TRY(dstat.alloc(col * 8));
    PH_TRY(dw.alloc(col * 8));
    PH_TRY(dR.alloc(col * 8));
    PH_TRY(dY.alloc(col * 8));
    PH_TRY(dQ.alloc(col * 8));
    PH_TRY(dWpos.alloc(col * 8));
    PH_TRY(dpos.alloc(col * 4));
    PH_TRY(dnan.alloc((size_t)nl * 4));
    PH_TRY(dES.alloc((size_t)m * nl * 8));
    PH_TRY(upload_pattern(ctx, c.Gp, c.Gi, m, dGp, dGi));
    PH_TRY(upload_pipelined(ctx, dstat.as<char>(), (size_t)g * 8, reinterpret_cast<const char*>(c.X), (size_t)g * 8, nl, nullptr));
    PH_TRY(upload_pipelined(ctx, dw.as<char>(), (size_t)g * 8, reinterpret_cast<const char*>(c.weight), (size_t)g * 8, nl,
                            nullptr));
    PH_HIP(hipMemcpyAsync(dnan.p, c.listnan.data(), (size_t)nl * 4, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(gsea_observed_operands(ctx, dstat.as<double>(), dw.as<double>(), dnan.as<uint32_t>(), g, nl, dR.as<double>(),
                                  dY.as<double>(), dQ.as<double>(), dpos.as<int32_t>(), dWpos.as<double>()));
    return launch_gsea_obs(ctx, c.gsea_weighted, c.score_type, dpos.as<int32_t>(), dWpos.as<double>(), dnan.as<uint32_t>(), g, nl,
                           dGp.as<int32_t>(), dGi.as<int32_t>(), m, dES.as<double>());
  });

  // ---- this shard's blocks of the null, slab by slab ------------------------------------------------------------------------
  s.step([&]() -> int {
    if (ctx->debug_fail_crossprod) { set_error("injected failure in the crossprod phase (test hook)"); return PLAIDHIP_EHIP; }
    if (p_hi <= p_lo) return PLAIDHIP_OK;
    const int32_t smax = (int32_t)std::min<int64_t>(slab, p_hi - p_lo);
    PH_TRY(dpart.alloc((size_t)(bhi - blo) * blk_doubles * 8));
    PH_TRY(dP.alloc((size_t)g * smax * 4));
    PH_TRY(dbad.alloc(8));
    PH_HIP(hipMemsetAsync(dbad.p, 0, 8, ctx->stream));
    if (c.perm == nullptr) {
      PH_TRY(dslabY.alloc((size_t)g * smax * 8));
      PH_TRY(dslabR.alloc((size_t)g * smax * 8));
    }
    if (c.null_out != nullptr) PH_TRY(dnull.alloc((size_t)m * smax * nl * 8));
    for (int64_t b0 = p_lo; b0 < p_hi; b0 += slab) {
      const int32_t nbs = (int32_t)std::min<int64_t>(slab, p_hi - b0);
      if (c.perm == nullptr) {
        PH_TRY(launch_gsea_placements(ctx, g, b0, nbs, c.seed, dslabY.as<double>(), dslabR.as<double>(), dP.as<int32_t>()));
      } else {
        PH_TRY(upload_pipelined(ctx, dP.as<char>(), (size_t)g * 4, reinterpret_cast<const char*>(c.perm + b0 * g), (size_t)g * 4,
                                nbs, nullptr));
        PH_TRY(launch_gsea_check_perm(ctx, dP.as<int32_t>(), g, nbs, (int32_t)b0, dbad.as<uint32_t>()));
        uint32_t bad[2] = {0u, 0u};
        PH_HIP(hipMemcpyAsync(bad, dbad.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));
        PH_REQUIRE(bad[0] == 0u, "gsea: column %u of perm is no permutation of 0..%d", bad[1] - 1u, g - 1);
      }
      PH_TRY(launch_gsea_null(ctx, c.gsea_weighted, c.score_type, dP.as<int32_t>(), nbs, dWpos.as<double>(), dnan.as<uint32_t>(),
                              dES.as<double>(), g, nl, dGp.as<int32_t>(), dGi.as<int32_t>(), m, dpart.as<double>(),
                              (b0 - p_lo) / PLAIDHIP_GSEA_PERM_BLOCK, c.null_out != nullptr ? dnull.as<double>() : nullptr));
      if (c.null_out != nullptr)
        for (int32_t l = 0; l < nl; ++l)
          PH_HIP(hipMemcpyAsync(c.null_out + ((int64_t)l * B + b0) * m, dnull.as<double>() + (size_t)l * nbs * m,
                                (size_t)nbs * m * 8, hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));   // (the slab's buffers are the next slab's)
    }
    if (ndev > 1) {
      PH_HIP(hipMemcpyAsync(sh.gsea_part.data() + (size_t)blo * blk_doubles, dpart.p, (size_t)(bhi - blo) * blk_doubles * 8,
                            hipMemcpyDeviceToHost, ctx->stream));
      PH_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PLAIDHIP_OK;
  });
  // ---- multilevel: this shard's rulers, on the observed placements it already holds ---------------------------------------
  if (c.method == kGseaMultilevel)
    s.step([&]() -> int { return gsea_ml_shard(ctx, c, ndev, k, sh, dES.as<double>(), dWpos.as<double>()); });
  sh.rv.arrive_and_wait();

  // ---- shard 0: the blocks in order, NES and pval; padj on the host ---------------------------------------------------------
  if (k == 0)
    s.step([&]() -> int {
      const double* part = dpart.as<double>();
      if (ndev > 1) {
        PH_TRY(dall.alloc((size_t)nblk * blk_doubles * 8));
        PH_HIP(hipMemcpyAsync(dall.p, sh.gsea_part.data(), (size_t)nblk * blk_doubles * 8, hipMemcpyHostToDevice, ctx->stream));
        part = dall.as<double>();
      }
      PH_TRY(dout.alloc((size_t)m * 12 * nl * 8));
      PH_TRY(launch_gsea_null_reduce(ctx, part, nblk, dES.as<double>(), dGp.as<int32_t>(), m, nl, c.score_type,
                                     dout.as<double>()));
      PH_HIP(hipMemcpyAsync(c.out, dout.p, (size_t)m * 12 * nl * 8, hipMemcpyDeviceToHost, ctx->stream));
      if (c.le_len != nullptr) {   // the leading edges, once, on the observed placements this shard already holds
        const size_t nnz = (size_t)c.Gp[m];
        PH_TRY(dlen.alloc((size_t)m * nl * 4));
        PH_TRY(didx.alloc(nnz * nl * 4));
        PH_TRY(launch_gsea_edges(ctx, c.gsea_weighted, c.score_type, dpos.as<int32_t>(), dWpos.as<double>(), dnan.as<uint32_t>(),
                                 g, nl, dGp.as<int32_t>(), dGi.as<int32_t>(), m, dlen.as<int32_t>(), didx.as<int32_t>()));
        PH_HIP(hipMemcpyAsync(c.le_len, dlen.p, (size_t)m * nl * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (nnz != 0) PH_HIP(hipMemcpyAsync(c.le_idx, didx.p, nnz * nl * 4, hipMemcpyDeviceToHost, ctx->stream));
      }
      PH_HIP(hipStreamSynchronize(ctx->stream));
      if (c.method == kGseaMultilevel) {   // the multilevel table, and the reported pval where the permutations saw too few
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const size_t mm = (size_t)m;
        for (int32_t l = 0; l < nl; ++l)
          for (int32_t j = 0; j < m; ++j) {
            double* o = c.out + (size_t)l * 12 * mm + j;
            double* q = c.ml_out + (size_t)l * 6 * mm + j;
            const double* r = sh.gsea_ml.data() + 4 * ((size_t)l * mm + j);
            const int side = gsea_ml_side(c.score_type, o[0]);
            if (side < 0 || r[0] != r[0]) {
              for (int t = 0; t < 6; ++t) q[t * mm] = nan;
              continue;
            }
            const double denom = (1.0 + o[(side == 0 ? 8 : 9) * mm]) / (1.0 + (double)B);
            const double ratio = r[0] / denom;
            q[0] = ratio < 1.0 ? ratio : 1.0;
            q[mm] = r[1];
            q[2 * mm] = r[2];
            q[3 * mm] = r[3];
            q[4 * mm] = r[0];
            q[5 * mm] = denom;
            if (o[4 * mm] < (double)c.ml_min) o[2 * mm] = q[0];
          }
      }
      std::vector<double> p, q;
      std::vector<int32_t> at;
      for (int32_t l = 0; l < nl; ++l) {   // Benjamini-Hochberg over the sets of the list that have a p-value
        double* o = c.out + (size_t)l * 12 * m;
        p.clear();
        at.clear();
        for (int32_t j = 0; j < m; ++j)
          if (o[2 * (size_t)m + j] == o[2 * (size_t)m + j]) { p.push_back(o[2 * (size_t)m + j]); at.push_back(j); }
        q.resize(p.size());
        if (!p.empty()) p_adjust_fdr(p.data(), (int64_t)p.size(), q.data());
        for (size_t e = 0; e < p.size(); ++e) o[3 * (size_t)m + at[e]] = q[e];
      }
      return PLAIDHIP_OK;
    });
  return s.finish();
}

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

// chain_contrast_sums for any [nblk][len] partials of the shard's columns (launch_reduce_blocks_flat): shard r adds its blocks,
// in order, to what the shards before it left in `run`; d_seed, d_run: len doubles each.  ndev rendezvous.
void chain_flat_sums(Shard& s, std::vector<double>& run, const double* ws, int64_t len, double* d_seed, double* d_run) {
  plaidhip_ctx* ctx = s.ctx;
  for (int r = 0; r < s.ndev; ++r) {
    if (r == s.k)
      s.step([&]() -> int {
        if (s.nloc == 0) return PLAIDHIP_OK;
        PH_HIP(hipMemcpyAsync(d_seed, run.data(), (size_t)len * 8, hipMemcpyHostToDevice, ctx->stream));
        PH_TRY(launch_reduce_blocks_flat(ctx, ws, len, s.nloc, d_seed, d_run));
        PH_HIP(hipMemcpyAsync(run.data(), d_run, (size_t)len * 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));
        return PLAIDHIP_OK;
      });
    s.sh.rv.arrive_and_wait();
  }
}

// plaid.limma with na = "fit", after the effects are chained: shard 0 merges the shards' NaN lists in shard order (a row's
// columns ascending), decides which rows are fitted (max_na) and which (row, fit) pairs are incomplete, and runs Gram and
// solve (kernels_lmfit.hip) over those: the pair's effects in sh.chain_x become gamma, its mean the mean over the observed
// samples, and sh.na_d / sh.na_u take every row's df.residual (NaN: not fitted) and u_j.  A pair's chain runs over the row's
// own missing samples in ascending order whatever the sharding, so every sharding has the one-device bits.
int limma_na_refit(plaidhip_ctx* ctx, const Call& c, int ndev, Shared& sh, double* d_E) {
  const int32_t rows = c.g, n = c.n, p = c.ncoef, nfit = c.nfit, q = c.nq;
  const size_t R = (size_t)rows;
  const int64_t W = (int64_t)nfit * (p + 1);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int64_t> off(R + 1, 0);
  for (size_t r = 0; r < R; ++r) {
    int64_t tot = 0;
    for (int k = 0; k < ndev; ++k) tot += sh.na_cnt[(size_t)k].empty() ? 0 : sh.na_cnt[(size_t)k][r];
    off[r + 1] = off[r] + tot;
  }
  std::vector<int32_t> list((size_t)off[R]);
  std::vector<size_t> pos((size_t)ndev, 0);
  for (size_t r = 0; r < R; ++r) {
    int64_t w = off[r];
    for (int k = 0; k < ndev; ++k) {
      const int32_t ck = sh.na_cnt[(size_t)k].empty() ? 0 : sh.na_cnt[(size_t)k][r];
      std::copy(sh.na_list[(size_t)k].begin() + pos[(size_t)k], sh.na_list[(size_t)k].begin() + pos[(size_t)k] + ck,
                list.begin() + w);
      pos[(size_t)k] += (size_t)ck;
      w += ck;
    }
  }
  sh.na_d.assign(R * nfit, nan);
  sh.na_u.assign(R * nfit * q, nan);
  std::vector<int32_t> pairs, nobs;
  for (int32_t f = 0; f < nfit; ++f)
    for (size_t r = 0; r < R; ++r) {
      const bool fitted = (double)(off[r + 1] - off[r]) / (double)n <= c.max_na;   // rowMeans(is.na(X)) <= max.na
      const int64_t mis = sh.na_pair[R * f + r], d = c.lm_nf[(size_t)f] - mis - p;
      if (fitted && d >= 1) sh.na_d[R * f + r] = (double)d;
      for (int32_t j = 0; j < q; ++j) sh.na_u[((size_t)f * q + j) * R + r] = c.lm_u[(size_t)f * q + j];
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
  PH_HIP(hipMemcpyAsync(d_E, sh.chain_x.data(), (size_t)W * R * 8, hipMemcpyHostToDevice, ctx->stream));
  PH_TRY(launch_lmfit_na_solve(ctx, (int64_t)np, dpairs.as<int32_t>(), doff.as<int64_t>(), dlist.as<int32_t>(), dQ.as<double>(),
                               c.use != nullptr ? duse.as<int8_t>() : nullptr, n, p, q, dv.as<double>(), dnobs.as<int32_t>(),
                               dnf.as<double>(), rows, d_E, du.as<double>(), dok.as<int32_t>()));
  PH_HIP(hipMemcpyAsync(sh.chain_x.data(), d_E, (size_t)W * R * 8, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipMemcpyAsync(upair.data(), du.p, np * q * 8, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipMemcpyAsync(okp.data(), dok.p, np * 4, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < np; ++i) {
    const size_t r = (size_t)pairs[2 * i], f = (size_t)pairs[2 * i + 1];
    if (!okp[i]) sh.na_d[R * f + r] = nan;
    for (int32_t j = 0; j < q; ++j) sh.na_u[(f * q + j) * R + r] = upair[i * q + j];
  }
  return PLAIDHIP_OK;
}

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
  if (c.method == kCamera) s.force_f64();   // (T = G'Z stays on the fp64 kernels whatever precision the context was given)
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
    std::vector<int32_t>& cnt = sh.na_cnt[(size_t)k];
    std::vector<int32_t>& list = sh.na_list[(size_t)k];
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
    for (size_t i = 0; i < pc.size(); ++i) sh.na_pair[i] += pc[i];
    return PLAIDHIP_OK;
  });
  chain_flat_sums(s, sh.chain_x, dws.as<double>(), W * rows, d_seed, d_run);
  if (c.na_fit) {   // (every shard's lists are complete: chain_flat_sums has met ndev times since)
    if (k == 0) s.step([&]() -> int { return limma_na_refit(ctx, c, ndev, sh, d_E); });
    sh.rv.arrive_and_wait();
  }

  // ---- the residual sums of squares of the shard's columns at the effects of ALL samples -------------------------------------
  s.step([&]() -> int {
    if (nloc == 0) return PLAIDHIP_OK;
    PH_HIP(hipMemcpyAsync(d_E, sh.chain_x.data(), (size_t)W * rows * 8, hipMemcpyHostToDevice, ctx->stream));
    return launch_row_design_rss(ctx, dA.as<double>(), ld, rows, nloc, dQ.as<double>(), dmask.p, p, nfit, d_E,
                                 dws.as<double>(), c.na_fit != 0);
  });
  chain_flat_sums(s, sh.chain_q, dws.as<double>(), (int64_t)nfit * rows, d_seed, d_run);
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
    PH_HIP(hipMemcpyAsync(d_rss, sh.chain_q.data(), (size_t)nfit * rows * 8, hipMemcpyHostToDevice, ctx->stream));
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
  chain_flat_sums(s, sh.cam_ss, d_part, (int64_t)nfit * m, d_chain, d_chain + (size_t)nfit * m);
  return s.finish();
}

// plaid.camera after the workers: eBayes and the gene statistics on the host (plaidhip_limma_finish), the member sums of t
// and the counts of ok members from ONE crossprod of the membership with [the t columns | the ok indicators] on the first
// context (a gene that is not ok holds 0.0 in both), then the pinned test (plaidhip_camera_finish).
int camera_tail(plaidhip_ctx* ctx, const Call& c, Shared& sh) {
  const int32_t g = c.g, m = c.m, nfit = c.nfit, q = c.nq, p = c.ncoef;
  const size_t R = (size_t)g, ncol = (size_t)nfit * q;
  std::vector<double> tab(R * 6 * ncol), hyp((size_t)nfit * 4);
  PH_TRY(plaidhip_limma_finish(g, p, nfit, q, sh.chain_x.data(), sh.chain_q.data(), c.lm_nf.data(), c.lm_v.data(), c.lm_u.data(),
                               tab.data(), hyp.data()));
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
                                estimate ? sh.cam_ss.data() : nullptr, dres.data(), dprior.data(), c.inter_gene_cor,
                                c.allow_neg_cor, c.out, gdf.data()));
  for (int32_t f = 0; f < nfit; ++f) {
    for (int h = 0; h < 4; ++h) c.hyper[6 * (size_t)f + h] = hyp[4 * (size_t)f + h];
    c.hyper[6 * (size_t)f + 4] = gdf[2 * (size_t)f];
    c.hyper[6 * (size_t)f + 5] = gdf[2 * (size_t)f + 1];
  }
  return PLAIDHIP_OK;
}

// every shard on a thread of its own (one shard: the calling thread); the first failure's text is reported
int run_call(plaidhip_ctx* const* ctxs, int ndev, const Call& c) {
  Shared sh(ndev);
  sh.med_all.assign((size_t)c.n, 0.0);
  if (c.method == kGsva || c.method == kGsvaExact) {
    sh.chain_sum.assign((size_t)c.g, 0.0);
    sh.chain_ssd.assign((size_t)c.g, 0.0);
    sh.row_sum.resize((size_t)ndev);
    sh.row_ssd.resize((size_t)ndev);
    sh.row_len.resize((size_t)ndev);
  }
  if (c.method == kPlaidTest) {
    sh.chain_x.assign((size_t)c.g * 2, 0.0);
    sh.chain_s.assign((size_t)c.m * 2, 0.0);
    sh.chain_q.assign((size_t)c.m * 2, 0.0);
    sh.pt_T.assign((size_t)c.m * 2, 0.0);
    sh.pt_F.assign((size_t)even_ld(c.g) * 2, 0.0);
    sh.row_sum.resize((size_t)ndev);
  }
  if (c.method == kPlaidTestContrasts) {   // plaid.test's, [C] of each
    const size_t C = (size_t)c.ncontrast;
    sh.chain_x.assign((size_t)c.g * 2 * C, 0.0);
    sh.chain_s.assign((size_t)c.m * 2 * C, 0.0);
    sh.chain_q.assign((size_t)c.m * 2 * C, 0.0);
    sh.pt_T.assign((size_t)c.m * 2 * C, 0.0);
    sh.pt_F.assign((size_t)even_ld(c.g) * 2 * C, 0.0);
    sh.row_sum.resize((size_t)ndev);
  }
  if (c.method == kCamera) sh.cam_ss.assign((size_t)c.nfit * c.m, 0.0);
  if (c.method == kLimma || c.method == kCamera) {
    sh.chain_x.assign((size_t)c.nfit * (c.ncoef + 1) * c.g, 0.0);
    sh.chain_q.assign((size_t)c.nfit * c.g, 0.0);
    if (c.na_fit) {
      sh.na_cnt.resize((size_t)ndev);
      sh.na_list.resize((size_t)ndev);
      sh.na_pair.assign((size_t)c.nfit * c.g, 0);
    }
  }
  if (c.method == kGseaMultilevel && !c.ml_ruler)
    sh.gsea_ml.assign((size_t)c.m * c.n * 4, std::numeric_limits<double>::quiet_NaN());
  if ((c.method == kGsea || (c.method == kGseaMultilevel && !c.ml_ruler)) && ndev > 1)
    sh.gsea_part.assign((size_t)((c.nperm + PLAIDHIP_GSEA_PERM_BLOCK - 1) / PLAIDHIP_GSEA_PERM_BLOCK) * c.n * 6 * c.m, 0.0);
  auto worker = [&](int k) {
    if (c.method == kGseaMultilevel && c.ml_ruler) return gsea_ruler_worker(ctxs[k], c, ndev, k, sh);
    if (c.method == kGsea || c.method == kGseaMultilevel) return gsea_worker(ctxs[k], c, ndev, k, sh);
    if (c.method == kFisher) return fisher_worker(ctxs[k], c, ndev, k, sh);
    if (c.method == kRankcor) return rankcor_worker(ctxs[k], c, ndev, k, sh);
    if (c.method == kPlage || c.method == kZscore) return plage_worker(ctxs[k], c, ndev, k, sh);
    if (c.method == kLimma || c.method == kCamera) return limma_worker(ctxs[k], c, ndev, k, sh);
    if (c.method == kPlaidTest) return plaid_test_worker(ctxs[k], c, ndev, k, sh);
    if (c.method == kPlaidTestContrasts) return plaid_test_contrasts_worker(ctxs[k], c, ndev, k, sh);
    return is_rank_sum(c.method) ? shard_worker(ctxs[k], c, ndev, k, sh) : scorer_worker(ctxs[k], c, ndev, k, sh);
  };
  int rc = PLAIDHIP_OK;
  if (ndev == 1) {
    rc = worker(0);
  } else {
    std::vector<int> rcs((size_t)ndev, PLAIDHIP_OK);
    std::vector<std::string> errs((size_t)ndev);
    std::vector<std::thread> th;
    for (int k = 0; k < ndev; ++k)
      th.emplace_back([&, k] {
        rcs[(size_t)k] = worker(k);
        if (rcs[(size_t)k] != PLAIDHIP_OK) errs[(size_t)k] = last_error_cstr();   // the worker's thread-local text
      });
    for (auto& t : th) t.join();
    // report the failure that started it (the others only say "another shard failed")
    for (int k = 0; k < ndev; ++k)
      if (rcs[(size_t)k] != PLAIDHIP_OK && !errs[(size_t)k].empty()) {
        rc = rcs[(size_t)k];
        set_error("device %d: %s", ctxs[k]->device, errs[(size_t)k].c_str());
        break;
      }
    if (rc == PLAIDHIP_OK)
      for (int k = 0; k < ndev; ++k)
        if (rcs[(size_t)k] != PLAIDHIP_OK) { rc = rcs[(size_t)k]; set_error("a device shard failed"); break; }
  }
  if (rc == PLAIDHIP_OK && c.method == kScse && c.removed_log2 != nullptr) *c.removed_log2 = sh.removed_log2 ? 1 : 0;
  if (rc == PLAIDHIP_OK && c.method == kPlaidTest) {   // the host half of plaid.test (R/plaid.R:410-474)
    const int64_t ldg = even_ld(c.g);
    double tot1 = 0.0, tot2 = 0.0;
    for (int32_t i = 0; i < c.g; ++i) { tot1 += sh.pt_F[(size_t)i]; tot2 += sh.pt_F[(size_t)ldg + i]; }
    std::vector<double> SM;
    if (c.tests & 4) {   // [group means | sums of squared deviations], [2][m] each
      SM.resize((size_t)c.m * 4);
      scaled_group_means(sh.chain_s, c.m, c.n0, c.n1, SM.data());
      std::copy(sh.chain_q.begin(), sh.chain_q.end(), SM.begin() + 2 * (size_t)c.m);
    }
    rc = plaidhip_plaid_test_finish(c.g, c.m, c.Gp, sh.pt_T.data(), tot1, tot2, (c.tests & 4) ? SM.data() : nullptr, c.n0,
                                    c.n1, c.tests, c.metap_method, c.out);
  }
  if (rc == PLAIDHIP_OK && c.method == kLimma && c.na_fit) {
    rc = plaidhip_limma_finish_na(c.g, c.ncoef, c.nfit, c.nq, sh.chain_x.data(), sh.chain_q.data(), c.lm_nf.data(),
                                  c.lm_v.data(), sh.na_d.data(), sh.na_u.data(), c.out, c.hyper);
    if (rc == PLAIDHIP_OK) {   // df.residual of the rows that came out of the fit; NaN for the others
      const size_t R = (size_t)c.g;
      for (int32_t f = 0; f < c.nfit; ++f) {
        const double* sigma2 = c.out + ((size_t)f * c.nq * 6 + 5) * R;   // (of the fit's first contrast: NaN = not ok)
        for (size_t r = 0; r < R; ++r)
          c.dfres[R * f + r] = std::isnan(sigma2[r]) ? std::numeric_limits<double>::quiet_NaN() : sh.na_d[R * f + r];
      }
    }
  } else if (rc == PLAIDHIP_OK && c.method == kLimma)   // eBayes and the tables, on the host from the chained sums
    rc = plaidhip_limma_finish(c.g, c.ncoef, c.nfit, c.nq, sh.chain_x.data(), sh.chain_q.data(), c.lm_nf.data(), c.lm_v.data(),
                               c.lm_u.data(), c.out, c.hyper);
  if (rc == PLAIDHIP_OK && c.method == kCamera) rc = camera_tail(ctxs[0], c, sh);
  if (rc == PLAIDHIP_OK && c.method == kPlaidTestContrasts) {   // the same host half, once per contrast with its group sizes
    const int64_t ldg = even_ld(c.g);
    const size_t m = (size_t)c.m;
    std::vector<double> SM, means;
    if (c.tests & 4) {
      SM.resize(m * 4);
      means.resize(m * 2 * (size_t)c.ncontrast);
      scaled_contrast_means(c, sh.chain_s, c.m, means.data());
    }
    for (int32_t j = 0; j < c.ncontrast && rc == PLAIDHIP_OK; ++j) {
      const double* F = sh.pt_F.data() + (size_t)j * 2 * ldg;
      double tot1 = 0.0, tot2 = 0.0;
      for (int32_t i = 0; i < c.g; ++i) { tot1 += F[(size_t)i]; tot2 += F[(size_t)ldg + i]; }
      if (c.tests & 4) {
        std::copy(means.begin() + (size_t)j * 2 * m, means.begin() + (size_t)(j + 1) * 2 * m, SM.begin());
        std::copy(sh.chain_q.begin() + (size_t)j * 2 * m, sh.chain_q.begin() + (size_t)(j + 1) * 2 * m, SM.begin() + 2 * m);
      }
      rc = plaidhip_plaid_test_finish(c.g, c.m, c.Gp, sh.pt_T.data() + (size_t)j * 2 * m, tot1, tot2,
                                      (c.tests & 4) ? SM.data() : nullptr, c.cn0[(size_t)j], c.cn1[(size_t)j], c.tests,
                                      c.metap_method, c.out + (size_t)j * 6 * m);
    }
  }
  return rc;
}

}  // namespace

namespace plaidhip {

// pageable host memory -> device through the pinned staging ring (the other host entry points' uploads: a plain
// hipMemcpy from pageable memory runs at ~21 GB/s, the ring at the link rate)
int upload_host(plaidhip_ctx* ctx, void* dst, size_t ldd_bytes, const void* src, size_t row_bytes, int64_t cols) {
  return upload_pipelined(ctx, static_cast<char*>(dst), ldd_bytes, static_cast<const char*>(src), row_bytes, cols, nullptr);
}

// GSVA's kernel CDF estimate of the columns [lo, lo + nloc) of the host matrix X on one device: all of X is uploaded (a
// dgCMatrix as its slots, expanded there into the dense form), then the two kernels of kernels_kcdf.hip
int gsva_kcdf_columns(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                      int32_t lo, int32_t nloc, double* dV) {
  if (g <= 0 || nloc <= 0) return PLAIDHIP_OK;
  DevBuf dfull, dp, di, dx, dh;
  PH_TRY(dfull.alloc((size_t)g * n * 8));
  PH_TRY(dh.alloc((size_t)g * 8));
  if (Xp == nullptr) {
    PH_TRY(upload_host(ctx, dfull.p, (size_t)g * 8, X_or_x, (size_t)g * 8, n));
  } else {
    const int64_t z = Xp[n];
    PH_TRY(dp.alloc((size_t)(n + 1) * 4));
    PH_TRY(di.alloc((size_t)std::max<int64_t>(z, 1) * 4));
    PH_TRY(dx.alloc((size_t)std::max<int64_t>(z, 1) * 8));
    PH_HIP(hipMemcpyAsync(dp.p, Xp, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    PH_TRY(upload_host(ctx, di.p, 1, Xi, 1, z * 4));
    PH_TRY(upload_host(ctx, dx.p, 1, X_or_x, 1, z * 8));
    PH_HIP(hipMemsetAsync(dh.p, 0, (size_t)g * 8, ctx->stream));   // (the rows' default: a zero)
    PH_TRY(launch_csc_expand(ctx, dp.as<int32_t>(), di.as<int32_t>(), dx.as<double>(), g, n, g, dh.as<double>(), nullptr, nullptr,
                             dfull.as<double>()));
  }
  PH_TRY(launch_gsva_kcdf(ctx, dfull.as<double>(), g, g, n, lo, lo + nloc, dh.as<double>(), dV, g));
  PH_HIP(hipStreamSynchronize(ctx->stream));   // (the buffers above are freed on return)
  return PLAIDHIP_OK;
}

// the bound of the walk kernel's bitmap (kernels_ks.hip), checked before a device is touched
int check_gsea_ks_genes(int32_t g) {
  if (g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("ssgsea_exact_ks: nrow(X) = %d (at most %d rows with single = FALSE)", g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  return PLAIDHIP_OK;
}

}  // namespace plaidhip

// ---- the argument checks of every method: check_call.  None touches a device. -----------------------------------------------
namespace {

// plaid / sing / ssgsea
int check_rank_sum_call(const Call& c) {
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  if ((int64_t)c.m * c.n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.X != nullptr || (c.Xp != nullptr && c.Xp[c.n] == 0), "null X");
  PH_REQUIRE(c.S_out != nullptr, "null S_out");
  if (c.Xp != nullptr) PH_TRY(check_host_csc(c.Xp, c.Xi, c.g, c.n));
  return PLAIDHIP_OK;
}

// replaid.ssgsea.exact; replaid.gsva.exact and replaid.sing.exact (alpha 0) run it inside theirs.  S_out: the result, or
// any one of sing.exact's
int check_ssgsea_exact_call(const Call& c, const double* S_out) {
  PH_REQUIRE(std::isfinite(c.alpha), "ssgsea_exact: alpha must be finite (got %g)", c.alpha);
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.g < (1 << 26), "ssgsea_exact: nrow(X) = %d (at most 2^26 - 1 rows)", c.g);
  if ((int64_t)c.m * c.n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "ssgsea_exact: null Gi");
  PH_REQUIRE(c.X != nullptr || (c.Xp != nullptr && c.Xp[c.n] == 0), "ssgsea_exact: null X");
  PH_REQUIRE(S_out != nullptr, "ssgsea_exact: null S_out");
  if (c.Xp != nullptr) {
    const int32_t* Xp = c.Xp;
    const int32_t* Xi = c.Xi;
    PH_TRY(check_host_csc(Xp, Xi, c.g, c.n));
    PH_REQUIRE(Xp[c.n] == 0 || Xi != nullptr, "ssgsea_exact: null Xi");
    for (int32_t j = 0; j < c.n; ++j)   // the expansion walks the rows of a column in order (kernels_walk.hip)
      for (int32_t q = Xp[j] + 1; q < Xp[j + 1]; ++q)
        PH_REQUIRE(Xi[q] > Xi[q - 1], "ssgsea_exact: row indices of column %d are not increasing (Xi[%d] = %d after %d)", j, q,
                   Xi[q], Xi[q - 1]);
  }
  return PLAIDHIP_OK;
}

int check_gsva_exact_call(const Call& c, int ndev) {
  PH_REQUIRE(std::isfinite(c.tau) && c.tau >= 0.0, "gsva_exact: tau must be finite and >= 0 (got %g)", c.tau);
  PH_REQUIRE(c.rowtf >= 0 && c.rowtf <= 3, "Error: unknown row transform %d", c.rowtf);                     // R/plaid.R:348
  PH_REQUIRE(c.rowtf != 3 || c.n >= 2, "gsva_exact: rowtf = \"gauss\" needs at least 2 samples (got %d)", c.n);
  PH_REQUIRE(c.rowtf != 1 || ndev == 1, "gsva_exact_multi: rowtf = \"ecdf\" ranks all samples of a gene together and is not "
                                        "sharded by sample; score it on one device (plaidhip_gsva_exact)");
  PH_TRY(check_ssgsea_exact_call(c, c.S_out));
  if (c.g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("gsva_exact: nrow(X) = %d (at most %d rows)", c.g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  return PLAIDHIP_OK;
}

int check_sing_exact_call(const Call& c) {
  double* const* out = c.sx_out;
  const double* any = nullptr;
  for (int o = 0; o < 6; ++o) any = any ? any : out[o];
  PH_REQUIRE((int64_t)c.m * c.n == 0 || any != nullptr, "sing_exact: no output requested");
  PH_TRY(check_ssgsea_exact_call(c, any));
  if (c.Dp != nullptr) {
    PH_TRY(check_host_common(c.Dp, c.g, c.n, c.m));
    PH_REQUIRE((int64_t)c.m * c.n == 0 || c.Di != nullptr || c.Dp[c.m] == 0, "sing_exact: null Di");
  } else {
    PH_REQUIRE(!out[0] && !out[2] && !out[3] && !out[5], "sing_exact: total and down results need the down sets");
  }
  if ((out[3] || out[4] || out[5]) && c.g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("sing_exact: nrow(X) = %d (at most %d rows with the dispersion)", c.g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  return PLAIDHIP_OK;
}

// replaid.ucell.exact / replaid.aucell.exact.  The order is part of the contract: the rank bound and the 2^53 bound of the
// integer epilogue come before anything reads X.
int check_truncated_exact_call(const Call& c) {
  const bool ucell = c.method == kUcellExact;
  const char* who = ucell ? "ucell_exact" : "aucell_exact";
  const char* what = ucell ? "maxRank" : "aucMaxRank";
  const double* any = ucell ? nullptr : c.S_out;
  if (ucell) {
    for (int o = 0; o < 3; ++o) any = any ? any : c.sx_out[o];
    PH_REQUIRE(std::isfinite(c.w_neg) && c.w_neg >= 0.0, "ucell_exact: w_neg must be finite and >= 0 (got %g)", c.w_neg);
  }
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  if (ucell && c.Dp != nullptr) PH_TRY(check_host_common(c.Dp, c.g, c.n, c.m));
  if (ucell && c.Dp == nullptr)
    PH_REQUIRE(!c.sx_out[0] && !c.sx_out[2], "ucell_exact: total and down results need the down sets");
  if ((int64_t)c.m * c.n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.max_rank >= 1.0 && c.max_rank <= (double)c.g && c.max_rank == std::floor(c.max_rank),
             "%s: %s must be an integer in 1..nrow(X) = %d (got %g)", who, what, c.g, c.max_rank);
  if (2.0 * (double)c.g * c.max_rank >= 0x1p53) {
    set_error("%s: 2 nrow(X) %s = 2 x %d x %.0f does not stay below 2^53", who, what, c.g, c.max_rank);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(any != nullptr, "%s: no output requested", who);
  PH_TRY(check_ssgsea_exact_call(c, any));
  if (ucell && c.Dp != nullptr) PH_REQUIRE(c.Di != nullptr || c.Dp[c.m] == 0, "ucell_exact: null Di");
  if (ucell && c.k_full != nullptr) {
    PH_REQUIRE(c.Dp == nullptr || c.k_full_down != nullptr, "ucell_exact: impute needs k_full_down beside the down sets");
    for (int pass = 0; pass < (c.Dp != nullptr ? 2 : 1); ++pass) {
      const double* K = pass ? c.k_full_down : c.k_full;
      const int32_t* P = pass ? c.Dp : c.Gp;
      for (int32_t j = 0; j < c.m; ++j) {
        PH_REQUIRE(std::isfinite(K[j]) && K[j] == std::floor(K[j]) && K[j] >= (double)(P[j + 1] - P[j]),
                   "ucell_exact: k_full%s[%d] = %g is no integer >= the %d aligned members", pass ? "_down" : "", j, K[j],
                   P[j + 1] - P[j]);
        if (2.0 * K[j] * (c.max_rank + 1.0) + K[j] * (K[j] + 1.0) >= 0x1p53) {
          set_error("ucell_exact: k_full%s[%d] = %g with maxRank = %.0f does not stay below 2^53", pass ? "_down" : "", j, K[j],
                    c.max_rank);
          return PLAIDHIP_EUNSUPPORTED;
        }
      }
    }
  }
  return PLAIDHIP_OK;
}

// replaid.ucell / aucell / scse / gsva
int check_scorer_call(const Call& c, int ndev, bool multi) {
  if (c.method == kScse && c.removed_log2 != nullptr) *c.removed_log2 = c.remove_log2 > 0 ? 1 : 0;
  PH_REQUIRE(is_scorer(c.method), "scorer: bad method %d", c.method);
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  if (c.method == kUcell) PH_REQUIRE(c.rmax > 0, "ucell: rmax must be positive");
  if (c.method == kAucell) PH_REQUIRE(c.auc_max_rank > 0, "aucell: aucMaxRank must be positive");
  if (c.method == kGsva) {
    PH_REQUIRE(c.rowtf == 0 || c.rowtf == 1, "Error: unknown row transform %d", c.rowtf);              // R/plaid.R:348
    PH_REQUIRE(c.rowtf == 0 || (!multi && ndev == 1), "gsva: rowtf = \"ecdf\" ranks all samples of a gene together and is "
               "not sharded by sample; score it on one device (plaidhip_gsva / plaidhip_gsva_csc)");
  }
  if ((int64_t)c.m * c.n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.X != nullptr || (c.Xp != nullptr && c.Xp[c.n] == 0), "null X");
  PH_REQUIRE(c.S_out != nullptr, "null S_out");
  if (c.method == kUcell) PH_REQUIRE(c.k_full != nullptr, "ucell: null k_full");
  if (c.Xp != nullptr) {
    PH_TRY(check_host_csc(c.Xp, c.Xi, c.g, c.n));
    PH_REQUIRE(c.Xp[c.n] == 0 || c.Xi != nullptr, "null Xi");
    // (the ranks of the rows' stored values use a g x n buffer as scratch: a column repeating a row index could pass it)
    if (c.method == kGsva)
      PH_REQUIRE((int64_t)c.Xp[c.n] <= (int64_t)c.g * c.n, "gsva: %d stored values in a %d x %d matrix (repeated row "
                 "indices?)", c.Xp[c.n], c.g, c.n);
  }
  return PLAIDHIP_OK;
}

// plaid.test, and their messages; counts the groups of y into c.n0 / c.n1
int check_plaid_test_call(Call& c) {
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.m == 0 || c.out, "plaid_test: null out");
  PH_REQUIRE(c.n == 0 || ((c.Xp != nullptr || c.X != nullptr) && c.y != nullptr), "plaid_test: null X / y");
  PH_REQUIRE((c.tests & 7) != 0 && (c.tests & ~7) == 0, "plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)");
  PH_REQUIRE(c.metap_method == 0 || c.metap_method == 1, "Invalid method: %d", c.metap_method);   // R/plaid.R:533
  c.n0 = c.n1 = 0;
  for (int32_t j = 0; j < c.n; ++j) {
    PH_REQUIRE(c.y[j] == 0 || c.y[j] == 1, "elements of y must be 0 or 1");                        // R/plaid.R:394
    if (c.y[j]) ++c.n1; else ++c.n0;
  }
  if (c.Xp != nullptr) {
    PH_TRY(check_host_csc(c.Xp, c.Xi, c.g, c.n));
    PH_REQUIRE(c.Xp[c.n] == 0 || (c.Xi && c.X), "plaid_test: null Xi/Xx");
  }
  return PLAIDHIP_OK;
}

// plaid.test.contrasts: plaid.test's checks with Y (n x C; 0, 1, -1 = NA) for y; counts every contrast's groups
int check_plaid_test_contrasts_call(Call& c) {
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.ncontrast >= 0 && c.ncontrast <= 65535, "plaid_test_contrasts: C = %d (0 <= C <= 65535)", c.ncontrast);
  PH_REQUIRE(c.m == 0 || c.ncontrast == 0 || c.out, "plaid_test_contrasts: null out");
  PH_REQUIRE(c.n == 0 || c.Xp != nullptr || c.X != nullptr, "plaid_test_contrasts: null X");
  PH_REQUIRE(c.n == 0 || c.ncontrast == 0 || c.y != nullptr, "plaid_test_contrasts: null Y");
  PH_REQUIRE((c.tests & 7) != 0 && (c.tests & ~7) == 0, "plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)");
  PH_REQUIRE(c.metap_method == 0 || c.metap_method == 1, "Invalid method: %d", c.metap_method);   // R/plaid.R:533
  c.cn0.assign((size_t)c.ncontrast, 0);
  c.cn1.assign((size_t)c.ncontrast, 0);
  for (int32_t j = 0; j < c.ncontrast; ++j)
    for (int32_t i = 0; i < c.n; ++i) {
      const int32_t lab = c.y[(size_t)j * c.n + i];
      PH_REQUIRE(lab == 0 || lab == 1 || lab == -1, "elements of Y must be 0, 1 or NA (-1): contrast %d, sample %d is %d",
                 j + 1, i + 1, lab);
      if (lab == 1) ++c.cn1[(size_t)j];
      else if (lab == 0) ++c.cn0[(size_t)j];
    }
  if (c.Xp != nullptr) {
    PH_TRY(check_host_csc(c.Xp, c.Xi, c.g, c.n));
    PH_REQUIRE(c.Xp[c.n] == 0 || (c.Xi && c.X), "plaid_test_contrasts: null Xi/Xx");
  }
  return PLAIDHIP_OK;
}

// plaid.gsea; the order is part of the contract (include/plaidhip.h).  Finds whether any weight differs from 1 and the lists
// that hold a NaN or an infinity
int check_gsea_call(Call& c) {
  PH_REQUIRE(c.score_type >= PLAIDHIP_GSEA_STD && c.score_type <= PLAIDHIP_GSEA_NEG, "gsea: score_type = %d (0 std, 1 pos, 2 neg)",
             c.score_type);
  PH_REQUIRE((c.le_len == nullptr) == (c.le_idx == nullptr), "gsea: le_len and le_idx are passed both or neither");
  PH_REQUIRE(c.nperm >= 1, "gsea: nperm = %d (at least 1)", c.nperm);
  PH_REQUIRE(c.n >= 1, "gsea: %d ranked lists (at least 1)", c.n);
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  if (c.g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("gsea: %d genes (at most %d)", c.g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(c.X != nullptr && c.weight != nullptr, "gsea: null stat / weight");
  c.gsea_weighted = 0;
  for (int64_t e = 0; e < (int64_t)c.g * c.n; ++e) {
    const double w = c.weight[e];
    PH_REQUIRE(std::isfinite(w) && w >= 0.0, "gsea: weight[%lld] = %g (weights are finite and >= 0)", (long long)e, w);
    if (w != 1.0) c.gsea_weighted = 1;
  }
  c.listnan.assign((size_t)c.n, 0u);
  for (int32_t l = 0; l < c.n; ++l)
    for (int32_t i = 0; i < c.g; ++i)
      if (!std::isfinite(c.X[(int64_t)l * c.g + i])) { c.listnan[(size_t)l] = 1u; break; }
  if (c.m == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "gsea: null Gi");
  PH_REQUIRE(c.out != nullptr, "gsea: null out");
  return PLAIDHIP_OK;
}

// the chains' own parameters, in the order of include/plaidhip.h
int check_gsea_ml_params(const Call& c, const char* who) {
  PH_REQUIRE(c.ml_sample >= 3 && c.ml_sample <= PLAIDHIP_GSEA_ML_MAX_SAMPLE && (c.ml_sample & 1) == 1,
             "%s: sample_size = %d (odd, 3..%d)", who, c.ml_sample, PLAIDHIP_GSEA_ML_MAX_SAMPLE);
  PH_REQUIRE(c.ml_sweeps >= 1 && c.ml_sweeps <= 32, "%s: sweeps = %d (1..32)", who, c.ml_sweeps);
  PH_REQUIRE(c.ml_eps >= 0.0 && c.ml_eps < 1.0, "%s: eps = %g (0 <= eps < 1)", who, c.ml_eps);
  return PLAIDHIP_OK;
}

// plaid.gsea with multilevel p-values, or one ruler; the order is part of the contract (include/plaidhip.h)
int check_gsea_multilevel_call(Call& c) {
  if (!c.ml_ruler) {
    PH_TRY(check_gsea_ml_params(c, "gsea_multilevel"));
    PH_REQUIRE(c.ml_min >= 0, "gsea_multilevel: ml_min = %d (at least 0)", c.ml_min);
    PH_REQUIRE(c.n < (1 << 30), "gsea_multilevel: %d ranked lists (below 2^30)", c.n);
    PH_REQUIRE(c.ml_out != nullptr || c.m == 0, "gsea_multilevel: null ml_out");
    return check_gsea_call(c);
  }
  PH_TRY(check_gsea_ml_params(c, "gsea_ruler"));
  PH_REQUIRE(c.ml_side == 0 || c.ml_side == 1, "gsea_ruler: side = %d (0 positive, 1 negative)", c.ml_side);
  PH_REQUIRE(c.ml_l >= 0 && c.ml_l < (1 << 30), "gsea_ruler: list number %d (0..2^30 - 1)", c.ml_l);
  PH_REQUIRE(c.g >= 2 && c.ml_k >= 1 && c.ml_k < c.g, "gsea_ruler: k = %d of %d genes (1..g - 1)", c.ml_k, c.g);
  PH_REQUIRE(c.ml_gamma == c.ml_gamma, "gsea_ruler: gamma is NaN");
  PH_REQUIRE(c.score_type >= PLAIDHIP_GSEA_STD && c.score_type <= PLAIDHIP_GSEA_NEG, "gsea_ruler: score_type = %d (0 std, 1 pos, 2 neg)",
             c.score_type);
  PH_REQUIRE(c.score_type == PLAIDHIP_GSEA_STD || c.ml_side == (c.score_type == PLAIDHIP_GSEA_NEG ? 1 : 0),
             "gsea_ruler: side = %d does not go with score_type = %d", c.ml_side, c.score_type);
  if (c.g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("gsea_ruler: %d genes (at most %d)", c.g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(c.X != nullptr && c.weight != nullptr, "gsea_ruler: null stat / weight");
  PH_REQUIRE(c.ml_nstages && c.ml_end && c.ml_m && c.ml_s && c.ml_h, "gsea_ruler: null output");
  c.gsea_weighted = 0;
  for (int32_t i = 0; i < c.g; ++i) {
    const double w = c.weight[i];
    PH_REQUIRE(std::isfinite(w) && w >= 0.0, "gsea_ruler: weight[%d] = %g (weights are finite and >= 0)", i, w);
    PH_REQUIRE(std::isfinite(c.X[i]), "gsea_ruler: stat[%d] is not finite", i);
    if (w != 1.0) c.gsea_weighted = 1;
  }
  return PLAIDHIP_OK;
}

// plaid.fisher; the order is part of the contract (include/plaidhip.h)
int check_fisher_call(const Call& c) {
  PH_REQUIRE(c.n >= 1, "fisher: %d lists (at least 1)", c.n);
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.sig != nullptr && c.tot_out != nullptr && (c.out != nullptr || c.m == 0), "fisher: null sig / out / tot_out");
  PH_REQUIRE((c.le_len == nullptr) == (c.le_idx == nullptr), "fisher: ov_len and ov_idx are passed both or neither");
  if (c.g > PLAIDHIP_FISHER_MAX_GENES) {
    set_error("fisher: %d genes (at most %d)", c.g, PLAIDHIP_FISHER_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(c.Gp[0] == 0, "fisher: Gp[0] = %d (a column pointer starts at 0)", c.Gp[0]);
  for (int32_t j = 0; j < c.m; ++j)
    PH_REQUIRE(c.Gp[j + 1] >= c.Gp[j], "fisher: Gp[%d] = %d after %d (a column pointer does not decrease)", j + 1, c.Gp[j + 1],
               c.Gp[j]);
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "fisher: null Gi");
  for (int32_t e = 0; e < c.Gp[c.m]; ++e)
    PH_REQUIRE(c.Gi[e] >= 0 && c.Gi[e] < c.g, "fisher: Gi[%d] = %d (rows are 0..%d)", e, c.Gi[e], c.g - 1);
  for (int64_t e = 0; e < (int64_t)c.g * c.n; ++e)
    PH_REQUIRE(c.sig[e] >= -1 && c.sig[e] <= 1, "fisher: sig[%lld] = %d (-1 down, 0, +1 up)", (long long)e, (int)c.sig[e]);
  return PLAIDHIP_OK;
}

// plaid.rankcor; the order is part of the contract (include/plaidhip.h)
int check_rankcor_call(const Call& c) {
  PH_REQUIRE(c.n >= 1, "rankcor: %d lists (at least 1)", c.n);
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.X != nullptr && c.tot_out != nullptr && (c.out != nullptr || c.m == 0), "rankcor: null stat / out / tot_out");
  PH_REQUIRE(c.use_rank == 0 || c.use_rank == 1, "rankcor: use_rank = %d (0 values, 1 ranks)", c.use_rank);
  PH_REQUIRE(c.ties == PLAIDHIP_TIES_AVERAGE || c.ties == PLAIDHIP_TIES_MIN || c.ties == PLAIDHIP_TIES_MAX,
             "rankcor: ties = %d (0 average, 1 min, 2 max)", c.ties);
  if (c.g > PLAIDHIP_RANKCOR_MAX_GENES) {
    set_error("rankcor: %d genes (at most %d)", c.g, PLAIDHIP_RANKCOR_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(c.Gp[0] == 0, "rankcor: Gp[0] = %d (a column pointer starts at 0)", c.Gp[0]);
  for (int32_t j = 0; j < c.m; ++j) {
    PH_REQUIRE(c.Gp[j + 1] >= c.Gp[j], "rankcor: Gp[%d] = %d after %d (a column pointer does not decrease)", j + 1, c.Gp[j + 1],
               c.Gp[j]);
    PH_REQUIRE(c.Gp[j + 1] - c.Gp[j] <= c.g, "rankcor: set %d has %d members (at most the %d genes)", j + 1,
               c.Gp[j + 1] - c.Gp[j], c.g);
  }
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "rankcor: null Gi");
  for (int32_t e = 0; e < c.Gp[c.m]; ++e)
    PH_REQUIRE(c.Gi[e] >= 0 && c.Gi[e] < c.g, "rankcor: Gi[%d] = %d (rows are 0..%d)", e, c.Gi[e], c.g - 1);
  return PLAIDHIP_OK;
}

// replaid.plage and replaid.zscore; the order is part of the contract (include/plaidhip.h)
int check_plage_call(const Call& c) {
  const bool plage = c.method == kPlage;
  const char* who = plage ? "plage" : "zscore";
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.n >= 2, "%s: %d samples (at least 2)", who, c.n);
  if (plage) {
    PH_REQUIRE(c.tol > 0.0, "plage: tol = %g (a positive number)", c.tol);   // (a NaN is refused here too)
    PH_REQUIRE(c.maxit >= 1, "plage: maxit = %d (at least 1)", c.maxit);
  }
  PH_REQUIRE(c.Gp[0] == 0, "%s: Gp[0] = %d (a column pointer starts at 0)", who, c.Gp[0]);
  for (int32_t j = 0; j < c.m; ++j) {
    PH_REQUIRE(c.Gp[j + 1] >= c.Gp[j], "%s: Gp[%d] = %d after %d (a column pointer does not decrease)", who, j + 1, c.Gp[j + 1],
               c.Gp[j]);
    PH_REQUIRE(!plage || c.Gp[j + 1] - c.Gp[j] <= PLAIDHIP_PLAGE_MAX_SET, "plage: set %d has %d members (at most %d)", j + 1,
               c.Gp[j + 1] - c.Gp[j], PLAIDHIP_PLAGE_MAX_SET);
  }
  if (c.m == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.X != nullptr || (c.Xp != nullptr && c.Xp[c.n] == 0), "%s: null X", who);
  PH_REQUIRE(c.S_out != nullptr, "%s: null S_out", who);
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "%s: null Gi", who);
  if (c.Xp != nullptr) {
    PH_TRY(check_host_csc(c.Xp, c.Xi, c.g, c.n));
    PH_REQUIRE(c.Xp[c.n] == 0 || c.Xi != nullptr, "%s: null Xi", who);
    for (int32_t j = 0; j < c.n; ++j)   // (the expansion takes a column's rows as sorted and distinct)
      for (int32_t q = c.Xp[j] + 1; q < c.Xp[j + 1]; ++q)
        PH_REQUIRE(c.Xi[q] > c.Xi[q - 1], "%s: row indices of column %d are not increasing (Xi[%d] = %d after %d)", who, j, q,
                   c.Xi[q], c.Xi[q - 1]);
  }
  for (int32_t e = 0; e < c.Gp[c.m]; ++e)
    PH_REQUIRE(c.Gi[e] >= 0 && c.Gi[e] < c.g, "%s: Gi[%d] = %d (rows are 0..%d)", who, e, c.Gi[e], c.g - 1);
  return PLAIDHIP_OK;
}

// plaid.limma; the order is part of the contract (include/plaidhip.h).  Makes every fit's Q, v, u and n_f: the designs are
// decomposed here, on the host, so that a design that cannot be fitted is refused before any device is touched
int check_limma_call(Call& c) {
  const char* who = c.method == kCamera ? "camera" : "limma";
  const bool sets = c.method != kCamera || c.m != 0;   // (plaid.camera without sets writes nothing)
  const int32_t rows = c.g, n = c.n, p = c.ncoef, nfit = c.nfit, q = c.nq;
  PH_REQUIRE(rows >= 0 && n >= 0 && n <= PLAIDHIP_LIMMA_MAX_SAMPLES && nfit >= 0 && nfit <= PLAIDHIP_LIMMA_MAX_FITS && q >= 0,
             "%s: bad dims rows=%d n=%d nfit=%d q=%d (n <= %d, nfit <= %d)", who, rows, n, nfit, q, PLAIDHIP_LIMMA_MAX_SAMPLES,
             PLAIDHIP_LIMMA_MAX_FITS);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "%s: p = %d coefficients (1 <= p <= %d)", who, p, PLAIDHIP_LIMMA_MAX_COEF);
  if (c.na_fit) {
    PH_REQUIRE(p <= PLAIDHIP_LIMMA_NA_MAX_COEF, "%s: p = %d coefficients with na = \"fit\" (p <= %d)", who, p,
               PLAIDHIP_LIMMA_NA_MAX_COEF);
    PH_REQUIRE(c.max_na >= 0.0 && c.max_na <= 1.0, "%s: max_na = %g (a share, 0 <= max_na <= 1)", who, c.max_na);
  }
  PH_REQUIRE(c.K != nullptr || q == p, "%s: q = %d without K (the p = %d unit vectors)", who, q, p);
  PH_REQUIRE(c.design != nullptr || nfit == 0, "%s: null design", who);
  PH_REQUIRE(rows == 0 || nfit == 0 || q == 0 || !sets || (c.X != nullptr && c.out != nullptr && c.hyper != nullptr),
             "%s: null A / out / hyper", who);
  PH_REQUIRE(!c.na_fit || rows == 0 || nfit == 0 || q == 0 || c.dfres != nullptr, "%s: null dfres", who);
  if (c.K != nullptr)
    for (int64_t e = 0; e < (int64_t)p * q; ++e)
      PH_REQUIRE(std::isfinite(c.K[e]), "%s: K[%lld] = %g (the contrasts are finite)", who, (long long)e, c.K[e]);
  c.lm_Q.assign((size_t)n * p * nfit, 0.0);
  c.lm_v.assign((size_t)p * q * nfit, 0.0);
  c.lm_u.assign((size_t)q * nfit, 0.0);
  c.lm_nf.assign((size_t)nfit, 0);
  c.lm_invn.assign((size_t)nfit, 0.0);
  for (int32_t f = 0; f < nfit; ++f) {
    PH_TRY(limma_design(who, c.design + (size_t)f * n * p, n, p, c.use != nullptr ? c.use + (size_t)f * n : nullptr, c.K, q,
                        f + 1, c.lm_Q.data() + (size_t)f * n * p, nullptr, c.lm_v.data() + (size_t)f * p * q,
                        c.lm_u.data() + (size_t)f * q, &c.lm_nf[(size_t)f]));
    c.lm_invn[(size_t)f] = 1.0 / (double)c.lm_nf[(size_t)f];
  }
  return PLAIDHIP_OK;
}

// plaid.camera; the order is part of the contract (include/plaidhip.h): plaid.limma's checks in their order (the designs are
// decomposed there), then the membership's as plaid.rankcor makes them, then the fixed correlation
int check_camera_call(Call& c) {
  PH_REQUIRE(c.m >= 0, "camera: bad dims m=%d", c.m);
  PH_TRY(check_limma_call(c));
  PH_REQUIRE(c.Gp != nullptr, "camera: null Gp");
  PH_REQUIRE(c.Gp[0] == 0, "camera: Gp[0] = %d (a column pointer starts at 0)", c.Gp[0]);
  for (int32_t j = 0; j < c.m; ++j) {
    PH_REQUIRE(c.Gp[j + 1] >= c.Gp[j], "camera: Gp[%d] = %d after %d (a column pointer does not decrease)", j + 1, c.Gp[j + 1],
               c.Gp[j]);
    PH_REQUIRE(c.Gp[j + 1] - c.Gp[j] <= c.g, "camera: set %d has %d members (at most the %d genes)", j + 1,
               c.Gp[j + 1] - c.Gp[j], c.g);
  }
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "camera: null Gi");
  for (int32_t e = 0; e < c.Gp[c.m]; ++e)
    PH_REQUIRE(c.Gi[e] >= 0 && c.Gi[e] < c.g, "camera: Gi[%d] = %d (rows are 0..%d)", e, c.Gi[e], c.g - 1);
  PH_REQUIRE(std::isnan(c.inter_gene_cor) || (c.inter_gene_cor > -1.0 && c.inter_gene_cor < 1.0),
             "camera: inter_gene_cor = %g (a correlation inside (-1, 1), or NaN to estimate it)", c.inter_gene_cor);
  return PLAIDHIP_OK;
}

std::mutex g_multi_mu;
std::vector<plaidhip_ctx*> g_multi_ctx;  // one lazily created context per device, owned by the library
int g_multi_precision = PLAIDHIP_PRECISION_F64;   // plaidhip_multi_set_precision: applies to these contexts

// the device list's own checks, which touch no device
int check_devices(const int* devices, int ndev) {
  PH_REQUIRE(ndev >= 1 && ndev <= 64, "multi: ndev = %d", ndev);
  if (devices != nullptr)
    for (int k = 0; k < ndev; ++k)
      for (int q = 0; q < k; ++q) PH_REQUIRE(devices[q] != devices[k], "multi: device %d listed twice", devices[k]);
  return PLAIDHIP_OK;
}

int multi_contexts(const int* devices, int ndev, std::vector<plaidhip_ctx*>& out) {
  int count = 0;
  PH_TRY(plaidhip_device_count(&count));
  std::lock_guard<std::mutex> lk(g_multi_mu);
  if ((int)g_multi_ctx.size() < count) g_multi_ctx.resize((size_t)count, nullptr);
  out.clear();
  for (int k = 0; k < ndev; ++k) {
    const int d = devices ? devices[k] : k;
    PH_REQUIRE(d >= 0 && d < count, "multi: device %d out of range [0, %d)", d, count);
    if (g_multi_ctx[(size_t)d] == nullptr) PH_TRY(plaidhip_init(d, nullptr, &g_multi_ctx[(size_t)d]));
    g_multi_ctx[(size_t)d]->precision = g_multi_precision;
    out.push_back(g_multi_ctx[(size_t)d]);
  }
  return PLAIDHIP_OK;
}

// The test hooks' engine: `nshards` contexts on ONE device -- worker threads, rendezvous, cross-shard scalars and the
// failure path are what a 1-GPU box can exercise of plaidhip_*_multi.  fail_shard >= 0: that shard fails in its crossprod
// phase (the call must return an error, not hang).  The error text of the call outlives the contexts' release.
int run_on_one_device(int device, int nshards, int fail_shard, const Call& c) {
  std::vector<plaidhip_ctx*> ctxs((size_t)nshards, nullptr);
  int rc = PLAIDHIP_OK;
  for (int k = 0; k < nshards && rc == PLAIDHIP_OK; ++k) {
    rc = plaidhip_init(device, nullptr, &ctxs[(size_t)k]);
    if (rc == PLAIDHIP_OK && k == fail_shard) ctxs[(size_t)k]->debug_fail_crossprod = 1;
  }
  if (rc == PLAIDHIP_OK) rc = run_call(ctxs.data(), nshards, c);
  const std::string err = rc != PLAIDHIP_OK ? std::string(last_error_cstr()) : std::string();
  for (plaidhip_ctx* x : ctxs)
    if (x) plaidhip_finalize(x);
  if (rc != PLAIDHIP_OK) set_error("%s", err.c_str());
  return rc;
}

}  // namespace

namespace plaidhip {

int check_call(Call& c, int ndev, bool multi) {
  if (is_rank_sum(c.method)) return check_rank_sum_call(c);
  switch (c.method) {
    case kPlaidTest: return check_plaid_test_call(c);
    case kPlaidTestContrasts: return check_plaid_test_contrasts_call(c);
    case kGsea: return check_gsea_call(c);
    case kGseaMultilevel: return check_gsea_multilevel_call(c);
    case kFisher: return check_fisher_call(c);
    case kRankcor: return check_rankcor_call(c);
    case kPlage:
    case kZscore: return check_plage_call(c);
    case kLimma: return check_limma_call(c);
    case kCamera: return check_camera_call(c);
    case kSsgseaExact:
      PH_TRY(check_ssgsea_exact_call(c, c.S_out));
      return c.single ? PLAIDHIP_OK : check_gsea_ks_genes(c.g);
    case kGsvaExact: return check_gsva_exact_call(c, ndev);
    case kSingExact: return check_sing_exact_call(c);
    case kUcellExact:
    case kAucellExact: return check_truncated_exact_call(c);
    default: return check_scorer_call(c, ndev, multi);   // (which refuses what is no method at all)
  }
}

int dispatch(const Target& t, Call c) {
  // (the shard count first: check_call reads it.  A null context after the arguments: tests reach the checks without one)
  if (t.kind == Target::kDevices) PH_TRY(check_devices(t.devices, t.ndev));
  if (t.kind == Target::kHook) PH_REQUIRE(t.ndev >= 1 && t.ndev <= 64, "debug_sharded: nshards = %d", t.ndev);
  PH_TRY(check_call(c, t.ndev, t.kind == Target::kDevices));
  if (t.kind == Target::kContext) PH_REQUIRE(t.ctx != nullptr, "null plaidhip_ctx");
  if (c.method == kGseaMultilevel && c.ml_ruler) {
    // (one ruler: no sets to be without)
  } else if (c.method == kPlaidTestContrasts) {
    if (c.m == 0 || c.ncontrast == 0) return PLAIDHIP_OK;
  } else if (c.method == kLimma) {
    if (c.g == 0 || c.nfit == 0 || c.nq == 0) return PLAIDHIP_OK;
  } else if (c.method == kCamera) {
    if (c.g == 0 || c.nfit == 0 || c.nq == 0 || c.m == 0) return PLAIDHIP_OK;
  } else if (c.method == kPlaidTest ? c.m == 0 : (int64_t)c.m * c.n == 0) {
    return PLAIDHIP_OK;
  }
  if (t.kind == Target::kHook) return run_on_one_device(t.device, t.ndev, t.fail_shard, c);
  std::vector<plaidhip_ctx*> ctxs(1, t.ctx);
  if (t.kind == Target::kContext)
    PH_HIP(hipSetDevice(t.ctx->device));
  else
    PH_TRY(multi_contexts(t.devices, t.ndev, ctxs));
  return run_call(ctxs.data(), t.ndev, c);
}

}  // namespace plaidhip

// ---- multi-device entry points (include/plaidhip.h) and the test hooks: build the Call, dispatch ------------------------------
extern "C" {

int plaidhip_multi_set_precision(int mode) try {
  PH_REQUIRE(mode == PLAIDHIP_PRECISION_F64 || mode == PLAIDHIP_PRECISION_MIXED, "multi_set_precision: bad mode %d", mode);
  std::lock_guard<std::mutex> lk(g_multi_mu);
  g_multi_precision = mode;
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_multi_finalize(void) try {
  std::lock_guard<std::mutex> lk(g_multi_mu);
  for (plaidhip_ctx*& c : g_multi_ctx)
    if (c) { plaidhip_finalize(c); c = nullptr; }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// Each plaidhip_*_multi entry; then the test hooks (not part of include/plaidhip.h): the same calls on `nshards` contexts of
// one device (run_on_one_device), so a hook's signature is its entry's with (device, nshards, fail_shard) for (devices,
// ndev).  Two hooks serve several entries by Method ordinal: plaid / sing / ssgsea (0 - 2) and ucell / aucell / scse /
// gsva (3 - 6; the parameters a method does not take are ignored).

int plaidhip_plaid_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                         int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, int stat, int normalize, double* S_out) try {
  PH_REQUIRE(stat == PLAIDHIP_STAT_MEAN || stat == PLAIDHIP_STAT_SUM, "plaid_multi: bad stat %d", stat);
  return dispatch(on_devices(devices, ndev), plaid_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, stat, normalize, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_sing_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const int32_t* Gp,
                        const int32_t* Gi, int32_t m, double* S_out) try {
  return dispatch(on_devices(devices, ndev), sing_call({nullptr, nullptr, X, g, n, Gp, Gi, m}, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_sing_csc_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g,
                            int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out) try {
  PH_REQUIRE(Xp != nullptr, "sing_csc_multi: null Xp");
  return dispatch(on_devices(devices, ndev), sing_call({Xp, Xi, Xx, g, n, Gp, Gi, m}, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_ssgsea_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                          int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, double* S_out) try {
  return dispatch(on_devices(devices, ndev), ssgsea_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_ucell_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                         int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, const double* k_full, double rmax,
                         double* S_out) try {
  return dispatch(on_devices(devices, ndev), ucell_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, k_full, rmax, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_aucell_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                          int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double auc_max_rank, double* S_out) try {
  return dispatch(on_devices(devices, ndev), aucell_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, auc_max_rank, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_scse_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                        int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, int remove_log2, int score_mean,
                        double* S_out, int* removed_log2) try {
  return dispatch(on_devices(devices, ndev),
                  scse_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, remove_log2, score_mean, S_out, removed_log2));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsva_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                        int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf, double* S_out) try {
  return dispatch(on_devices(devices, ndev), gsva_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, tau, rowtf, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plaid_test_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                              int32_t g, int32_t n, const int32_t* y, const int32_t* Gp, const int32_t* Gi, int32_t m,
                              const double* gsetX, int tests, int metap_method, double* out) try {
  return dispatch(on_devices(devices, ndev),
                  plaid_test_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, y, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plaid_test_contrasts_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi,
                                        const double* X_or_x, int32_t g, int32_t n, const int32_t* Y, int32_t C,
                                        const int32_t* Gp, const int32_t* Gi, int32_t m, const double* gsetX, int tests,
                                        int metap_method, double* out) try {
  return dispatch(on_devices(devices, ndev),
                  plaid_test_contrasts_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Y, C, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_ssgsea_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                                int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale,
                                int norm, double* S_out) try {
  return dispatch(on_devices(devices, ndev), ssgsea_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, scale, norm, S_out, 1));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_ssgsea_exact_ks_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                                   int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha,
                                   int scale, int norm, double* S_out) try {
  return dispatch(on_devices(devices, ndev), ssgsea_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, scale, norm, S_out, 0));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsva_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                              int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf,
                              int max_diff, double* S_out) try {
  return dispatch(on_devices(devices, ndev), gsva_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, tau, rowtf, max_diff, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_sing_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                              int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di,
                              int32_t m, int center, double* total, double* up, double* down, double* total_disp,
                              double* up_disp, double* down_disp) try {
  return dispatch(on_devices(devices, ndev), sing_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Dp, Di, center, total, up, down,
                                                             total_disp, up_disp, down_disp));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_sharded_on_one_device(int device, int nshards, int fail_shard, int method, const int32_t* Xp,
                                         const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n, const int32_t* Gp,
                                         const int32_t* Gi, int32_t m, int stat, int normalize, double alpha, double* S_out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  rank_sum_call(method, {Xp, Xi, X_or_x, g, n, Gp, Gi, m}, stat, normalize, alpha, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_scorer_sharded_on_one_device(int device, int nshards, int fail_shard, int method, const int32_t* Xp,
                                                const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                const int32_t* Gp, const int32_t* Gi, int32_t m, const double* k_full,
                                                double rmax, double auc_max_rank, int remove_log2, int score_mean, double tau,
                                                int rowtf, double* S_out, int* removed_log2) try {
  PH_REQUIRE(is_scorer(method), "scorer: bad method %d", method);   // (the ordinal picks the checks: none but these four)
  return dispatch(on_hook(device, nshards, fail_shard),
                  scorer_call(method, {Xp, Xi, X_or_x, g, n, Gp, Gi, m}, k_full, rmax, auc_max_rank, remove_log2, score_mean, tau,
                              rowtf, S_out, removed_log2));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_plaid_test_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                    const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                    const int32_t* y, const int32_t* Gp, const int32_t* Gi, int32_t m,
                                                    const double* gsetX, int tests, int metap_method, double* out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  plaid_test_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, y, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_plaid_test_contrasts_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                              const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                              const int32_t* Y, int32_t C, const int32_t* Gp,
                                                              const int32_t* Gi, int32_t m, const double* gsetX, int tests,
                                                              int metap_method, double* out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  plaid_test_contrasts_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Y, C, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_ssgsea_exact_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                      const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                      const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale,
                                                      int norm, double* S_out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  ssgsea_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, scale, norm, S_out, 1));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_ssgsea_exact_ks_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                         const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                         const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha,
                                                         int scale, int norm, double* S_out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  ssgsea_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, scale, norm, S_out, 0));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_gsva_exact_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                    const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                    const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf,
                                                    int max_diff, double* S_out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  gsva_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, tau, rowtf, max_diff, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_sing_exact_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp, const int32_t* Xi,
                                                    const double* X_or_x, int32_t g, int32_t n, const int32_t* Gp,
                                                    const int32_t* Gi, const int32_t* Dp, const int32_t* Di, int32_t m,
                                                    int center, double* total, double* up, double* down, double* total_disp,
                                                    double* up_disp, double* down_disp) try {
  return dispatch(on_hook(device, nshards, fail_shard), sing_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Dp, Di, center, total,
                                                                         up, down, total_disp, up_disp, down_disp));
} catch (...) { return plaidhip::on_exception(); }

// impute != 0: K = k_full (k_full_down for the down sets), which must be given; impute == 0: they are not read
int plaidhip_ucell_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                               int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di,
                               int32_t m, double max_rank, double w_neg, int impute, const double* k_full,
                               const double* k_full_down, double* total, double* up, double* down) try {
  PH_REQUIRE(!impute || k_full != nullptr || m == 0, "ucell_exact: impute needs k_full");
  return dispatch(on_devices(devices, ndev),
                  ucell_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Dp, Di, max_rank, w_neg, impute ? k_full : nullptr,
                                   impute ? k_full_down : nullptr, total, up, down));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_aucell_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                                int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double auc_max_rank,
                                double* S_out) try {
  return dispatch(on_devices(devices, ndev), aucell_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, auc_max_rank, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_ucell_exact_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                     const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                     const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di,
                                                     int32_t m, double max_rank, double w_neg, int impute, const double* k_full,
                                                     const double* k_full_down, double* total, double* up, double* down) try {
  PH_REQUIRE(!impute || k_full != nullptr || m == 0, "ucell_exact: impute needs k_full");
  return dispatch(on_hook(device, nshards, fail_shard),
                  ucell_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Dp, Di, max_rank, w_neg, impute ? k_full : nullptr,
                                   impute ? k_full_down : nullptr, total, up, down));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_aucell_exact_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                      const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                      const int32_t* Gp, const int32_t* Gi, int32_t m, double auc_max_rank,
                                                      double* S_out) try {
  return dispatch(on_hook(device, nshards, fail_shard), aucell_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, auc_max_rank, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsea_multi(const int* devices, int ndev, const double* stat, const double* weight, int32_t g, int32_t c,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed,
                        double* out, double* null_out) try {
  return dispatch(on_devices(devices, ndev), gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsea_scored_multi(const int* devices, int ndev, const double* stat, const double* weight, int32_t g, int32_t c,
                               const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm,
                               uint64_t seed, int score_type, double* out, double* null_out, int32_t* le_len,
                               int32_t* le_idx) try {
  return dispatch(on_devices(devices, ndev),
                  gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out, score_type, le_len, le_idx));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_gsea_scored_sharded_on_one_device(int device, int nshards, int fail_shard, const double* stat,
                                                     const double* weight, int32_t g, int32_t c, const int32_t* Gp,
                                                     const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm,
                                                     uint64_t seed, int score_type, double* out, double* null_out,
                                                     int32_t* le_len, int32_t* le_idx) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out, score_type, le_len, le_idx));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsea_multilevel_multi(const int* devices, int ndev, const double* stat, const double* weight, int32_t g, int32_t c,
                                   const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm,
                                   uint64_t seed, int score_type, int32_t sample_size, int32_t sweeps, double eps,
                                   int32_t ml_min, double* out, double* null_out, int32_t* le_len, int32_t* le_idx,
                                   double* ml_out) try {
  return dispatch(on_devices(devices, ndev),
                  gsea_multilevel_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, score_type, sample_size, sweeps, eps,
                                       ml_min, out, null_out, le_len, le_idx, ml_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_gsea_multilevel_sharded_on_one_device(int device, int nshards, int fail_shard, const double* stat,
                                                         const double* weight, int32_t g, int32_t c, const int32_t* Gp,
                                                         const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm,
                                                         uint64_t seed, int score_type, int32_t sample_size, int32_t sweeps,
                                                         double eps, int32_t ml_min, double* out, double* null_out,
                                                         int32_t* le_len, int32_t* le_idx, double* ml_out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  gsea_multilevel_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, score_type, sample_size, sweeps, eps,
                                       ml_min, out, null_out, le_len, le_idx, ml_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_fisher_multi(const int* devices, int ndev, const int8_t* sig, int32_t g, int32_t c, const int32_t* Gp,
                          const int32_t* Gi, int32_t m, double* out, double* tot_out, int32_t* ov_len, int32_t* ov_idx) try {
  return dispatch(on_devices(devices, ndev), fisher_call(sig, g, c, Gp, Gi, m, out, tot_out, ov_len, ov_idx));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_multi(const int* devices, int ndev, const double* A, int32_t rows, int32_t n, const double* design,
                         int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q, double* out,
                         double* hyper) try {
  return dispatch(on_devices(devices, ndev), limma_call(A, rows, n, design, p, nfit, use, K, q, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_limma_sharded_on_one_device(int device, int nshards, int fail_shard, const double* A, int32_t rows, int32_t n,
                                               const double* design, int32_t p, int32_t nfit, const int8_t* use, const double* K,
                                               int32_t q, double* out, double* hyper) try {
  return dispatch(on_hook(device, nshards, fail_shard), limma_call(A, rows, n, design, p, nfit, use, K, q, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_na_multi(const int* devices, int ndev, const double* A, int32_t rows, int32_t n, const double* design,
                            int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q, double max_na, double* out,
                            double* hyper, double* dfres) try {
  return dispatch(on_devices(devices, ndev), limma_na_call(A, rows, n, design, p, nfit, use, K, q, max_na, out, hyper, dfres));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_limma_na_sharded_on_one_device(int device, int nshards, int fail_shard, const double* A, int32_t rows,
                                                  int32_t n, const double* design, int32_t p, int32_t nfit, const int8_t* use,
                                                  const double* K, int32_t q, double max_na, double* out, double* hyper,
                                                  double* dfres) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  limma_na_call(A, rows, n, design, p, nfit, use, K, q, max_na, out, hyper, dfres));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_camera_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const double* design, int32_t p,
                          int32_t nfit, const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi,
                          int32_t m, double inter_gene_cor, int allow_neg_cor, double* out, double* hyper) try {
  return dispatch(on_devices(devices, ndev),
                  camera_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, inter_gene_cor, allow_neg_cor, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_camera_sharded_on_one_device(int device, int nshards, int fail_shard, const double* X, int32_t g, int32_t n,
                                                const double* design, int32_t p, int32_t nfit, const int8_t* use,
                                                const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                                                double inter_gene_cor, int allow_neg_cor, double* out, double* hyper) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  camera_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, inter_gene_cor, allow_neg_cor, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_fisher_sharded_on_one_device(int device, int nshards, int fail_shard, const int8_t* sig, int32_t g, int32_t c,
                                                const int32_t* Gp, const int32_t* Gi, int32_t m, double* out, double* tot_out,
                                                int32_t* ov_len, int32_t* ov_idx) try {
  return dispatch(on_hook(device, nshards, fail_shard), fisher_call(sig, g, c, Gp, Gi, m, out, tot_out, ov_len, ov_idx));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_rankcor_multi(const int* devices, int ndev, const double* stat, int32_t g, int32_t c, const int32_t* Gp,
                           const int32_t* Gi, int32_t m, int use_rank, int ties, double* out, double* tot_out) try {
  return dispatch(on_devices(devices, ndev), rankcor_call(stat, g, c, Gp, Gi, m, use_rank, ties, out, tot_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_rankcor_sharded_on_one_device(int device, int nshards, int fail_shard, const double* stat, int32_t g,
                                                 int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m, int use_rank,
                                                 int ties, double* out, double* tot_out) try {
  return dispatch(on_hook(device, nshards, fail_shard), rankcor_call(stat, g, c, Gp, Gi, m, use_rank, ties, out, tot_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plage_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                         int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double tol, int32_t maxit, double* S_out,
                         double* info_out, double* load_out) try {
  return dispatch(on_devices(devices, ndev), plage_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, tol, maxit, S_out, info_out, load_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_zscore_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                          int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out, double* size_out) try {
  return dispatch(on_devices(devices, ndev), zscore_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, S_out, size_out));
} catch (...) { return plaidhip::on_exception(); }

// which Gram kernel replaid.plage launches: 0 the product's (rounded products), 1 the MFMA form
int plaidhip_debug_plage_gram(int mode) try {
  PH_REQUIRE(mode == 0 || mode == 1, "debug_plage_gram: mode = %d", mode);
  plaidhip::debug_plage_set_gram(mode);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// method: kPlage (18) or kZscore (19), which takes no tol / maxit / load_out and the sizes in info_out
int plaidhip_debug_plage_sharded_on_one_device(int device, int nshards, int fail_shard, int method, const int32_t* Xp,
                                               const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n, const int32_t* Gp,
                                               const int32_t* Gi, int32_t m, double tol, int32_t maxit, double* S_out,
                                               double* info_out, double* load_out) try {
  PH_REQUIRE(method == kPlage || method == kZscore, "debug_plage_sharded: method = %d", method);
  const Operands x{Xp, Xi, X_or_x, g, n, Gp, Gi, m};
  return dispatch(on_hook(device, nshards, fail_shard),
                  method == kPlage ? plage_call(x, tol, maxit, S_out, info_out, load_out) : zscore_call(x, S_out, info_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_gsea_sharded_on_one_device(int device, int nshards, int fail_shard, const double* stat, const double* weight,
                                              int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m,
                                              const int32_t* perm, int32_t nperm, uint64_t seed, double* out,
                                              double* null_out) try {
  return dispatch(on_hook(device, nshards, fail_shard), gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out));
} catch (...) { return plaidhip::on_exception(); }

}  // extern "C"
