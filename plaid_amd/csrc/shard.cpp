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
// plain functions, one file per family (shard_*.cpp), over one scaffold (shard.h: Shard -- the columns, `step`, the common
// exit -- and Shared) and the shared blocks of this file (the pinned ring, the CSC upload, the medians' coupling, the
// chained row reductions).  What the engine knows about a method is `route`, below; run_call is: prepare, run the
// threads, report the first failure, tail.  The way in (the checks, dispatch, the entries) is multi.cpp.
//
// Uploads are pipelined: R hands over pageable memory, which the HIP runtime copies at ~21 GB/s; staged through
// pinned buffers by a few feeder threads (memcpy at ~75 GB/s with four threads, tools/ubench/pcie.cpp) the DMA
// runs at the link rate (~57 GB/s) and the kernels of a column panel start as soon as the panel has landed.
#include <sys/mman.h>

#include "shard.h"

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

}  // namespace

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
void merge_range(Shard& s, double mn, double mx, bool any_nan) {
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

namespace {
// Chained, ordered reduction over the samples: in round r only shard r works, continuing shard r - 1's running sums (`run`,
// on the host) block by block with `reduce` (d_seed -> d_run) -- the additions of the one-device call in their order.
// ndev rendezvous.
void chain_sums(Shard& s, std::vector<double>& run, size_t bytes, double* d_seed, double* d_run,
                const std::function<int()>& reduce) {
  plaidhip_ctx* ctx = s.ctx;
  for (int r = 0; r < s.ndev; ++r) {
    if (r == s.k)
      s.step([&]() -> int {
        if (s.nloc == 0) return PLAIDHIP_OK;
        PH_HIP(hipMemcpyAsync(d_seed, run.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        PH_TRY(reduce());
        PH_HIP(hipMemcpyAsync(run.data(), d_run, bytes, hipMemcpyDeviceToHost, ctx->stream));
        PH_HIP(hipStreamSynchronize(ctx->stream));
        return PLAIDHIP_OK;
      });
    s.sh.rv.arrive_and_wait();
  }
}
}  // namespace

// the [nblk][groups][rows] block partials in ws, group by group; run, d_seed, d_run: groups x rows doubles each
void chain_block_sums(Shard& s, std::vector<double>& run, const double* ws, int32_t rows, int groups, double* d_seed,
                      double* d_run) {
  chain_sums(s, run, (size_t)rows * groups * 8, d_seed, d_run, [&]() -> int {
    for (int q = 0; q < groups; ++q)
      PH_TRY(launch_reduce_blocks_seeded(s.ctx, ws + (size_t)q * rows, rows, s.nloc, d_seed + (size_t)q * rows,
                                         d_run + (size_t)q * rows));
    return PLAIDHIP_OK;
  });
}

// any [nblk][len] partials of the shard's columns at once (launch_reduce_blocks_flat); run, d_seed, d_run: len doubles each
void chain_flat_sums(Shard& s, std::vector<double>& run, const double* ws, int64_t len, double* d_seed, double* d_run) {
  chain_sums(s, run, (size_t)len * 8, d_seed, d_run,
             [&]() -> int { return launch_reduce_blocks_flat(s.ctx, ws, len, s.nloc, d_seed, d_run); });
}

namespace {
bool no_scores(const Call& c) { return (int64_t)c.m * c.n == 0; }
}  // namespace

// What the engine knows about a method on the run side, in one place (the argument checks are check_call's, multi.cpp).
// No default label: the compiler names a method that is missing here.  block_cut: dense replaid.gsva (and replaid.gsva.exact
// with its z transform), plaid.test (dense or not: its score rows are chained too), plaid.limma and plaid.camera chain row
// reductions over the samples.
Route route(const Call& c) {
  switch ((Method)c.method) {
    case kPlaid: case kSing: case kSsgsea: return {false, no_scores, nullptr, shard_worker, nullptr};
    case kUcell: case kAucell: return {false, no_scores, nullptr, scorer_worker, nullptr};
    case kScse: return {false, no_scores, nullptr, scorer_worker, scse_tail};
    case kGsva: return {c.Xp == nullptr, no_scores, gsva_prepare, scorer_worker, nullptr};
    case kGsvaExact: return {c.rowtf == 0 && c.Xp == nullptr, no_scores, gsva_prepare, scorer_worker, nullptr};
    case kSsgseaExact: return {false, no_scores, nullptr, ssgsea_exact_worker, nullptr};
    case kSingExact: return {false, no_scores, nullptr, sing_exact_worker, nullptr};
    case kUcellExact: case kAucellExact: return {false, no_scores, nullptr, truncated_exact_worker, nullptr};
    case kPlaidTest: case kPlaidTestContrasts: return {true, plaid_test_empty, plaid_test_prepare, plaid_test_worker, plaid_test_tail};
    case kGsea: return {false, no_scores, gsea_prepare, gsea_worker, nullptr};
    case kGseaMultilevel:   // (one ruler: no sets to be without)
      if (c.ml_ruler) return {false, [](const Call&) { return false; }, nullptr, gsea_ruler_worker, nullptr};
      return {false, no_scores, gsea_prepare, gsea_worker, nullptr};
    case kFisher: return {false, no_scores, nullptr, fisher_worker, nullptr};
    case kRankcor: return {false, no_scores, nullptr, rankcor_worker, nullptr};
    case kPlage: case kZscore: return {false, no_scores, nullptr, plage_worker, nullptr};
    case kLimma: return {true, limma_empty, limma_prepare, c.weighted ? limma_w_worker : limma_worker, limma_tail};
    case kCamera: return {true, limma_empty, limma_prepare, limma_worker, camera_tail};
    case kFry: return {true, limma_empty, limma_prepare, limma_worker, fry_tail};
    case kRoast: return {false, limma_empty, roast_prepare, roast_worker, roast_tail};
    case kRomer: return {false, limma_empty, romer_prepare, romer_worker, romer_tail};
    case kVoom: return {true, voom_empty, voom_prepare, voom_worker, nullptr};
  }
  return {false, no_scores, nullptr, nullptr, nullptr};   // (no method at all: check_call has refused it)
}

void shard_columns(const Call& c, int ndev, int k, int32_t* lo, int32_t* nloc) {
  int64_t lo64 = 0, hi64 = 0;
  if (route(c).block_cut) {
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

int run_call(plaidhip_ctx* const* ctxs, int ndev, const Call& c) {
  Shared sh(ndev);
  sh.med_all.assign((size_t)c.n, 0.0);
  const Route r = route(c);
  PH_REQUIRE(r.worker != nullptr, "run_call: bad method %d", c.method);
  if (r.prepare) r.prepare(sh, c, ndev);
  auto worker = [&](int k) { return r.worker(ctxs[k], c, ndev, k, sh); };
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
  if (rc == PLAIDHIP_OK && r.tail) rc = r.tail(ctxs[0], c, sh);
  return rc;
}

}  // namespace plaidhip
