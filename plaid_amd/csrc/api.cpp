// C-ABI entry points (include/plaidhip.h): context lifecycle, device-level wrappers and the
// host-buffer pipelines the R `.Call` shim binds.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include <algorithm>
#include <limits>
#include <vector>

#include "call.h"
#include "roast.h"
#include "romer.h"

namespace plaidhip {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

const char* last_error_cstr() { return g_err; }

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  set_error("HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
  return (e == hipErrorOutOfMemory) ? PLAIDHIP_ENOMEM : PLAIDHIP_EHIP;
}

int ensure_workspace(plaidhip_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->ws_bytes) return PLAIDHIP_OK;
  if (ctx->ws) {
    PH_HIP(hipStreamSynchronize(ctx->stream));
    PH_HIP(hipFree(ctx->ws));
    ctx->ws = nullptr;
    ctx->ws_bytes = 0;
    ctx->rank_fb_count[0] = nullptr;   // (the bucket ranker's hand-over counter lived there)
  }
  bytes = (bytes + 4095) & ~(size_t)4095;
  PH_HIP(hipMalloc(&ctx->ws, bytes));
  ctx->ws_bytes = bytes;
  return PLAIDHIP_OK;
}

int32_t host_max_col_nnz(const int32_t* Xp, int32_t n) {
  int32_t mx = 0;
  for (int32_t c = 0; c < n; ++c) mx = std::max(mx, Xp[c + 1] - Xp[c]);
  return mx;
}

int ctx_buffer(plaidhip_ctx* ctx, int k, size_t bytes, void** out) {
  if (bytes < 256) bytes = 256;
  if (ctx->hbuf_bytes[k] < bytes) {
    if (ctx->hbuf[k]) {
      PH_HIP(hipStreamSynchronize(ctx->stream));
      PH_HIP(hipFree(ctx->hbuf[k]));
      ctx->hbuf[k] = nullptr;
      ctx->hbuf_bytes[k] = 0;
    }
    const size_t want = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    PH_HIP(hipMalloc(&ctx->hbuf[k], want));
    ctx->hbuf_bytes[k] = want;
  }
  *out = ctx->hbuf[k];
  return PLAIDHIP_OK;
}

int allow_full_lds(plaidhip_ctx* ctx, const void* kernel, std::atomic<uint32_t>* done_mask) {
  if (ctx->device >= 32) {   // no bit for it: set the attribute every time (idempotent)
    PH_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    return PLAIDHIP_OK;
  }
  const uint32_t bit = 1u << ctx->device;
  if (done_mask->load(std::memory_order_acquire) & bit) return PLAIDHIP_OK;
  PH_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
  done_mask->fetch_or(bit, std::memory_order_release);
  return PLAIDHIP_OK;
}

}  // namespace plaidhip

using namespace plaidhip;

#define PH_CTX(ctx)                                   \
  PH_REQUIRE((ctx) != nullptr, "null plaidhip_ctx");  \
  PH_HIP(hipSetDevice((ctx)->device))

#define PH_TRY(expr)                      \
  do {                                    \
    int rc_ = (expr);                     \
    if (rc_ != PLAIDHIP_OK) return rc_;   \
  } while (0)

namespace plaidhip {
int DevBuf::alloc(size_t bytes) {
  hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
  if (e != hipSuccess) { p = nullptr; return hip_fail(e, "hipMalloc", __FILE__, __LINE__); }
  return PLAIDHIP_OK;
}
}  // namespace plaidhip

namespace {

// The host-level entry points prepare the gene-set collection themselves.  An R session calls them again and
// again with the same matG, so the last few prepared collections stay in the context (keyed by sizes and a hash
// of the pattern) instead of being rebuilt: preparing C2's 5,000 sets costs ~20 ms of a 76 ms call (acquire_geneset).

// two independent 64-bit hashes over the int32 words of the pattern (a 128-bit key; it only ever lives in this process).
// Two ids per step and four interleaved lanes per hash: one multiply chain is latency-bound at ~1.4 ns per id (7.5 ms of
// every call for the 5.2e6 ids of a 61,459-set collection), four chains side by side fill the multiplier.
void hash_words(const int32_t* w, size_t count, uint64_t& h1, uint64_t& h2) {
  uint64_t a[4], b[4];
  for (int l = 0; l < 4; ++l) {
    a[l] = h1 + (uint64_t)l * 0x9e3779b97f4a7c15ull;
    b[l] = h2 ^ ((uint64_t)(l + 1) * 0xd6e8feb86659fd93ull);
  }
  size_t i = 0;
  for (; i + 8 <= count; i += 8)
    for (int l = 0; l < 4; ++l) {
      uint64_t v;
      memcpy(&v, w + i + 2 * l, 8);
      a[l] = (a[l] ^ v) * 0x100000001b3ull;
      a[l] ^= a[l] >> 29;
      b[l] = (b[l] + v + 0x9e3779b97f4a7c15ull) * 0xbf58476d1ce4e5b9ull;
      b[l] ^= b[l] >> 31;
    }
  for (; i < count; ++i) {   // the last words, with their position
    const uint64_t v = ((uint64_t)(uint32_t)w[i] << 3) | (uint64_t)(i & 7);
    a[0] = (a[0] ^ v) * 0x100000001b3ull;
    a[0] ^= a[0] >> 29;
    b[0] = (b[0] + v + 0x9e3779b97f4a7c15ull) * 0xbf58476d1ce4e5b9ull;
    b[0] ^= b[0] >> 31;
  }
  h1 = count;
  h2 = ~(uint64_t)count;
  for (int l = 0; l < 4; ++l) {
    h1 = (h1 ^ a[l]) * 0x94d049bb133111ebull;
    h1 ^= h1 >> 32;
    h2 = (h2 + b[l]) * 0xff51afd7ed558ccdull;
    h2 ^= h2 >> 33;
  }
}

}  // namespace
namespace plaidhip {
int acquire_geneset(plaidhip_ctx* ctx, int32_t g, int32_t m, const int32_t* Gp, const int32_t* Gi, plaidhip_geneset** out) {
  *out = nullptr;
  uint64_t h = 1469598103934665603ull, h2 = 0x243f6a8885a308d3ull;
  if (Gp != nullptr && m >= 0) {
    hash_words(Gp, (size_t)m + 1, h, h2);
    const int64_t z = m > 0 ? Gp[m] : 0;
    if (Gi != nullptr && z > 0) hash_words(Gi, (size_t)z, h, h2);
  }
  for (size_t k = 0; k < ctx->gs_cache.size(); ++k) {
    plaidhip_ctx::cached_geneset& e = ctx->gs_cache[k];
    if (e.hash == h && e.hash2 == h2 && e.g == g && e.m == m) {
      plaidhip_ctx::cached_geneset hit = e;
      ctx->gs_cache.erase(ctx->gs_cache.begin() + (long)k);
      ctx->gs_cache.push_back(hit);   // most recently used last
      *out = hit.gs;
      return PLAIDHIP_OK;
    }
  }
  plaidhip_geneset* gs = nullptr;
  PH_TRY(plaidhip_geneset_create(ctx, g, m, Gp, Gi, &gs));
  if (ctx->gs_cache.size() >= 4) {
    plaidhip_geneset_destroy(ctx->gs_cache.front().gs);
    ctx->gs_cache.erase(ctx->gs_cache.begin());
  }
  ctx->gs_cache.push_back(plaidhip_ctx::cached_geneset{h, h2, g, m, gs});
  *out = gs;
  return PLAIDHIP_OK;
}
}  // namespace plaidhip
namespace {

// (pageable memory: through the pinned staging ring once it is worth it, shard.cpp)
int h2d(plaidhip_ctx* ctx, void* dst, const void* src, size_t bytes) {
  return upload_host(ctx, dst, 1, src, 1, (int64_t)bytes);
}

// normalize_medians on a device-resident S (R/plaid.R:554-575), fully enqueued: ignore.zero is
// resolved on the device from the flag words, mean(medx) from the {sum, count} pair.
int normalize_on_device(plaidhip_ctx* ctx, double* dS, int32_t m, int32_t n, int ignore_zero,
                        uint32_t* d_flags, bool have_flags, double* d_med, double* d_red) {
  if (ignore_zero == PLAIDHIP_IGNORE_ZERO_AUTO && !have_flags) {
    PH_HIP(hipMemsetAsync(d_flags, 0, 4 * sizeof(uint32_t), ctx->stream));
    PH_TRY(launch_minflags(ctx, dS, (int64_t)m * n, d_flags));
  }
  PH_TRY(launch_col_medians(ctx, dS, m, m, n, ignore_zero, d_flags, d_med));
  PH_TRY(launch_sum(ctx, d_med, n, d_red));
  PH_TRY(launch_shift_columns(ctx, dS, m, m, n, d_med, 0.0, d_red));
  return PLAIDHIP_OK;
}

}  // namespace
namespace plaidhip {
// dgCMatrix slots handed over by a host language: @p non-decreasing from 0, @i inside [0, g)
int check_host_csc(const int32_t* Xp, const int32_t* Xi, int32_t g, int32_t n) {
  PH_REQUIRE(Xp != nullptr, "null Xp");
  PH_REQUIRE(Xp[0] == 0, "Xp[0] = %d, expected 0", Xp[0]);
  for (int32_t c = 0; c < n; ++c)
    PH_REQUIRE(Xp[c + 1] >= Xp[c], "Xp decreases at column %d (more than 2^31-1 stored values? split the matrix by columns)", c);
  if (Xi != nullptr) {
    const int64_t zx = Xp[n];
    for (int64_t q = 0; q < zx; ++q)
      PH_REQUIRE(Xi[q] >= 0 && Xi[q] < g, "Xi[%lld] = %d outside [0, %d)", (long long)q, Xi[q], g);
  }
  return PLAIDHIP_OK;
}

int check_host_common(const void* G_p, int32_t g, int32_t n, int32_t m) {
  PH_REQUIRE(g > 0 && n >= 0 && m >= 0, "bad dims g=%d n=%d m=%d", g, n, m);
  PH_REQUIRE(G_p != nullptr, "null Gp");
  return PLAIDHIP_OK;
}
}  // namespace plaidhip
extern "C" {

int plaidhip_version(void) { return PLAIDHIP_VERSION; }

int plaidhip_set_precision(plaidhip_ctx* ctx, int mode) try {
  PH_CTX(ctx);
  PH_REQUIRE(mode == PLAIDHIP_PRECISION_F64 || mode == PLAIDHIP_PRECISION_MIXED, "set_precision: unknown mode %d", mode);
  ctx->precision = mode;
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_set_stream(plaidhip_ctx* ctx, void* stream) try {
  PH_CTX(ctx);
  PH_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->own_stream) PH_HIP(hipStreamDestroy(ctx->stream));
  ctx->stream = reinterpret_cast<hipStream_t>(stream);   // nullptr: the null stream
  ctx->own_stream = false;
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_set_option(plaidhip_ctx* ctx, int option, int value) try {
  PH_CTX(ctx);
  switch (option) {
    case PLAIDHIP_OPT_SPMM_DENSE_KERNEL:
      PH_REQUIRE(value >= 0 && value <= 4, "set_option: dense kernel %d (0 auto, 1 one-column, 2 pair, 3 mfma, 4 auto with the pair kernel's scratch form)", value);
      ctx->opt_dense_kernel = value;
      break;
    case PLAIDHIP_OPT_SPMM_SPARSE_KERNEL:
      PH_REQUIRE(value >= 0 && value <= 2, "set_option: sparse kernel %d (0 auto, 1 scatter, 2 gather)", value);
      ctx->opt_sparse_kernel = value;
      break;
    case PLAIDHIP_OPT_NT_STORE:
      PH_REQUIRE(value >= -1 && value <= 1, "set_option: nt_store %d (-1 auto, 0, 1)", value);
      ctx->opt_nt_store = value;
      break;
    case PLAIDHIP_OPT_RANKS_F32:
      PH_REQUIRE(value >= 0 && value <= 2, "set_option: ranks_f32 %d (0 fp64, 1 fp32 staging, 2 u16 staging)", value);
      ctx->opt_ranks_f32 = value;
      break;
    case PLAIDHIP_OPT_SCATTER_FIXED:
      PH_REQUIRE(value == 0 || value == 1, "set_option: scatter_fixed %d (0, 1)", value);
      ctx->opt_scatter_fixed = value;
      break;
    case PLAIDHIP_OPT_SCATTER_ORDER:
      PH_REQUIRE(value == 0 || value == 1, "set_option: scatter_order %d (0 column-major, 1 chunk-major)", value);
      ctx->opt_scatter_order = value;
      break;
    case PLAIDHIP_OPT_FUSED_MEDIANS:
      PH_REQUIRE(value >= 0 && value <= 2, "set_option: fused_medians %d (0 by size, 1 whenever possible, 2 never)", value);
      ctx->opt_fused_medians = value;
      break;
    case PLAIDHIP_OPT_RANK_KERNEL:
      PH_REQUIRE(value >= 0 && value <= 3, "set_option: rank kernel %d (0 auto, 1 network, 2 bucket, 3 bucket with 512 x 40 for long columns)", value);
      ctx->opt_rank_kernel = value;
      break;
    default:
      PH_REQUIRE(false, "set_option: unknown option %d", option);
  }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

#ifdef PLAIDHIP_DIAG
int plaidhip_debug_set_ablation(int mode, void* dbg) { debug_set_ablation(mode, dbg); return PLAIDHIP_OK; }
int plaidhip_debug_set_rank_stamps(void* dbg) { debug_set_rank_stamps(dbg); return PLAIDHIP_OK; }
int plaidhip_debug_set_median_stamps(void* dbg) { debug_set_median_stamps(dbg); return PLAIDHIP_OK; }
#endif

const char* plaidhip_last_error_string(void) { return g_err; }

int plaidhip_device_count(int* count) try {
  PH_REQUIRE(count != nullptr, "device_count: null out pointer");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return hip_fail(e, "hipGetDeviceCount", __FILE__, __LINE__);
  }
  *count = n;
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_init(int device, void* stream, plaidhip_ctx** out) try {
  PH_REQUIRE(out != nullptr, "init: null out pointer");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    set_error("no HIP device visible (this library has no CPU path)");
    return PLAIDHIP_ENODEVICE;
  }
  PH_REQUIRE(device >= 0 && device < n, "init: device %d out of range [0,%d)", device, n);
  PH_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  PH_HIP(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    set_error("device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    return PLAIDHIP_ENODEVICE;
  }
  auto* ctx = new (std::nothrow) plaidhip_ctx();
  if (!ctx) { set_error("out of host memory"); return PLAIDHIP_ENOMEM; }
  ctx->device = device;
  ctx->num_cu = prop.multiProcessorCount;
  if (stream) {
    ctx->stream = reinterpret_cast<hipStream_t>(stream);
    ctx->own_stream = false;
  } else {
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete ctx; return hip_fail(e, "hipStreamCreate", __FILE__, __LINE__); }
    ctx->own_stream = true;
  }
  {
    void* sel = nullptr;   // two doubles the sparse crossprod decides its accumulator format from (allocated here: a launch
                           // inside a stream capture must not allocate)
    hipError_t e = hipMalloc(&sel, 128);
    if (e == hipSuccess) e = hipMemset(sel, 0, 128);
    // bytes 96..127: the EMPTY median bracket {offset 0, half width -1, ignore-zero 0} of a calibration launch (no score is a
    // candidate), written once here so that no launch needs a host-to-device copy
    static const double kEmptyBracket[4] = {0.0, -1.0, 0.0, 0.0};
    if (e == hipSuccess) e = hipMemcpy(static_cast<char*>(sel) + 96, kEmptyBracket, 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      if (ctx->own_stream) hipStreamDestroy(ctx->stream);
      delete ctx;
      return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
    }
    ctx->d_sel = static_cast<double*>(sel);
    ctx->d_spec = reinterpret_cast<uint32_t*>(static_cast<char*>(sel) + 64);
  }
  *out = ctx;
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limit(int which, int64_t* value) try {
  PH_REQUIRE(value != nullptr, "limit: null value");
  switch (which) {
    case PLAIDHIP_LIMIT_SPARSE_RANK_COLUMN: *value = max_sparse_rank_column(); return PLAIDHIP_OK;
    case PLAIDHIP_LIMIT_LDS_GENES: *value = kMaxLdsGenes; return PLAIDHIP_OK;
    default: set_error("limit: unknown id %d", which); return PLAIDHIP_EINVAL;
  }
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_finalize(plaidhip_ctx* ctx) try {
  if (!ctx) return PLAIDHIP_OK;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  for (plaidhip_ctx::cached_geneset& e : ctx->gs_cache) plaidhip_geneset_destroy(e.gs);
  ctx->gs_cache.clear();
  if (ctx->ws) hipFree(ctx->ws);
  if (ctx->rank_scratch) hipFree(ctx->rank_scratch);
  if (ctx->tie_scratch) hipFree(ctx->tie_scratch);
  if (ctx->kcdf_table) hipFree(ctx->kcdf_table);
  if (ctx->fmed_buf) hipFree(ctx->fmed_buf);
  if (ctx->d_sel) hipFree(ctx->d_sel);
  for (int k = 0; k < plaidhip_ctx::kHostBufs; ++k)
    if (ctx->hbuf[k]) hipFree(ctx->hbuf[k]);
  for (int t = 0; t < plaidhip_ctx::kFeeders; ++t) {
    for (int b = 0; b < 2; ++b)
      if (ctx->pin[t][b]) hipHostFree(ctx->pin[t][b]);
    if (ctx->copy_stream[t]) hipStreamDestroy(ctx->copy_stream[t]);
  }
  if (ctx->own_stream) hipStreamDestroy(ctx->stream);
  delete ctx;
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_synchronize(plaidhip_ctx* ctx) try {
  PH_CTX(ctx);
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_malloc(plaidhip_ctx* ctx, size_t bytes, void** dptr) try {
  PH_CTX(ctx);
  PH_REQUIRE(dptr != nullptr, "malloc: null out pointer");
  PH_HIP(hipMalloc(dptr, bytes ? bytes : 16));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_free(plaidhip_ctx* ctx, void* dptr) try {
  PH_CTX(ctx);
  if (dptr) PH_HIP(hipFree(dptr));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_memcpy_h2d(plaidhip_ctx* ctx, void* dst, const void* src, size_t bytes) try {
  PH_CTX(ctx);
  if (bytes) PH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_memcpy_d2h(plaidhip_ctx* ctx, void* dst, const void* src, size_t bytes) try {
  PH_CTX(ctx);
  if (bytes) PH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// ---- device-level ---------------------------------------------------------------------

int plaidhip_dev_spmm_dense_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* X,
                                int64_t ldx, int32_t n, int stat, double alpha, const void* alpha_div,
                                double beta, void* S, int64_t lds, void* flags) try {
  PH_CTX(ctx);
  PH_REQUIRE(gs != nullptr, "spmm: null geneset");
  PH_REQUIRE(n >= 0, "spmm: n=%d", n);
  PH_REQUIRE(n == 0 || (X != nullptr && S != nullptr), "spmm: null X/S");
  PH_REQUIRE(ldx >= gs->g && lds >= gs->m, "spmm: leading dims ldx=%lld (g=%d) lds=%lld (m=%d)",
             (long long)ldx, gs->g, (long long)lds, gs->m);
  PH_REQUIRE(stat == PLAIDHIP_STAT_MEAN || stat == PLAIDHIP_STAT_SUM, "spmm: bad stat %d", stat);
  return launch_spmm_dense_f64(ctx, gs, static_cast<const double*>(X), ldx, n, stat, alpha,
                               static_cast<const double*>(alpha_div), beta, static_cast<double*>(S), lds,
                               static_cast<uint32_t*>(flags));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_spmm_dense_fused_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* X,
                                      int64_t ldx, int32_t n, int stat, double alpha, const void* alpha_div,
                                      double beta, void* S, int64_t lds, void* flags) try {
  PH_CTX(ctx);
  PH_REQUIRE(gs != nullptr, "spmm_dense_fused: null geneset");
  PH_REQUIRE(n >= 0, "spmm_dense_fused: n=%d", n);
  PH_REQUIRE(n == 0 || (X != nullptr && S != nullptr), "spmm_dense_fused: null X/S");
  PH_REQUIRE(ldx >= gs->g && lds >= gs->m, "spmm_dense_fused: leading dims ldx=%lld (g=%d) lds=%lld (m=%d)",
             (long long)ldx, gs->g, (long long)lds, gs->m);
  PH_REQUIRE(stat == PLAIDHIP_STAT_MEAN || stat == PLAIDHIP_STAT_SUM, "spmm_dense_fused: bad stat %d", stat);
  return launch_spmm_dense_fused_f64(ctx, gs, static_cast<const double*>(X), ldx, n, stat, alpha,
                                     static_cast<const double*>(alpha_div), beta, static_cast<double*>(S), lds,
                                     static_cast<uint32_t*>(flags));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_spmm_ranks_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* R,
                                int64_t ldr, int32_t n, int stat, double alpha, const void* alpha_div,
                                double beta, void* S, int64_t lds, void* flags) try {
  PH_CTX(ctx);
  PH_REQUIRE(gs != nullptr, "spmm_ranks: null geneset");
  PH_REQUIRE(n >= 0, "spmm_ranks: n=%d", n);
  PH_REQUIRE(n == 0 || (R != nullptr && S != nullptr), "spmm_ranks: null R/S");
  PH_REQUIRE(ldr >= gs->g && lds >= gs->m, "spmm_ranks: leading dims ldr=%lld (g=%d) lds=%lld (m=%d)",
             (long long)ldr, gs->g, (long long)lds, gs->m);
  PH_REQUIRE(stat == PLAIDHIP_STAT_MEAN || stat == PLAIDHIP_STAT_SUM, "spmm_ranks: bad stat %d", stat);
  return launch_spmm_dense_f64(ctx, gs, static_cast<const double*>(R), ldr, n, stat, alpha,
                               static_cast<const double*>(alpha_div), beta, static_cast<double*>(S), lds,
                               static_cast<uint32_t*>(flags), PLAIDHIP_X_RANKS);
} catch (...) { return plaidhip::on_exception(); }

// Test hook (not part of include/plaidhip.h), read-only: did the last speculative launch of this context (the u16 quad
// kernel of plaidhip_dev_spmm_ranks_f64 and of the rank-valued scorers) meet a value that is not a rank, so that the fp64
// kernel enqueued behind it recomputed the scores?  *out = 1 if so, 0 if the u16 scores stand (or no speculative launch
// has run).  Waits for the context's stream, then compares the generation word the kernel leaves with the host's.
int plaidhip_debug_spec_fell_back(plaidhip_ctx* ctx, int* out) try {
  PH_CTX(ctx);
  PH_REQUIRE(out != nullptr, "debug_spec_fell_back: null out");
  *out = 0;
  if (ctx->d_spec == nullptr || ctx->spec_gen == 0u) return PLAIDHIP_OK;
  uint32_t seen = 0;
  PH_HIP(hipMemcpyAsync(&seen, ctx->d_spec, sizeof(seen), hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  *out = seen == ctx->spec_gen ? 1 : 0;
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// Test hook (not part of include/plaidhip.h), read-only: how many columns did the last rank launch of this context hand to
// the sorting network?  out[0]: the bucket ranker (launch_ranks: columns with a mixed fine bucket of more than 256 keys),
// out[1]: the value-partitioned ranker (launch_colranks_partitioned: columns with an open interval of more than 20,352
// keys); -1 where that launcher has not run with a hand-over list (the sorting network ranked everything, nothing was
// ranked, or the buffer that held the word has been released since).  Waits for the context's stream and reads the device
// words the launch left; meant to be called directly after the launch (other kernels reuse the workspace the first word
// lives in).  A partitioned launch ranks its segments with launch_ranks, but its own sorting-network pass reuses that
// workspace: out[0] is -1 after it.
int plaidhip_debug_rank_fallbacks(plaidhip_ctx* ctx, int32_t* out) try {
  PH_CTX(ctx);
  PH_REQUIRE(out != nullptr, "debug_rank_fallbacks: null out");
  for (int k = 0; k < 2; ++k) {
    out[k] = -1;
    if (ctx->rank_fb_count[k] != nullptr)
      PH_HIP(hipMemcpyAsync(&out[k], ctx->rank_fb_count[k], sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_spmm_csc_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* Xp,
                              const void* Xi, const void* Xx, int32_t n, int64_t nnz, int stat, double alpha,
                              const void* alpha_div, double beta, void* S, int64_t lds, void* flags) try {
  PH_CTX(ctx);
  PH_REQUIRE(gs != nullptr, "spmm_csc: null geneset");
  PH_REQUIRE(n >= 0, "spmm_csc: n=%d", n);
  PH_REQUIRE(n == 0 || (Xp != nullptr && S != nullptr), "spmm_csc: null Xp/S");
  PH_REQUIRE(lds >= gs->m, "spmm_csc: lds=%lld < m=%d", (long long)lds, gs->m);
  PH_REQUIRE(stat == PLAIDHIP_STAT_MEAN || stat == PLAIDHIP_STAT_SUM, "spmm_csc: bad stat %d", stat);
  return launch_spmm_csc_f64(ctx, gs, static_cast<const int32_t*>(Xp), static_cast<const int32_t*>(Xi),
                             static_cast<const double*>(Xx), n, nnz, stat, alpha,
                             static_cast<const double*>(alpha_div), beta, static_cast<double*>(S), lds,
                             static_cast<uint32_t*>(flags));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_crossprod_weighted_f64(plaidhip_ctx* ctx, const void* Wp, const void* Wi, const void* Wx, int32_t g,
                                        int32_t m, const void* Y, int64_t ldy, int32_t n, void* S, int64_t lds) try {
  PH_CTX(ctx);
  PH_REQUIRE(g > 0 && m >= 0 && n >= 0, "crossprod_weighted: bad dims g=%d m=%d n=%d", g, m, n);
  PH_REQUIRE(Wp != nullptr, "crossprod_weighted: null x@p");
  PH_REQUIRE((int64_t)m * n == 0 || (Y != nullptr && S != nullptr), "crossprod_weighted: null y/S");
  PH_REQUIRE(ldy >= g && lds >= m, "crossprod_weighted: leading dims ldy=%lld (g=%d) lds=%lld (m=%d)", (long long)ldy, g,
             (long long)lds, m);
  return launch_crossprod_weighted_f64(ctx, static_cast<const int32_t*>(Wp), static_cast<const int32_t*>(Wi),
                                       static_cast<const double*>(Wx), g, m, static_cast<const double*>(Y), ldy, nullptr,
                                       nullptr, nullptr, n, static_cast<double*>(S), lds);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_crossprod_weighted_csc_f64(plaidhip_ctx* ctx, const void* Wp, const void* Wi, const void* Wx, int32_t g,
                                            int32_t m, const void* Yp, const void* Yi, const void* Yx, int32_t n,
                                            void* S, int64_t lds) try {
  PH_CTX(ctx);
  PH_REQUIRE(g > 0 && m >= 0 && n >= 0, "crossprod_weighted_csc: bad dims g=%d m=%d n=%d", g, m, n);
  PH_REQUIRE(Wp != nullptr, "crossprod_weighted_csc: null x@p");
  PH_REQUIRE((int64_t)m * n == 0 || (Yp != nullptr && S != nullptr), "crossprod_weighted_csc: null y@p/S");
  PH_REQUIRE(lds >= m, "crossprod_weighted_csc: lds=%lld < m=%d", (long long)lds, m);
  return launch_crossprod_weighted_f64(ctx, static_cast<const int32_t*>(Wp), static_cast<const int32_t*>(Wi),
                                       static_cast<const double*>(Wx), g, m, nullptr, 0, static_cast<const int32_t*>(Yp),
                                       static_cast<const int32_t*>(Yi), static_cast<const double*>(Yx), n,
                                       static_cast<double*>(S), lds);
} catch (...) { return plaidhip::on_exception(); }

// which: 0 dense columns (matrixStats::colRanks: average / min / max / first / last / dense), 1 the stored values of a
// dgCMatrix (base::rank, R/plaid.R:639-642: no "dense"), 2 a dgCMatrix with its zeros ranked (sparseMatrixStats::colRanks,
// R/plaid.R:605-608: max / average / min only).  "random" is legal in R and refused here: its result is not a function of
// the input.  first / last / dense come without the fused power and column maximum (no caller of the reference combines them).
static int check_ties(int ties, int which = 0, double power = 1.0, const void* colmax = nullptr) {
  if (ties == PLAIDHIP_TIES_RANDOM) {
    set_error("colranks: ties.method = \"random\" is not supported (the ranks would not be reproducible)");
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(ties >= PLAIDHIP_TIES_AVERAGE && ties <= PLAIDHIP_TIES_DENSE, "colranks: unknown ties.method code %d", ties);
  if (ties >= PLAIDHIP_TIES_FIRST) {
    PH_REQUIRE(which != 2, "colranks: 'arg' should be one of \"max\", \"average\", \"min\" for a sparse matrix whose zeros are "
               "ranked (sparseMatrixStats::colRanks, R/plaid.R:605-608)");
    PH_REQUIRE(!(which == 1 && ties == PLAIDHIP_TIES_DENSE), "sparse_colranks: 'arg' should be one of \"average\", \"first\", \"last\", "
               "\"random\", \"max\", \"min\" (base::rank, R/plaid.R:639-642)");
    PH_REQUIRE(power == 1.0 && colmax == nullptr, "colranks: ties.method first / last / dense come without power / colmax");
  }
  return PLAIDHIP_OK;
}

int plaidhip_dev_spmm_csc_ranks_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* Xp,
                                    const void* Xi, const void* Rx, int32_t n, int64_t nnz, int stat, double alpha,
                                    const void* rmax, double beta, void* S, int64_t lds, void* flags) try {
  PH_CTX(ctx);
  PH_REQUIRE(gs != nullptr, "spmm_csc_ranks: null geneset");
  PH_REQUIRE(n >= 0, "spmm_csc_ranks: n=%d", n);
  PH_REQUIRE(n == 0 || (Xp != nullptr && S != nullptr), "spmm_csc_ranks: null Xp/S");
  PH_REQUIRE(rmax != nullptr, "spmm_csc_ranks: rmax (device double: the maximum of Rx) is required");
  PH_REQUIRE(lds >= gs->m, "spmm_csc_ranks: lds=%lld < m=%d", (long long)lds, gs->m);
  PH_REQUIRE(stat == PLAIDHIP_STAT_MEAN || stat == PLAIDHIP_STAT_SUM, "spmm_csc_ranks: bad stat %d", stat);
  return launch_spmm_csc_f64(ctx, gs, static_cast<const int32_t*>(Xp), static_cast<const int32_t*>(Xi),
                             static_cast<const double*>(Rx), n, nnz, stat, alpha, static_cast<const double*>(rmax), beta,
                             static_cast<double*>(S), lds, static_cast<uint32_t*>(flags), /*bounded=*/true,
                             static_cast<const double*>(rmax), 0.0);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_spmm_csc_fused_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* Xp, const void* Xi,
                                    const void* Xx, int32_t n, int64_t nnz, int stat, double alpha, const void* alpha_div,
                                    double beta, void* S, int64_t lds, void* flags, const void* rmax) try {
  PH_CTX(ctx);
  PH_REQUIRE(gs != nullptr, "spmm_csc_fused: null geneset");
  PH_REQUIRE(n >= 0, "spmm_csc_fused: n=%d", n);
  PH_REQUIRE(n == 0 || (Xp != nullptr && S != nullptr), "spmm_csc_fused: null Xp/S");
  PH_REQUIRE(lds >= gs->m, "spmm_csc_fused: lds=%lld < m=%d", (long long)lds, gs->m);
  PH_REQUIRE(stat == PLAIDHIP_STAT_MEAN || stat == PLAIDHIP_STAT_SUM, "spmm_csc_fused: bad stat %d", stat);
  PH_REQUIRE(rmax == nullptr || alpha_div == nullptr || alpha_div == rmax, "spmm_csc_fused: rmax and alpha_div differ");
  const double* div = static_cast<const double*>(rmax != nullptr ? rmax : alpha_div);
  return launch_spmm_csc_fused_f64(ctx, gs, static_cast<const int32_t*>(Xp), static_cast<const int32_t*>(Xi),
                                   static_cast<const double*>(Xx), n, nnz, stat, alpha, div, beta, static_cast<double*>(S), lds,
                                   static_cast<uint32_t*>(flags), rmax != nullptr, static_cast<const double*>(rmax), 0.0);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_col_medians_resume(plaidhip_ctx* ctx, const void* S, int64_t lds, int32_t m, int32_t n, int ignore_zero,
                                    const void* flags, void* med) try {
  PH_CTX(ctx);
  PH_REQUIRE(m >= 0 && n >= 0 && lds >= m, "col_medians_resume: bad dims m=%d n=%d lds=%lld", m, n, (long long)lds);
  PH_REQUIRE(n == 0 || (S != nullptr && med != nullptr), "col_medians_resume: null S/med");
  PH_REQUIRE(ignore_zero >= -1 && ignore_zero <= 1, "col_medians_resume: ignore_zero=%d", ignore_zero);
  PH_REQUIRE(ignore_zero >= 0 || flags != nullptr, "col_medians_resume: ignore_zero = auto needs the flag words");
  return launch_col_medians_resume(ctx, static_cast<const double*>(S), lds, m, n, ignore_zero,
                                   static_cast<const uint32_t*>(flags), static_cast<double*>(med));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_col_medians_resume_token(plaidhip_ctx* ctx, int64_t token, const void* S, int64_t lds, int32_t m, int32_t n,
                                          int ignore_zero, const void* flags, void* med) try {
  PH_CTX(ctx);
  PH_REQUIRE(token >= 0, "col_medians_resume_token: token=%lld (0 = none, > 0 = what fused_medians_info returned)", (long long)token);
  PH_REQUIRE(m >= 0 && n >= 0 && lds >= m, "col_medians_resume_token: bad dims m=%d n=%d lds=%lld", m, n, (long long)lds);
  PH_REQUIRE(n == 0 || (S != nullptr && med != nullptr), "col_medians_resume_token: null S/med");
  PH_REQUIRE(ignore_zero >= -1 && ignore_zero <= 1, "col_medians_resume_token: ignore_zero=%d", ignore_zero);
  PH_REQUIRE(ignore_zero >= 0 || flags != nullptr, "col_medians_resume_token: ignore_zero = auto needs the flag words");
  return launch_col_medians_resume(ctx, static_cast<const double*>(S), lds, m, n, ignore_zero,
                                   static_cast<const uint32_t*>(flags), static_cast<double*>(med), token);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_fused_medians_discard(plaidhip_ctx* ctx) try {
  PH_CTX(ctx);
  ctx->fmed.valid = false;
  ctx->fmed.token = 0;
  // the caller will not normalise: the candidate scratch (up to 0.2 x the bytes of S) goes back too.  (Stream-ordered work
  // may still read it: wait for the stream first.  The next fused crossprod allocates again.)
  if (ctx->fmed_buf != nullptr) {
    PH_HIP(hipStreamSynchronize(ctx->stream));
    PH_HIP(hipFree(ctx->fmed_buf));
    ctx->fmed_buf = nullptr;
    ctx->fmed_bytes = 0;
    ctx->fmed = decltype(ctx->fmed){};
  }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_fused_medians_info(plaidhip_ctx* ctx, int64_t info[4]) try {
  PH_CTX(ctx);
  PH_REQUIRE(info != nullptr, "fused_medians_info: null info");
  info[0] = ctx->fmed.n;
  info[1] = (int64_t)reinterpret_cast<intptr_t>(ctx->fmed.status);
  info[2] = (int64_t)reinterpret_cast<intptr_t>(ctx->fmed.cal);
  info[3] = ctx->fmed.valid ? (int64_t)ctx->fmed.token : 0;
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_colranks_dense_f64(plaidhip_ctx* ctx, const void* X, int64_t ldx, int32_t g,
                                    int32_t n, int ties, int is_signed, double power, void* R,
                                    int64_t ldr, void* colmax) try {
  PH_CTX(ctx);
  PH_TRY(check_ties(ties, 0, power, colmax));
  PH_REQUIRE(g >= 0 && n >= 0, "colranks: bad dims g=%d n=%d", g, n);
  PH_REQUIRE(g == 0 || n == 0 || (X && R), "colranks: null X/R");
  PH_REQUIRE(ldx >= g && ldr >= g, "colranks: leading dims below g");
  return launch_colranks_dense_f64(ctx, static_cast<const double*>(X), ldx, g, n, ties, is_signed,
                                   power, static_cast<double*>(R), ldr, static_cast<double*>(colmax));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_colranks_csc_f64(plaidhip_ctx* ctx, const void* Xp, const void* Xx, int32_t n,
                                  int32_t max_col_nnz, int ties, int is_signed, double power, void* Rx,
                                  void* colmax) try {
  PH_CTX(ctx);
  PH_TRY(check_ties(ties, 1, power, colmax));
  PH_REQUIRE(n >= 0 && max_col_nnz >= 0, "colranks_csc: n=%d max_col_nnz=%d", n, max_col_nnz);
  PH_REQUIRE(n == 0 || Xp != nullptr, "colranks_csc: null Xp");
  return launch_colranks_csc_f64(ctx, static_cast<const int32_t*>(Xp), static_cast<const double*>(Xx),
                                 n, max_col_nnz, ties, is_signed, power, static_cast<double*>(Rx),
                                 static_cast<double*>(colmax));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_colranks_csc_dense_f64(plaidhip_ctx* ctx, const void* Xp, const void* Xi, const void* Xx,
                                        int32_t g, int32_t n, int ties, int is_signed, double power,
                                        void* R, int64_t ldr, void* colmax) try {
  PH_CTX(ctx);
  PH_TRY(check_ties(ties, 2));
  PH_REQUIRE(g >= 0 && n >= 0 && ldr >= g, "colranks_csc_dense: bad dims g=%d n=%d ldr=%lld", g, n, (long long)ldr);
  PH_REQUIRE(n == 0 || g == 0 || (Xp && R), "colranks_csc_dense: null Xp/R");
  return launch_colranks_csc_dense_f64(ctx, static_cast<const int32_t*>(Xp), static_cast<const int32_t*>(Xi),
                                       static_cast<const double*>(Xx), g, n, ties, is_signed, power,
                                       static_cast<double*>(R), ldr, static_cast<double*>(colmax));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_colranks_csc_dense_nz_f64(plaidhip_ctx* ctx, const void* Xp, const void* Xi, const void* Xx, int32_t g,
                                           int32_t n, int32_t max_col_nnz, int ties, int is_signed, double power,
                                           void* Rx_scratch, void* R, int64_t ldr, void* colmax) try {
  PH_CTX(ctx);
  PH_TRY(check_ties(ties, 2));
  PH_REQUIRE(g >= 0 && n >= 0 && ldr >= g, "colranks_csc_dense_nz: bad dims g=%d n=%d ldr=%lld", g, n, (long long)ldr);
  PH_REQUIRE(n == 0 || g == 0 || (Xp && R), "colranks_csc_dense_nz: null Xp/R");
  PH_REQUIRE(max_col_nnz >= 0 && max_col_nnz <= g, "colranks_csc_dense_nz: max_col_nnz=%d outside [0, nrow(X)=%d]", max_col_nnz, g);
  if (max_col_nnz > max_sparse_rank_column()) {
    set_error("colranks_csc_dense_nz: a column with %d stored values (at most %d are ranked in one pass: use "
              "plaidhip_dev_colranks_csc_dense_f64)", max_col_nnz, max_sparse_rank_column());
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(max_col_nnz == 0 || Rx_scratch != nullptr, "colranks_csc_dense_nz: null Rx_scratch");
  return launch_colranks_csc_dense_nz_f64(ctx, static_cast<const int32_t*>(Xp), static_cast<const int32_t*>(Xi),
                                          static_cast<const double*>(Xx), g, n, max_col_nnz, ties, is_signed, power,
                                          static_cast<double*>(Rx_scratch), static_cast<double*>(R), ldr,
                                          static_cast<double*>(colmax));
} catch (...) { return plaidhip::on_exception(); }

// replaid.ssgsea.exact's operand pass (kernels_walk.hip), stream-ordered
int plaidhip_dev_ssgsea_exact_operands_f64(plaidhip_ctx* ctx, const void* X, int64_t ldx, int32_t g, int32_t n, double alpha,
                                           void* Q, void* W, void* P, int64_t ldq, void* scratch, void* colnan) try {
  PH_CTX(ctx);
  PH_REQUIRE(std::isfinite(alpha), "ssgsea_exact_operands: alpha must be finite (got %g)", alpha);
  PH_REQUIRE(g >= 0 && n >= 0 && g < (1 << 26), "ssgsea_exact_operands: bad dims g=%d n=%d", g, n);
  PH_REQUIRE(ldx >= g && ldq >= g, "ssgsea_exact_operands: leading dims below g");
  PH_REQUIRE(n == 0 || colnan != nullptr, "ssgsea_exact_operands: null colnan");
  PH_REQUIRE(g == 0 || n == 0 || (X && Q && scratch), "ssgsea_exact_operands: null X/Q/scratch");
  PH_REQUIRE(alpha == 0.0 || g == 0 || n == 0 || (W && P), "ssgsea_exact_operands: W and P are needed when alpha != 0");
  return launch_ssgsea_exact_operands(ctx, static_cast<const double*>(X), ldx, nullptr, nullptr, g, n, 0, 0, alpha,
                                      static_cast<double*>(Q), static_cast<double*>(W), static_cast<double*>(P), ldq,
                                      static_cast<double*>(scratch), static_cast<uint32_t*>(colnan));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_ssgsea_exact_operands_csc_f64(plaidhip_ctx* ctx, const void* Xp, const void* Xi, const void* Xx, int32_t g,
                                               int32_t n, int32_t max_col_nnz, int64_t nnz, double alpha, void* Q, void* W,
                                               void* P, int64_t ldq, void* scratch, void* colnan) try {
  PH_CTX(ctx);
  PH_REQUIRE(std::isfinite(alpha), "ssgsea_exact_operands_csc: alpha must be finite (got %g)", alpha);
  PH_REQUIRE(g >= 0 && n >= 0 && g < (1 << 26) && ldq >= g, "ssgsea_exact_operands_csc: bad dims g=%d n=%d ldq=%lld", g, n,
             (long long)ldq);
  PH_REQUIRE(max_col_nnz >= 0 && max_col_nnz <= g && nnz >= 0, "ssgsea_exact_operands_csc: max_col_nnz=%d nnz=%lld", max_col_nnz,
             (long long)nnz);
  PH_REQUIRE(n == 0 || (Xp && colnan), "ssgsea_exact_operands_csc: null Xp/colnan");
  PH_REQUIRE(g == 0 || n == 0 || Q != nullptr, "ssgsea_exact_operands_csc: null Q");
  PH_REQUIRE(nnz == 0 || (Xi && Xx && scratch), "ssgsea_exact_operands_csc: null Xi/Xx/scratch");
  PH_REQUIRE(alpha == 0.0 || g == 0 || n == 0 || (W && P), "ssgsea_exact_operands_csc: W and P are needed when alpha != 0");
  return launch_ssgsea_exact_operands(ctx, static_cast<const double*>(Xx), 0, static_cast<const int32_t*>(Xp),
                                      static_cast<const int32_t*>(Xi), g, n, max_col_nnz, nnz, alpha, static_cast<double*>(Q),
                                      static_cast<double*>(W), static_cast<double*>(P), ldq, static_cast<double*>(scratch),
                                      static_cast<uint32_t*>(colnan));
} catch (...) { return plaidhip::on_exception(); }

// the walk of replaid.ssgsea.exact(single = FALSE) on device operands (kernels_ks.hip), stream-ordered
int plaidhip_dev_gsea_ks_f64(plaidhip_ctx* ctx, const void* Q, const void* W, int64_t ldq, const void* colnan, int32_t g,
                             int32_t n, const void* Gp, const void* Gi, int32_t m, double alpha, int scale, void* S,
                             int64_t lds) try {
  PH_CTX(ctx);
  PH_REQUIRE(std::isfinite(alpha), "gsea_ks: alpha must be finite (got %g)", alpha);
  PH_REQUIRE(g > 0 && n >= 0 && m >= 0 && ldq >= g && lds >= m, "gsea_ks: bad dims g=%d n=%d m=%d ldq=%lld lds=%lld", g, n, m,
             (long long)ldq, (long long)lds);
  PH_TRY(check_gsea_ks_genes(g));
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(Q && colnan && Gp && Gi && S, "gsea_ks: null Q/colnan/Gp/Gi/S");
  PH_REQUIRE(alpha == 0.0 || W != nullptr, "gsea_ks: W is needed when alpha != 0");
  double* Wpos = nullptr;
  if (alpha != 0.0) {
    PH_TRY(ensure_workspace(ctx, (size_t)ldq * n * 8));
    Wpos = static_cast<double*>(ctx->ws);
  }
  return launch_gsea_ks(ctx, static_cast<const double*>(Q), static_cast<const double*>(W), Wpos, ldq,
                        static_cast<const uint32_t*>(colnan), g, n, static_cast<const int32_t*>(Gp),
                        static_cast<const int32_t*>(Gi), m, alpha, scale, static_cast<double*>(S), lds);
} catch (...) { return plaidhip::on_exception(); }

// the walk of replaid.gsva.exact on the device's last ranks (kernels_ks.hip), stream-ordered
int plaidhip_dev_gsva_ks_f64(plaidhip_ctx* ctx, const void* Q, int64_t ldq, const void* colnan, int32_t g, int32_t n,
                             const void* Gp, const void* Gi, int32_t m, double tau, int max_diff, void* S, int64_t lds) try {
  PH_CTX(ctx);
  PH_REQUIRE(std::isfinite(tau) && tau >= 0.0, "gsva_ks: tau must be finite and >= 0 (got %g)", tau);
  PH_REQUIRE(g > 0 && n >= 0 && m >= 0 && ldq >= g && lds >= m, "gsva_ks: bad dims g=%d n=%d m=%d ldq=%lld lds=%lld", g, n, m,
             (long long)ldq, (long long)lds);
  if (g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("gsva_ks: nrow(X) = %d (at most %d rows)", g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(Q && colnan && Gp && Gi && S, "gsva_ks: null Q/colnan/Gp/Gi/S");
  double* T = nullptr;
  if (tau != 0.0) {   // the weight table
    PH_TRY(ensure_workspace(ctx, (size_t)g * 8));
    T = static_cast<double*>(ctx->ws);
  }
  return launch_gsva_ks(ctx, static_cast<const double*>(Q), ldq, static_cast<const uint32_t*>(colnan), g, n,
                        static_cast<const int32_t*>(Gp), static_cast<const int32_t*>(Gi), m, tau, max_diff, T,
                        static_cast<double*>(S), lds);
} catch (...) { return plaidhip::on_exception(); }

// the dispersion of replaid.sing.exact on the device's min and last ranks (kernels_sing.hip), stream-ordered
int plaidhip_dev_sing_mad_f64(plaidhip_ctx* ctx, const void* R, const void* Q, int64_t ldq, const void* colnan, int32_t g,
                              int32_t n, const void* Gp, const void* Gi, int32_t m, void* S, int64_t lds) try {
  PH_CTX(ctx);
  PH_REQUIRE(g > 0 && n >= 0 && m >= 0 && ldq >= g && lds >= m, "sing_mad: bad dims g=%d n=%d m=%d ldq=%lld lds=%lld", g, n, m,
             (long long)ldq, (long long)lds);
  if (g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("sing_mad: nrow(X) = %d (at most %d rows)", g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(R && Q && colnan && Gp && Gi && S, "sing_mad: null R/Q/colnan/Gp/Gi/S");
  PH_TRY(ensure_workspace(ctx, (size_t)g * n * 4));   // the ranks by position
  uint32_t* Rpos = static_cast<uint32_t*>(ctx->ws);
  PH_TRY(launch_sing_rpos(ctx, static_cast<const double*>(R), static_cast<const double*>(Q), ldq,
                          static_cast<const uint32_t*>(colnan), g, n, Rpos, g));
  return launch_sing_mad(ctx, static_cast<const double*>(Q), ldq, Rpos, g, static_cast<const uint32_t*>(colnan), g, n,
                         static_cast<const int32_t*>(Gp), static_cast<const int32_t*>(Gi), m, static_cast<double*>(S), lds);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_minflags(plaidhip_ctx* ctx, const void* S, int64_t count, void* flags) try {
  PH_CTX(ctx);
  PH_REQUIRE(flags != nullptr && count >= 0, "minflags: bad arguments");
  return launch_minflags(ctx, static_cast<const double*>(S), count, static_cast<uint32_t*>(flags));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_col_medians(plaidhip_ctx* ctx, const void* S, int64_t lds, int32_t m, int32_t n,
                             int ignore_zero, const void* flags, void* med) try {
  PH_CTX(ctx);
  PH_REQUIRE(m >= 0 && n >= 0 && lds >= m, "col_medians: bad dims m=%d n=%d lds=%lld", m, n, (long long)lds);
  PH_REQUIRE(ignore_zero >= -1 && ignore_zero <= 1, "col_medians: bad ignore_zero %d", ignore_zero);
  PH_REQUIRE(ignore_zero >= 0 || flags != nullptr, "col_medians: ignore_zero=auto needs the flags words");
  PH_REQUIRE(n == 0 || med != nullptr, "col_medians: null med");
  return launch_col_medians(ctx, static_cast<const double*>(S), lds, m, n, ignore_zero,
                            static_cast<const uint32_t*>(flags), static_cast<double*>(med));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_sum(plaidhip_ctx* ctx, const void* v, int64_t count, void* out) try {
  PH_CTX(ctx);
  PH_REQUIRE(out != nullptr && count >= 0, "sum: bad arguments");
  return launch_sum(ctx, static_cast<const double*>(v), count, static_cast<double*>(out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_max(plaidhip_ctx* ctx, const void* v, int64_t count, void* out) try {
  PH_CTX(ctx);
  PH_REQUIRE(out != nullptr && count >= 0, "max: bad arguments");
  return launch_max(ctx, static_cast<const double*>(v), count, static_cast<double*>(out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_shift_columns(plaidhip_ctx* ctx, void* S, int64_t lds, int32_t m, int32_t n,
                               const void* med, double add, const void* red) try {
  PH_CTX(ctx);
  PH_REQUIRE(m >= 0 && n >= 0 && lds >= m, "shift_columns: bad dims");
  return launch_shift_columns(ctx, static_cast<double*>(S), lds, m, n, static_cast<const double*>(med), add,
                              static_cast<const double*>(red));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_shift_columns_cast_f32(plaidhip_ctx* ctx, const void* S, int64_t lds, int32_t m, int32_t n, const void* med,
                                        double add, const void* red, void* out, int64_t ldo) try {
  PH_CTX(ctx);
  PH_REQUIRE(m >= 0 && n >= 0 && lds >= m && ldo >= m, "shift_columns_cast_f32: bad dims");
  PH_REQUIRE((m == 0 || n == 0) || (S != nullptr && med != nullptr && out != nullptr), "shift_columns_cast_f32: null argument");
  return launch_shift_columns_cast_f32(ctx, static_cast<const double*>(S), lds, m, n, static_cast<const double*>(med), add,
                                       static_cast<const double*>(red), static_cast<float*>(out), ldo);
} catch (...) { return plaidhip::on_exception(); }

// ---- host-level pipelines ---------------------------------------------------------------


int plaidhip_plaid_dense(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n,
                         const int32_t* Gp, const int32_t* Gi, int32_t m, int stat, int normalize,
                         double* S_out) try {
  PH_REQUIRE(stat == PLAIDHIP_STAT_MEAN || stat == PLAIDHIP_STAT_SUM, "plaid_dense: bad stat %d", stat);
  PH_REQUIRE(n == 0 || (X && S_out), "plaid_dense: null X/S_out");
  // one shard on this context: pipelined upload, crossprod per column panel, normalize_medians, download (shard_rank_sum.cpp)
  return dispatch(on_context(ctx), plaid_call({nullptr, nullptr, X, g, n, Gp, Gi, m}, stat, normalize, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plaid_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx,
                       int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                       int stat, int normalize, double* S_out) try {
  PH_REQUIRE(stat == PLAIDHIP_STAT_MEAN || stat == PLAIDHIP_STAT_SUM, "plaid_csc: bad stat %d", stat);
  PH_REQUIRE(Xp != nullptr && (n == 0 || S_out), "plaid_csc: null Xp/S_out");
  return dispatch(on_context(ctx), plaid_call({Xp, Xi, Xx, g, n, Gp, Gi, m}, stat, normalize, S_out));
} catch (...) { return plaidhip::on_exception(); }

// chunked_crossprod with a general sparse x: upload the slots, one launch, download (host pointers)
static int crossprod_weighted_host(plaidhip_ctx* ctx, const int32_t* Wp, const int32_t* Wi, const double* Wx, int32_t g,
                                   int32_t m, const double* Y, const int32_t* Yp, const int32_t* Yi, const double* Yx,
                                   int32_t n, double* S_out) {
  PH_REQUIRE(g > 0 && m >= 0 && n >= 0, "crossprod_weighted: bad dims g=%d m=%d n=%d", g, m, n);
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(S_out != nullptr, "crossprod_weighted: null S_out");
  PH_TRY(check_host_csc(Wp, Wi, g, m));
  const int64_t zw = Wp[m];
  PH_REQUIRE(zw == 0 || (Wi != nullptr && Wx != nullptr), "crossprod_weighted: null x@i / x@x");
  int64_t zy = 0;
  if (Yp != nullptr) {
    PH_TRY(check_host_csc(Yp, Yi, g, n));
    zy = Yp[n];
    PH_REQUIRE(zy == 0 || (Yi != nullptr && Yx != nullptr), "crossprod_weighted: null y@i / y@x");
  } else {
    PH_REQUIRE(Y != nullptr, "crossprod_weighted: null y");
  }
  DevBuf dWp, dWi, dWx, dY, dYi, dYx, dS;
  PH_TRY(dWp.alloc((size_t)(m + 1) * 4));
  PH_TRY(dWi.alloc((size_t)(zw > 0 ? zw : 1) * 4));
  PH_TRY(dWx.alloc((size_t)(zw > 0 ? zw : 1) * 8));
  PH_TRY(dS.alloc((size_t)m * n * 8));
  PH_TRY(h2d(ctx, dWp.p, Wp, (size_t)(m + 1) * 4));
  PH_TRY(h2d(ctx, dWi.p, Wi, (size_t)zw * 4));
  PH_TRY(h2d(ctx, dWx.p, Wx, (size_t)zw * 8));
  if (Yp != nullptr) {
    PH_TRY(dY.alloc((size_t)(n + 1) * 4));
    PH_TRY(dYi.alloc((size_t)(zy > 0 ? zy : 1) * 4));
    PH_TRY(dYx.alloc((size_t)(zy > 0 ? zy : 1) * 8));
    PH_TRY(h2d(ctx, dY.p, Yp, (size_t)(n + 1) * 4));
    PH_TRY(h2d(ctx, dYi.p, Yi, (size_t)zy * 4));
    PH_TRY(h2d(ctx, dYx.p, Yx, (size_t)zy * 8));
    PH_TRY(launch_crossprod_weighted_f64(ctx, dWp.as<int32_t>(), dWi.as<int32_t>(), dWx.as<double>(), g, m, nullptr, 0,
                                         dY.as<int32_t>(), dYi.as<int32_t>(), dYx.as<double>(), n, dS.as<double>(), m));
  } else {
    PH_TRY(dY.alloc((size_t)g * n * 8));
    PH_TRY(h2d(ctx, dY.p, Y, (size_t)g * n * 8));
    PH_TRY(launch_crossprod_weighted_f64(ctx, dWp.as<int32_t>(), dWi.as<int32_t>(), dWx.as<double>(), g, m, dY.as<double>(),
                                         g, nullptr, nullptr, nullptr, n, dS.as<double>(), m));
  }
  PH_TRY(copy_home(ctx, S_out, dS.p, (size_t)m * n * 8));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return PLAIDHIP_OK;
}

int plaidhip_crossprod_weighted_dense(plaidhip_ctx* ctx, const int32_t* Wp, const int32_t* Wi, const double* Wx,
                                      int32_t g, int32_t m, const double* Y, int32_t n, double* S_out) try {
  PH_CTX(ctx);
  return crossprod_weighted_host(ctx, Wp, Wi, Wx, g, m, Y, nullptr, nullptr, nullptr, n, S_out);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_crossprod_weighted_csc(plaidhip_ctx* ctx, const int32_t* Wp, const int32_t* Wi, const double* Wx,
                                    int32_t g, int32_t m, const int32_t* Yp, const int32_t* Yi, const double* Yx,
                                    int32_t n, double* S_out) try {
  PH_CTX(ctx);
  PH_REQUIRE(Yp != nullptr, "crossprod_weighted_csc: null y@p");
  return crossprod_weighted_host(ctx, Wp, Wi, Wx, g, m, nullptr, Yp, Yi, Yx, n, S_out);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_normalize_medians(plaidhip_ctx* ctx, double* S, int32_t m, int32_t n, int ignore_zero,
                               double* med_out) try {
  PH_CTX(ctx);
  PH_REQUIRE(m >= 0 && n >= 0, "normalize_medians: bad dims");
  PH_REQUIRE(ignore_zero >= -1 && ignore_zero <= 1, "normalize_medians: bad ignore_zero %d", ignore_zero);
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(S != nullptr, "normalize_medians: null S");
  DevBuf dS, dsmall;
  PH_TRY(dS.alloc((size_t)m * n * 8));
  PH_TRY(dsmall.alloc(64 + (size_t)n * 8));
  uint32_t* d_flags = dsmall.as<uint32_t>();
  double* d_red = reinterpret_cast<double*>(dsmall.as<char>() + 16);
  double* d_med = reinterpret_cast<double*>(dsmall.as<char>() + 64);
  PH_TRY(h2d(ctx, dS.p, S, (size_t)m * n * 8));
  PH_TRY(normalize_on_device(ctx, dS.as<double>(), m, n, ignore_zero, d_flags, false, d_med, d_red));
  PH_TRY(copy_home(ctx, S, dS.p, (size_t)m * n * 8));
  if (med_out) PH_HIP(hipMemcpyAsync(med_out, d_med, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_colranks_dense(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, int ties,
                            int is_signed, double* R_out) try {
  PH_CTX(ctx);
  PH_TRY(check_ties(ties, 0));
  PH_REQUIRE(g >= 0 && n >= 0, "colranks_dense: bad dims");
  if ((int64_t)g * n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(X && R_out, "colranks_dense: null X/R_out");
  DevBuf dX, dR;
  PH_TRY(dX.alloc((size_t)g * n * 8));
  PH_TRY(dR.alloc((size_t)g * n * 8));
  PH_TRY(h2d(ctx, dX.p, X, (size_t)g * n * 8));
  PH_TRY(launch_colranks_dense_f64(ctx, dX.as<double>(), g, g, n, ties, is_signed, 1.0, dR.as<double>(), g, nullptr));
  PH_TRY(copy_home(ctx, R_out, dR.p, (size_t)g * n * 8));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_colranks_csc(plaidhip_ctx* ctx, const int32_t* Xp, const double* Xx, int32_t n,
                          int ties, int is_signed, double* Rx_out) try {
  PH_CTX(ctx);
  PH_TRY(check_ties(ties, 1));
  PH_REQUIRE(n >= 0 && Xp != nullptr, "colranks_csc: bad arguments");
  PH_TRY(check_host_csc(Xp, nullptr, 0, n));
  const int64_t zx = Xp[n];
  if (zx == 0) return PLAIDHIP_OK;
  PH_REQUIRE(Xx && Rx_out, "colranks_csc: null Xx/Rx_out");
  DevBuf dXp, dXx, dR;
  PH_TRY(dXp.alloc((size_t)(n + 1) * 4));
  PH_TRY(dXx.alloc((size_t)zx * 8));
  PH_TRY(dR.alloc((size_t)zx * 8));
  PH_TRY(h2d(ctx, dXp.p, Xp, (size_t)(n + 1) * 4));
  PH_TRY(h2d(ctx, dXx.p, Xx, (size_t)zx * 8));
  PH_TRY(launch_colranks_csc_f64(ctx, dXp.as<int32_t>(), dXx.as<double>(), n, host_max_col_nnz(Xp, n), ties, is_signed,
                                 1.0, dR.as<double>(), nullptr));
  PH_TRY(copy_home(ctx, Rx_out, dR.p, (size_t)zx * 8));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_colranks_csc_dense(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx,
                                int32_t g, int32_t n, int ties, int is_signed, double* R_out) try {
  PH_CTX(ctx);
  PH_TRY(check_ties(ties, 2));
  PH_REQUIRE(g >= 0 && n >= 0 && Xp != nullptr, "colranks_csc_dense: bad arguments");
  PH_TRY(check_host_csc(Xp, Xi, g, n));
  if ((int64_t)g * n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(R_out != nullptr, "colranks_csc_dense: null R_out");
  const int64_t zx = Xp[n];
  DevBuf dXp, dXi, dXx, dR;
  PH_TRY(dXp.alloc((size_t)(n + 1) * 4));
  PH_TRY(dXi.alloc((size_t)zx * 4));
  PH_TRY(dXx.alloc((size_t)zx * 8));
  PH_TRY(dR.alloc((size_t)g * n * 8));
  PH_TRY(h2d(ctx, dXp.p, Xp, (size_t)(n + 1) * 4));
  PH_TRY(h2d(ctx, dXi.p, Xi, (size_t)zx * 4));
  PH_TRY(h2d(ctx, dXx.p, Xx, (size_t)zx * 8));
  // zeros tie: the dense ranks follow from the ranks of the stored values (kernels_rank.hip) unless a column stores
  // more values than the rank kernel takes in one pass -- then the column is densified and ranked as a dense one
  const int32_t max_nnz = host_max_col_nnz(Xp, n);
  if (max_nnz <= max_sparse_rank_column()) {
    DevBuf dRx;
    PH_TRY(dRx.alloc((size_t)(zx > 0 ? zx : 1) * 8));
    PH_TRY(launch_colranks_csc_dense_nz_f64(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), dXx.as<double>(), g, n, max_nnz, ties,
                                            is_signed, 1.0, dRx.as<double>(), dR.as<double>(), g, nullptr));
    PH_TRY(copy_home(ctx, R_out, dR.p, (size_t)g * n * 8));
    PH_HIP(hipStreamSynchronize(ctx->stream));   // (dRx is released behind this)
    return PLAIDHIP_OK;
  }
  PH_TRY(launch_colranks_csc_dense_f64(ctx, dXp.as<int32_t>(), dXi.as<int32_t>(), dXx.as<double>(), g, n, ties,
                                       is_signed, 1.0, dR.as<double>(), g, nullptr));
  PH_TRY(copy_home(ctx, R_out, dR.p, (size_t)g * n * 8));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_sing_dense(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out) try {
  return dispatch(on_context(ctx), sing_call({nullptr, nullptr, X, g, n, Gp, Gi, m}, S_out));
} catch (...) { return plaidhip::on_exception(); }

// replaid.sing for a dgCMatrix X: colranks(X, ties.method = "min") ranks the zeros too (sparse branch without keep.zero,
// R/plaid.R:602-609), / nrow(X) - 0.5, plaid(normalize = FALSE) (:215-217).  The reference densifies X to rank it; here
// the CSC slots go to the device as they are, the dense min-ranks are built per panel of columns from the ranks of the
// stored values (zeros tie), and the rank crossprod runs on each panel (shard_rank_sum.cpp: shard_worker): neither the host nor
// the PCIe link sees a dense X.
int plaidhip_sing_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                      const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out) try {
  PH_REQUIRE(Xp != nullptr, "sing_csc: null Xp");
  return dispatch(on_context(ctx), sing_call({Xp, Xi, Xx, g, n, Gp, Gi, m}, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_ssgsea_dense(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n,
                          const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha,
                          double* S_out) try {
  return dispatch(on_context(ctx), ssgsea_call({nullptr, nullptr, X, g, n, Gp, Gi, m}, alpha, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_ssgsea_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx,
                        int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                        double alpha, double* S_out) try {
  PH_REQUIRE(Xp != nullptr, "ssgsea_csc: null Xp");
  // sparse branch: ranks of the non-zeros only, zeros stay 0 (R/plaid.R:600-601, 631-650); the "- 0.5" of
  // R/plaid.R:251 applies to the zeros too, which the (alpha, beta) epilogue covers
  return dispatch(on_context(ctx), ssgsea_call({Xp, Xi, Xx, g, n, Gp, Gi, m}, alpha, S_out));
} catch (...) { return plaidhip::on_exception(); }

// replaid.ssgsea.exact: the one-device form of the sharded engine (shard_exact.cpp: ssgsea_exact_worker)
int plaidhip_ssgsea_exact(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                          const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale, int norm,
                          double* S_out) try {
  return dispatch(on_context(ctx), ssgsea_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, scale, norm, S_out, 1));
} catch (...) { return plaidhip::on_exception(); }

// replaid.ssgsea.exact(single = FALSE): the same engine with the walk kernel of kernels_ks.hip
int plaidhip_ssgsea_exact_ks(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                             const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale, int norm,
                             double* S_out) try {
  return dispatch(on_context(ctx), ssgsea_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, scale, norm, S_out, 0));
} catch (...) { return plaidhip::on_exception(); }

}  // extern "C"

// ---- replaid.ucell / aucell / scse / gsva and plaid.test: the one-shard case of the sharded engine ------------------------
// (shard_scorer.cpp: scorer_worker, shard_plaid_test.cpp: plaid_test_worker; dispatch checks the arguments first)
extern "C" {

int plaidhip_ucell(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                   int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                   const double* k_full, double rmax, double* S_out) try {
  return dispatch(on_context(ctx), ucell_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, k_full, rmax, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_aucell(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                    int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                    double auc_max_rank, double* S_out) try {
  return dispatch(on_context(ctx), aucell_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, auc_max_rank, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_scse(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                  int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                  int remove_log2, int score_mean, double* S_out, int* removed_log2) try {
  return dispatch(on_context(ctx), scse_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, remove_log2, score_mean, S_out, removed_log2));
} catch (...) { return plaidhip::on_exception(); }

// Row-wise two-group sums / sums of squared deviations on device pointers: the pieces of plaid.test that a sample-sharded
// caller all-reduces between (plaid_amd/sharded.py: sharded_plaid_test).  A: rows x n column-major with leading dimension
// ld; y: 0 / 1 per column; sums / ssd: [2][rows] (group 0, group 1).
int plaidhip_dev_row_group_sums(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const int32_t* y,
                                double* sums) try {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && n >= 0 && ld >= rows, "row_group_sums: bad shape rows=%d n=%d ld=%lld", rows, n, (long long)ld);
  if (rows == 0) return PLAIDHIP_OK;
  PH_REQUIRE(sums && (n == 0 || (A && y)), "row_group_sums: null argument");
  PH_TRY(ensure_workspace(ctx, (size_t)row_group_ws_doubles(rows, n) * 8));
  return launch_row_group_moments(ctx, A, ld, rows, n, y, 1, 1, sums, nullptr, static_cast<double*>(ctx->ws));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_row_group_ssd(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const int32_t* y,
                               const double* mean, double* ssd) try {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && n >= 0 && ld >= rows, "row_group_ssd: bad shape rows=%d n=%d ld=%lld", rows, n, (long long)ld);
  if (rows == 0) return PLAIDHIP_OK;
  PH_REQUIRE(ssd && mean && (n == 0 || (A && y)), "row_group_ssd: null argument");
  PH_TRY(ensure_workspace(ctx, (size_t)row_group_ws_doubles(rows, n) * 8));
  return launch_row_group_ssd(ctx, A, ld, rows, n, y, mean, ssd, static_cast<double*>(ctx->ws));
} catch (...) { return plaidhip::on_exception(); }

// the two entries above for C label columns at once (kernels_contrasts.hip); Y: n x C, sums / mean / ssd: [C][2][rows].  The
// label masks and the block partials live in the context's workspace.
static int dev_row_contrast_moment(plaidhip_ctx* ctx, const char* what, const double* A, int64_t ld, int32_t rows, int32_t n,
                                   const int32_t* Y, int32_t C, const double* mean, bool need_mean, double* out) {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && n >= 0 && ld >= rows && C >= 0 && C <= 65535, "%s: bad shape rows=%d n=%d ld=%lld C=%d", what, rows,
             n, (long long)ld, C);
  if (rows == 0 || C == 0) return PLAIDHIP_OK;
  PH_REQUIRE(out && (!need_mean || mean) && (n == 0 || (A && Y)), "%s: null argument", what);
  const size_t part = (size_t)row_contrast_ws_doubles(rows, n, C) * 8;
  PH_TRY(ensure_workspace(ctx, part + (size_t)contrast_mask_bytes(n, C)));
  double* ws = static_cast<double*>(ctx->ws);
  void* masks = static_cast<char*>(ctx->ws) + part;
  PH_TRY(launch_contrast_masks(ctx, Y, n, n, C, masks));
  PH_TRY(launch_row_contrast_partials(ctx, A, ld, rows, n, masks, C, nullptr, 0.0, mean, ws));
  return launch_reduce_blocks_flat(ctx, ws, (int64_t)C * 2 * rows, n, nullptr, out);
}

int plaidhip_dev_row_contrast_sums(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const int32_t* Y,
                                   int32_t C, double* sums) try {
  return dev_row_contrast_moment(ctx, "row_contrast_sums", A, ld, rows, n, Y, C, nullptr, false, sums);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_row_contrast_ssd(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const int32_t* Y,
                                  int32_t C, const double* mean, double* ssd) try {
  return dev_row_contrast_moment(ctx, "row_contrast_ssd", A, ld, rows, n, Y, C, mean, true, ssd);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_contrast_tile(void) { return PLAIDHIP_CONTRAST_TILE; }

// The host half of plaid.test (R/plaid.R:410-474): p-values, effect sizes, meta-p and FDR from the reduced statistics.
// Shared by the sharded engine (shard_plaid_test.cpp: plaid_test_tail) and by callers over RCCL, which all-reduce the statistics first.
int plaidhip_plaid_test_finish(int32_t g, int32_t m, const int32_t* Gp, const double* T, double tot1, double tot2,
                               const double* SM, int64_t n0, int64_t n1, int tests, int metap_method, double* out) try {
  PH_REQUIRE(g >= 0 && m >= 0 && (m == 0 || (Gp && out)), "plaid_test_finish: null Gp / out");
  PH_REQUIRE((tests & 7) != 0 && (tests & ~7) == 0, "plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)");
  PH_REQUIRE(metap_method == 0 || metap_method == 1, "Invalid method: %d", metap_method);      // R/plaid.R:533
  PH_REQUIRE(m == 0 || !(tests & 3) || T, "plaid_test_finish: null T");
  PH_REQUIRE(m == 0 || !(tests & 4) || SM, "plaid_test_finish: null SM");
  if (m == 0) return PLAIDHIP_OK;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double* o_fc = out;
  double* o_p1 = out + (size_t)m;
  double* o_p2 = out + 2 * (size_t)m;
  double* o_p3 = out + 3 * (size_t)m;
  double* o_pm = out + 4 * (size_t)m;
  double* o_q = out + 5 * (size_t)m;
  for (int32_t j = 0; j < m; ++j) {
    const double k = (double)(Gp[j + 1] - Gp[j]);
    double eff = 0.0, pv[3];
    int np = 0;
    o_p1[j] = o_p2[j] = o_p3[j] = nan;
    if (tests & 1) {
      double mean1;
      o_p1[j] = clamp_p(onesample_p(k, T[j], T[(size_t)m + j], &mean1));
      eff += mean1;
      pv[np++] = o_p1[j];
    }
    if (tests & 2) {
      double diff;
      o_p2[j] = clamp_p(twosample_p((double)g, k, T[j], T[(size_t)m + j], tot1, tot2, &diff));
      eff += diff;
      pv[np++] = o_p2[j];
    }
    if (tests & 4) {
      const double m0 = SM[j], m1 = SM[(size_t)m + j];
      o_p3[j] = clamp_p(welch_p(m0, m1, SM[2 * (size_t)m + j], SM[3 * (size_t)m + j], (double)n0, (double)n1));
      eff += m1 - m0;                                                                           // :431
      pv[np++] = o_p3[j];
    }
    o_fc[j] = eff / np;                                                                         // rowMeans(F), :453
    o_pm[j] = np > 1 ? combine_p(pv, np, metap_method) : pv[0];                                 // :455-460
  }
  p_adjust_fdr(o_pm, m, o_q);                                                                   // :463
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plaid_test(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const int32_t* y,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, const double* gsetX, int tests,
                        int metap_method, double* out) try {
  return dispatch(on_context(ctx), plaid_test_call({nullptr, nullptr, X, g, n, Gp, Gi, m}, y, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

// plaid.test.contrasts: the one-shard case of plaid_test_worker with C label columns (shard_plaid_test.cpp)
int plaidhip_plaid_test_contrasts(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const int32_t* Y, int32_t C,
                                  const int32_t* Gp, const int32_t* Gi, int32_t m, const double* gsetX, int tests,
                                  int metap_method, double* out) try {
  return dispatch(on_context(ctx),
                  plaid_test_contrasts_call({nullptr, nullptr, X, g, n, Gp, Gi, m}, Y, C, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plaid_test_contrasts_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g,
                                      int32_t n, const int32_t* Y, int32_t C, const int32_t* Gp, const int32_t* Gi, int32_t m,
                                      const double* gsetX, int tests, int metap_method, double* out) try {
  PH_REQUIRE(Xp != nullptr, "plaid_test_contrasts: null X");
  return dispatch(on_context(ctx), plaid_test_contrasts_call({Xp, Xi, Xx, g, n, Gp, Gi, m}, Y, C, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

// replaid.gsva.exact: the one-device form of the sharded engine (shard_scorer.cpp: scorer_worker, kGsvaExact)
int plaidhip_gsva_exact(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf, int max_diff,
                        double* S_out) try {
  return dispatch(on_context(ctx), gsva_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, tau, rowtf, max_diff, S_out));
} catch (...) { return plaidhip::on_exception(); }

// plaid.gsea: the one-device form of the sharded engine (shard_gsea.cpp: gsea_worker, kGsea)
int plaidhip_gsea(plaidhip_ctx* ctx, const double* stat, const double* weight, int32_t g, int32_t c, const int32_t* Gp,
                  const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed, double* out,
                  double* null_out) try {
  return dispatch(on_context(ctx), gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out));
} catch (...) { return plaidhip::on_exception(); }

// plaid.gsea with a score type and, when asked for, the leading edges: the same Call
int plaidhip_gsea_scored(plaidhip_ctx* ctx, const double* stat, const double* weight, int32_t g, int32_t c, const int32_t* Gp,
                         const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed, int score_type,
                         double* out, double* null_out, int32_t* le_len, int32_t* le_idx) try {
  return dispatch(on_context(ctx),
                  gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out, score_type, le_len, le_idx));
} catch (...) { return plaidhip::on_exception(); }

// plaid.gsea with multilevel p-values, and one ruler's trace: the same engine (shard_gsea.cpp: gsea_worker / gsea_ruler_worker,
// kGseaMultilevel)
int plaidhip_gsea_multilevel(plaidhip_ctx* ctx, const double* stat, const double* weight, int32_t g, int32_t c,
                             const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed,
                             int score_type, int32_t sample_size, int32_t sweeps, double eps, int32_t ml_min, double* out,
                             double* null_out, int32_t* le_len, int32_t* le_idx, double* ml_out) try {
  return dispatch(on_context(ctx), gsea_multilevel_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, score_type, sample_size,
                                                        sweeps, eps, ml_min, out, null_out, le_len, le_idx, ml_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsea_ruler(plaidhip_ctx* ctx, const double* stat, const double* weight, int32_t g, int32_t k, int32_t l, int side,
                        int score_type, double gamma, uint64_t seed, int32_t sample_size, int32_t sweeps, double eps,
                        int32_t* nstages, int32_t* end_status, double* m_out, int32_t* s_out, double* h_out) try {
  return dispatch(on_context(ctx), gsea_ruler_call(stat, weight, g, k, l, side, score_type, gamma, seed, sample_size, sweeps, eps,
                                                   nstages, end_status, m_out, s_out, h_out));
} catch (...) { return plaidhip::on_exception(); }

// plaid.rankcor: the one-device form of the sharded engine (shard_lists.cpp: rankcor_worker, kRankcor)
int plaidhip_rankcor(plaidhip_ctx* ctx, const double* stat, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m,
                     int use_rank, int ties, double* out, double* tot_out) try {
  return dispatch(on_context(ctx), rankcor_call(stat, g, c, Gp, Gi, m, use_rank, ties, out, tot_out));
} catch (...) { return plaidhip::on_exception(); }

// replaid.plage / replaid.zscore: the one-device forms of the sharded engine (shard_lists.cpp: plage_worker, kPlage / kZscore)
int plaidhip_plage(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                   double tol, int32_t maxit, double* S_out, double* info_out, double* load_out) try {
  return dispatch(on_context(ctx), plage_call({nullptr, nullptr, X, g, n, Gp, Gi, m}, tol, maxit, S_out, info_out, load_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plage_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                       const int32_t* Gp, const int32_t* Gi, int32_t m, double tol, int32_t maxit, double* S_out, double* info_out,
                       double* load_out) try {
  PH_REQUIRE(Xp != nullptr, "plage_csc: null Xp");
  return dispatch(on_context(ctx), plage_call({Xp, Xi, Xx, g, n, Gp, Gi, m}, tol, maxit, S_out, info_out, load_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_zscore(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                    double* S_out, double* size_out) try {
  return dispatch(on_context(ctx), zscore_call({nullptr, nullptr, X, g, n, Gp, Gi, m}, S_out, size_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_zscore_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out, double* size_out) try {
  PH_REQUIRE(Xp != nullptr, "zscore_csc: null Xp");
  return dispatch(on_context(ctx), zscore_call({Xp, Xi, Xx, g, n, Gp, Gi, m}, S_out, size_out));
} catch (...) { return plaidhip::on_exception(); }

// plaid.fisher: the one-device form of the sharded engine (shard_lists.cpp: fisher_worker, kFisher)
int plaidhip_fisher(plaidhip_ctx* ctx, const int8_t* sig, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m,
                    double* out, double* tot_out, int32_t* ov_len, int32_t* ov_idx) try {
  return dispatch(on_context(ctx), fisher_call(sig, g, c, Gp, Gi, m, out, tot_out, ov_len, ov_idx));
} catch (...) { return plaidhip::on_exception(); }

// plaid.limma: the one-device form of the sharded engine (shard_limma.cpp: limma_worker, kLimma)
int plaidhip_limma(plaidhip_ctx* ctx, const double* A, int32_t rows, int32_t n, const double* design, int32_t p, int32_t nfit,
                   const int8_t* use, const double* K, int32_t q, double* out, double* hyper) try {
  return dispatch(on_context(ctx), limma_call(A, rows, n, design, p, nfit, use, K, q, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_na(plaidhip_ctx* ctx, const double* A, int32_t rows, int32_t n, const double* design, int32_t p, int32_t nfit,
                      const int8_t* use, const double* K, int32_t q, double max_na, double* out, double* hyper,
                      double* dfres) try {
  return dispatch(on_context(ctx), limma_na_call(A, rows, n, design, p, nfit, use, K, q, max_na, out, hyper, dfres));
} catch (...) { return plaidhip::on_exception(); }

// the two device passes of plaid.limma on device pointers (kernels_lmfit.hip).  The workspace holds the block partials, then
// the masks, then (effects only) the tile weights.
static int dev_row_design_pass(plaidhip_ctx* ctx, const char* what, const double* A, int64_t ld, int32_t rows, int32_t n,
                               const double* Q, const int8_t* use, const double* invn, int32_t p, int32_t nfit, const double* E,
                               bool rss, const double* seed, double* out) {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && n >= 0 && ld >= rows && nfit >= 0 && nfit <= PLAIDHIP_LIMMA_MAX_FITS,
             "%s: bad shape rows=%d n=%d ld=%lld nfit=%d (nfit <= %d)", what, rows, n, (long long)ld, nfit, PLAIDHIP_LIMMA_MAX_FITS);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "%s: p = %d coefficients (1 <= p <= %d)", what, p, PLAIDHIP_LIMMA_MAX_COEF);
  PH_REQUIRE(n <= PLAIDHIP_LIMMA_MAX_SAMPLES, "%s: %d samples (at most %d)", what, n, PLAIDHIP_LIMMA_MAX_SAMPLES);
  if (rows == 0 || nfit == 0) return PLAIDHIP_OK;
  PH_REQUIRE(out && (!rss || E) && (n == 0 || (A && Q && (rss || invn))), "%s: null argument", what);
  const int64_t W = (int64_t)nfit * (p + 1), cols = rss ? nfit : W;
  const size_t part = ((size_t)row_design_ws_doubles(rows, n, cols) * 8 + 15) / 16 * 16;
  const size_t mb = (size_t)lmfit_mask_bytes(n, W);
  PH_TRY(ensure_workspace(ctx, part + mb + (rss ? 0 : (size_t)lmfit_weight_bytes(n, W))));
  double* ws = static_cast<double*>(ctx->ws);
  void* masks = static_cast<char*>(ctx->ws) + part;
  double* wt = rss ? nullptr : reinterpret_cast<double*>(static_cast<char*>(ctx->ws) + part + mb);   // (the RSS pass reads no weight)
  PH_TRY(launch_lmfit_masks(ctx, Q, use, invn, n, p, nfit, masks, wt));
  if (rss) PH_TRY(launch_row_design_rss(ctx, A, ld, rows, n, Q, masks, p, nfit, E, ws));
  else PH_TRY(launch_row_design_effects(ctx, A, ld, rows, n, masks, wt, (int32_t)W, ws));
  return launch_reduce_blocks_flat(ctx, ws, cols * rows, n, seed, out);
}

int plaidhip_dev_row_design_effects(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* Q,
                                    const int8_t* use, const double* invn, int32_t p, int32_t nfit, const double* seed,
                                    double* E) try {
  return dev_row_design_pass(ctx, "row_design_effects", A, ld, rows, n, Q, use, invn, p, nfit, nullptr, false, seed, E);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_row_design_rss(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* Q,
                                const int8_t* use, int32_t p, int32_t nfit, const double* E, const double* seed,
                                double* rss) try {
  return dev_row_design_pass(ctx, "row_design_rss", A, ld, rows, n, Q, use, nullptr, p, nfit, E, true, seed, rss);
} catch (...) { return plaidhip::on_exception(); }

// plaid.voom: the one-device form of the sharded engine (shard_voom.cpp: voom_worker, kVoom)
int plaidhip_voom(plaidhip_ctx* ctx, const double* counts, int32_t rows, int32_t n, const double* design, int32_t p,
                  const double* lib_size, double span, double* E, double* W, double* lib_out, double* offset, double* knots_x,
                  double* knots_y, int32_t* nknots) try {
  return dispatch(on_context(ctx),
                  voom_call(counts, rows, n, design, p, lib_size, span, E, W, lib_out, offset, knots_x, knots_y, nknots));
} catch (...) { return plaidhip::on_exception(); }

// plaid.voom's weights pass on device pointers (kernels_voom.hip), stream-ordered
int plaidhip_dev_voom_weights(plaidhip_ctx* ctx, const double* Q, const double* offset, int32_t n, int32_t p, const double* Eff,
                              int32_t rows, const double* knots_x, const double* knots_y, int32_t nknots, double* W,
                              int64_t ldw) try {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && n >= 0 && ldw >= rows, "voom_weights: bad shape rows=%d n=%d ldw=%lld", rows, n, (long long)ldw);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "voom_weights: p = %d coefficients (1 <= p <= %d)", p, PLAIDHIP_LIMMA_MAX_COEF);
  PH_REQUIRE(nknots >= 1 && nknots <= PLAIDHIP_VOOM_MAX_KNOTS, "voom_weights: %d knots (1 <= knots <= %d)", nknots,
             PLAIDHIP_VOOM_MAX_KNOTS);
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(Q && offset && Eff && knots_x && knots_y && W, "voom_weights: null argument");
  return launch_voom_weights(ctx, Q, offset, n, p, Eff, rows, knots_x, knots_y, nknots, W, ldw);
} catch (...) { return plaidhip::on_exception(); }

// plaid.limma with weights: the one-device form of the sharded engine (shard_limma_w.cpp: limma_w_worker)
int plaidhip_limma_w(plaidhip_ctx* ctx, const double* A, const double* Wt, const double* aw, int32_t rows, int32_t n,
                     const double* design, int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q, double max_na,
                     double* out, double* hyper, double* dfres) try {
  return dispatch(on_context(ctx), limma_w_call(A, Wt, aw, rows, n, design, p, nfit, use, K, q, max_na, out, hyper, dfres));
} catch (...) { return plaidhip::on_exception(); }

// the two device passes of the weighted fit on device pointers (kernels_lmfit_w.hip).  The workspace holds the block partials,
// then the masks, then the table of products; the counts' partials take the partials' place after the sums are reduced.
static int dev_limma_w_pass(plaidhip_ctx* ctx, const char* what, const double* A, const double* Wt, const double* aw, int64_t ld,
                            int32_t rows, int32_t n, const double* Q, const int8_t* use, const double* invn, int32_t p,
                            int32_t nfit, const double* G, bool rss, const double* seed, double* out, const double* seed_cnt,
                            double* cnt) {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && n >= 0 && ld >= rows && nfit >= 0 && nfit <= PLAIDHIP_LIMMA_MAX_FITS,
             "%s: bad shape rows=%d n=%d ld=%lld nfit=%d (nfit <= %d)", what, rows, n, (long long)ld, nfit, PLAIDHIP_LIMMA_MAX_FITS);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_NA_MAX_COEF, "%s: p = %d coefficients (1 <= p <= %d)", what, p,
             PLAIDHIP_LIMMA_NA_MAX_COEF);
  PH_REQUIRE(n <= PLAIDHIP_LIMMA_MAX_SAMPLES, "%s: %d samples (at most %d)", what, n, PLAIDHIP_LIMMA_MAX_SAMPLES);
  const int64_t W = (int64_t)nfit * lmfit_w_columns(p), C = 2 * (int64_t)nfit + 1, cols = rss ? nfit : std::max(W, C);
  PH_REQUIRE(lmfit_tiles(W) <= 65535, "%s: %lld tiles of weight columns (at most 65535)", what, (long long)lmfit_tiles(W));
  if (rows == 0 || nfit == 0) return PLAIDHIP_OK;
  PH_REQUIRE(out && (!rss || G) && (n == 0 || (A && Q && (rss || invn))), "%s: null argument", what);
  const size_t part = ((size_t)row_design_ws_doubles(rows, n, cols) * 8 + 15) / 16 * 16;
  const size_t mb = (size_t)lmfit_mask_bytes(n, W);
  PH_TRY(ensure_workspace(ctx, part + mb + (size_t)lmfit_weight_bytes(n, W)));
  double* ws = static_cast<double*>(ctx->ws);
  void* masks = static_cast<char*>(ctx->ws) + part;
  double* wt = reinterpret_cast<double*>(static_cast<char*>(ctx->ws) + part + mb);
  PH_TRY(launch_lmfit_w_table(ctx, Q, use, invn, n, p, nfit, masks, wt));   // (the RSS pass reads the masks alone: invn may be null)
  if (rss) {
    PH_TRY(launch_row_design_w_rss(ctx, A, Wt, aw, ld, rows, n, Q, masks, p, nfit, G, ws));
    return launch_reduce_blocks_flat(ctx, ws, (int64_t)nfit * rows, n, seed, out);
  }
  PH_TRY(launch_row_design_w_sums(ctx, A, Wt, aw, ld, rows, n, masks, wt, p, nfit, ws));
  PH_TRY(launch_reduce_blocks_flat(ctx, ws, W * rows, n, seed, out));
  if (cnt == nullptr) return PLAIDHIP_OK;
  PH_TRY(launch_lmfit_w_counts(ctx, A, Wt, aw, ld, rows, n, use, nfit, ws));
  return launch_reduce_blocks_flat(ctx, ws, C * rows, n, seed_cnt, cnt);
}

int plaidhip_dev_limma_w_sums(plaidhip_ctx* ctx, const double* A, const double* Wt, const double* aw, int64_t ld, int32_t rows,
                              int32_t n, const double* Q, const int8_t* use, const double* invn, int32_t p, int32_t nfit,
                              const double* seed, double* S, const double* seed_cnt, double* cnt) try {
  return dev_limma_w_pass(ctx, "limma_w_sums", A, Wt, aw, ld, rows, n, Q, use, invn, p, nfit, nullptr, false, seed, S, seed_cnt,
                          cnt);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_limma_w_rss(plaidhip_ctx* ctx, const double* A, const double* Wt, const double* aw, int64_t ld, int32_t rows,
                             int32_t n, const double* Q, const int8_t* use, int32_t p, int32_t nfit, const double* G,
                             const double* seed, double* rss) try {
  return dev_limma_w_pass(ctx, "limma_w_rss", A, Wt, aw, ld, rows, n, Q, use, nullptr, p, nfit, G, true, seed, rss, nullptr,
                          nullptr);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_tile(void) { return PLAIDHIP_LIMMA_TILE; }

// plaid.camera: the one-device form of the sharded engine (shard_limma.cpp: limma_worker with kCamera, camera_tail)
int plaidhip_camera(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit,
                    const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                    double inter_gene_cor, int allow_neg_cor, double* out, double* hyper) try {
  return dispatch(on_context(ctx),
                  camera_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, inter_gene_cor, allow_neg_cor, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

// the two device passes of plaid.camera on device pointers (kernels_camera.hip).  The workspace holds the masks of the
// residual pass, or the block partials of the sums of squares.
int plaidhip_dev_camera_residuals(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* Q,
                                  const int8_t* use, int32_t p, int32_t nfit, int32_t fit, const double* E, const double* rss,
                                  double d, double* Z, int64_t ldz) try {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && n >= 0 && ld >= rows && ldz >= rows && nfit >= 0 && nfit <= PLAIDHIP_LIMMA_MAX_FITS,
             "camera_residuals: bad shape rows=%d n=%d ld=%lld ldz=%lld nfit=%d (nfit <= %d)", rows, n, (long long)ld,
             (long long)ldz, nfit, PLAIDHIP_LIMMA_MAX_FITS);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "camera_residuals: p = %d coefficients (1 <= p <= %d)", p,
             PLAIDHIP_LIMMA_MAX_COEF);
  PH_REQUIRE(n <= PLAIDHIP_LIMMA_MAX_SAMPLES, "camera_residuals: %d samples (at most %d)", n, PLAIDHIP_LIMMA_MAX_SAMPLES);
  PH_REQUIRE(fit >= 0 && fit < nfit, "camera_residuals: fit %d of %d", fit, nfit);
  PH_REQUIRE(d >= 1.0, "camera_residuals: d = %g residual degrees of freedom (at least 1)", d);
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(A && Q && E && rss && Z, "camera_residuals: null argument");
  const int64_t W = (int64_t)nfit * (p + 1);
  PH_TRY(ensure_workspace(ctx, (size_t)lmfit_mask_bytes(n, W)));
  PH_TRY(launch_lmfit_masks(ctx, Q, use, nullptr, n, p, nfit, ctx->ws, nullptr));
  return launch_camera_residuals(ctx, A, ld, rows, n, Q, ctx->ws, p, fit, E, rss, d, Z, ldz);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_camera_sumsq(plaidhip_ctx* ctx, const double* T, int64_t ldt, int32_t m, int32_t n, const double* seed,
                              double* out) try {
  PH_CTX(ctx);
  PH_REQUIRE(m >= 0 && n >= 0 && ldt >= m && n <= PLAIDHIP_LIMMA_MAX_SAMPLES, "camera_sumsq: bad shape m=%d n=%d ldt=%lld (n <= %d)",
             m, n, (long long)ldt, PLAIDHIP_LIMMA_MAX_SAMPLES);
  if (m == 0) return PLAIDHIP_OK;
  PH_REQUIRE(out && (n == 0 || T), "camera_sumsq: null argument");
  PH_TRY(ensure_workspace(ctx, (size_t)camera_sumsq_ws_doubles(n, m) * 8));
  double* ws = static_cast<double*>(ctx->ws);
  PH_TRY(launch_camera_sumsq(ctx, T, ldt, m, n, ws, m));
  return launch_reduce_blocks_flat(ctx, ws, m, n, seed, out);
} catch (...) { return plaidhip::on_exception(); }

// plaid.fry: the one-device form of the sharded engine (shard_limma.cpp: limma_worker with kFry, fry_tail)
int plaidhip_fry(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit,
                 const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                 int standardize, double* out, double* hyper) try {
  return dispatch(on_context(ctx), fry_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, standardize, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

// the device passes of plaid.fry on device pointers (kernels_fry.hip; the residual effects are kernels_lmfit.hip's effects
// pass with Q2 for Q).  The workspace holds the masks of the residual pass; the block partials, masks and tile weights of
// the effects pass.
int plaidhip_dev_fry_residuals(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* Q,
                               const int8_t* use, int32_t p, int32_t nfit, int32_t fit, const double* E, const double* cg,
                               double* Z, int64_t ldz) try {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && n >= 0 && ld >= rows && ldz >= rows && nfit >= 0 && nfit <= PLAIDHIP_LIMMA_MAX_FITS,
             "fry_residuals: bad shape rows=%d n=%d ld=%lld ldz=%lld nfit=%d (nfit <= %d)", rows, n, (long long)ld,
             (long long)ldz, nfit, PLAIDHIP_LIMMA_MAX_FITS);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "fry_residuals: p = %d coefficients (1 <= p <= %d)", p,
             PLAIDHIP_LIMMA_MAX_COEF);
  PH_REQUIRE(n <= PLAIDHIP_LIMMA_MAX_SAMPLES, "fry_residuals: %d samples (at most %d)", n, PLAIDHIP_LIMMA_MAX_SAMPLES);
  PH_REQUIRE(fit >= 0 && fit < nfit, "fry_residuals: fit %d of %d", fit, nfit);
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(A && Q && E && cg && Z, "fry_residuals: null argument");
  const int64_t W = (int64_t)nfit * (p + 1);
  PH_TRY(ensure_workspace(ctx, (size_t)lmfit_mask_bytes(n, W)));
  PH_TRY(launch_lmfit_masks(ctx, Q, use, nullptr, n, p, nfit, ctx->ws, nullptr));
  return launch_fry_residuals(ctx, A, ld, rows, n, Q, ctx->ws, p, fit, E, cg, Z, ldz);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_fry_residual_effects(plaidhip_ctx* ctx, const double* Z, int64_t ldz, int32_t rows, int32_t n,
                                      const double* Q2, const int8_t* use, int32_t d, const double* seed, double* rho) try {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && n >= 0 && ldz >= rows && n <= PLAIDHIP_LIMMA_MAX_SAMPLES,
             "fry_residual_effects: bad shape rows=%d n=%d ldz=%lld (n <= %d)", rows, n, (long long)ldz,
             PLAIDHIP_LIMMA_MAX_SAMPLES);
  PH_REQUIRE(d >= 1 && d + 1 <= PLAIDHIP_FRY_MIXED_MAX, "fry_residual_effects: d = %d residual effects (1 <= d <= %d)", d,
             PLAIDHIP_FRY_MIXED_MAX - 1);
  if (rows == 0) return PLAIDHIP_OK;
  PH_REQUIRE(rho && (n == 0 || (Z && Q2)), "fry_residual_effects: null argument");
  const int64_t W = d + 1;   // (the effects pass's mean column: weight 0.0 here)
  const size_t part = ((size_t)row_design_ws_doubles(rows, n, W) * 8 + 15) / 16 * 16;
  const size_t mb = (size_t)lmfit_mask_bytes(n, W);
  PH_TRY(ensure_workspace(ctx, part + mb + (size_t)lmfit_weight_bytes(n, W)));
  DevBuf dzero;
  PH_TRY(dzero.alloc(8));
  PH_HIP(hipMemsetAsync(dzero.p, 0, 8, ctx->stream));
  double* ws = static_cast<double*>(ctx->ws);
  void* masks = static_cast<char*>(ctx->ws) + part;
  double* wt = reinterpret_cast<double*>(static_cast<char*>(ctx->ws) + part + mb);
  PH_TRY(launch_lmfit_masks(ctx, Q2, use, dzero.as<double>(), n, d, 1, masks, wt));
  PH_TRY(launch_row_design_effects(ctx, Z, ldz, rows, n, masks, wt, (int32_t)W, ws));
  PH_TRY(launch_reduce_blocks_flat(ctx, ws, W * rows, n, seed, rho));
  PH_HIP(hipStreamSynchronize(ctx->stream));   // (dzero is released on return)
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_fry_gram(plaidhip_ctx* ctx, const double* rho, const double* e, int32_t rows, int32_t d, int32_t q,
                          const int32_t* Gp, const int32_t* Gi, int32_t m, double* C, double* b, double* a, double* tr,
                          double* fro) try {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && m >= 0, "fry_gram: bad dims rows=%d m=%d", rows, m);
  PH_REQUIRE(d >= 1 && d + 1 <= PLAIDHIP_FRY_MIXED_MAX, "fry_gram: d = %d residual effects (1 <= d <= %d)", d,
             PLAIDHIP_FRY_MIXED_MAX - 1);
  PH_REQUIRE(q >= 1 && q <= PLAIDHIP_FRY_MAX_CONTRASTS, "fry_gram: q = %d contrasts (1 <= q <= %d)", q,
             PLAIDHIP_FRY_MAX_CONTRASTS);
  if (m == 0) return PLAIDHIP_OK;
  PH_REQUIRE(rho && e && Gp && Gi && C && b && a && tr && fro, "fry_gram: null argument");
  return launch_fry_gram(ctx, rho, e, d, q, Gp, Gi, 0, m, C, b, a, tr, fro);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_fry_eigen(plaidhip_ctx* ctx, const double* M, int32_t dim, int64_t nprob, const int32_t* Dk, double* lam1,
                           double* lamD, int32_t* sweeps, int32_t* converged) try {
  PH_CTX(ctx);
  PH_REQUIRE(dim >= 1 && dim <= PLAIDHIP_FRY_MIXED_MAX, "fry_eigen: dim = %d (1 <= dim <= %d)", dim, PLAIDHIP_FRY_MIXED_MAX);
  PH_REQUIRE(nprob >= 0 && nprob <= 0x7fffffff, "fry_eigen: %lld problems", (long long)nprob);
  if (nprob == 0) return PLAIDHIP_OK;
  PH_REQUIRE(M && Dk && lam1 && lamD && sweeps && converged, "fry_eigen: null argument");
  return launch_fry_eigen(ctx, M, nullptr, nullptr, nullptr, dim, 1, nprob, Dk, lam1, lamD, sweeps, converged);
} catch (...) { return plaidhip::on_exception(); }

// plaid.roast: the one-device form of the sharded engine (shard_limma.cpp: limma_worker with kRoast, roast_tail)
int plaidhip_roast(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit,
                   const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                   int set_statistic, int zscore, int32_t nrot, uint64_t seed, int midp, const double* rotations, double* out,
                   double* hyper) try {
  return dispatch(on_context(ctx), roast_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, set_statistic, zscore, nrot, seed,
                                              midp, rotations, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

// plaid.romer: the one-device form of the sharded engine (shard_romer.cpp: romer_worker, romer_tail)
int plaidhip_romer(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit,
                   const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                   int set_statistic, int32_t nrot, uint64_t seed, int shrink_resid, const double* shrink, const double* rotations,
                   double* out, double* hyper) try {
  return dispatch(on_context(ctx), romer_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, set_statistic, nrot, seed,
                                              shrink_resid, shrink, rotations, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

// the device passes of plaid.romer on device pointers (kernels_romer.hip); chunk: rotations per launch (a multiple of 64; 0: all)
static int romer_dev_dims(const char* who, int32_t U, int64_t ldu, int set_statistic, int32_t nrot, int32_t chunk) {
  PH_REQUIRE(U >= 0 && U <= PLAIDHIP_ROMER_MAX_GENES && ldu >= U, "%s: U = %d keys a column, ldu = %lld (U <= %d)", who, U,
             (long long)ldu, PLAIDHIP_ROMER_MAX_GENES);
  PH_REQUIRE(set_statistic >= 0 && set_statistic <= 2, "%s: set_statistic = %d (0 mean, 1 floormean, 2 mean50)", who, set_statistic);
  PH_REQUIRE(nrot >= 1 && nrot <= PLAIDHIP_ROAST_MAX_ROTATIONS, "%s: nrot = %d (1 <= nrot <= %d)", who, nrot,
             PLAIDHIP_ROAST_MAX_ROTATIONS);
  PH_REQUIRE(chunk >= 0 && chunk % 64 == 0, "%s: chunk = %d rotations (a multiple of 64, or 0: all)", who, chunk);
  return PLAIDHIP_OK;
}

int plaidhip_dev_romer_keys(plaidhip_ctx* ctx, const double* Z, int32_t rows, const int32_t* uidx, int32_t U, int64_t ldu,
                            int set_statistic, int32_t nrot, int32_t chunk, double* Ka, double* Kb, double* Kc, uint32_t* flag) try {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && U <= rows, "romer_keys: rows = %d, U = %d", rows, U);
  PH_TRY(romer_dev_dims("romer_keys", U, ldu, set_statistic, nrot, chunk));
  if (U == 0) return PLAIDHIP_OK;
  PH_REQUIRE(Z && uidx && Ka && Kc && (Kb || set_statistic != PLAIDHIP_ROMER_STAT_FLOORMEAN), "romer_keys: null argument");
  const int32_t step = chunk == 0 ? (nrot + 63) / 64 * 64 : chunk;
  for (int32_t k0 = 0; k0 < nrot; k0 += step) {
    const int64_t off = (int64_t)k0 * ldu;
    PH_TRY(launch_romer_keys(ctx, Z + (size_t)(k0 / 64) * rows * 64, rows, uidx, U, ldu, set_statistic, std::min(nrot - k0, step),
                             Ka + off, Kb ? Kb + off : nullptr, Kc + off, flag));
  }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_romer_sides(plaidhip_ctx* ctx, const double* Ra, const double* Rb, const double* Rc, int64_t ldu, int32_t U,
                             const int32_t* Gp, const int32_t* Gi, int32_t m, int set_statistic, int32_t nrot, int32_t chunk,
                             int64_t* stat, const int64_t* obs, int32_t* cnt) try {
  PH_CTX(ctx);
  PH_REQUIRE(m >= 0, "romer_sides: bad dims m=%d", m);
  PH_TRY(romer_dev_dims("romer_sides", U, ldu, set_statistic, nrot, chunk));
  PH_REQUIRE((obs == nullptr) == (cnt == nullptr), "romer_sides: obs and cnt go together");
  if (m == 0 || U == 0) return PLAIDHIP_OK;
  PH_REQUIRE(Ra && Rc && (Rb || set_statistic != PLAIDHIP_ROMER_STAT_FLOORMEAN) && Gp && Gi && (stat || cnt),
             "romer_sides: null argument");
  const int32_t step = chunk == 0 ? nrot : chunk;
  int32_t cls_cnt[2] = {0, 0};
  DevBuf dsel, dS;
  std::vector<int32_t> gp((size_t)m + 1), gi, sel;
  plaidhip_geneset* gs = nullptr;
  PH_HIP(hipMemcpyAsync(gp.data(), Gp, ((size_t)m + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  if (set_statistic == PLAIDHIP_ROMER_STAT_MEAN50) {   // the size classes need the set sizes on the host
    romer_mean50_classes(gp.data(), m, sel, cls_cnt);
    PH_TRY(dsel.alloc((size_t)m * 4));
    if (!sel.empty()) PH_HIP(hipMemcpyAsync(dsel.p, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  } else {                                             // the rank crossprod needs the prepared collection
    PH_REQUIRE(gp[0] == 0 && gp[(size_t)m] >= 0, "romer_sides: Gp[0] = %d, Gp[m] = %d", gp[0], gp[(size_t)m]);
    gi.resize((size_t)gp[(size_t)m] + 1);
    if (gp[(size_t)m] > 0) PH_HIP(hipMemcpy(gi.data(), Gi, (size_t)gp[(size_t)m] * 4, hipMemcpyDeviceToHost));
    PH_TRY(plaidhip_geneset_create(ctx, U, m, gp.data(), gi.data(), &gs));
    if (dS.alloc((size_t)romer_nkeys(set_statistic) * m * std::min(nrot, step) * 8) != PLAIDHIP_OK) {
      plaidhip_geneset_destroy(gs);
      return PLAIDHIP_ENOMEM;
    }
  }
  const int saved = ctx->precision;
  ctx->precision = PLAIDHIP_PRECISION_F64;
  int rc = PLAIDHIP_OK;
  for (int32_t k0 = 0; k0 < nrot && rc == PLAIDHIP_OK; k0 += step) {
    const int64_t off = (int64_t)k0 * ldu;
    rc = launch_romer_sides(ctx, gs, Ra + off, Rb ? Rb + off : nullptr, Rc + off, ldu, U, Gp, Gi, m, set_statistic,
                            std::min(nrot - k0, step), k0, nrot, dsel.as<int32_t>(), cls_cnt, dS.as<double>(), stat, obs, cnt);
  }
  ctx->precision = saved;
  hipStreamSynchronize(ctx->stream);   // (dsel, dS and the collection are released on return)
  if (gs != nullptr) plaidhip_geneset_destroy(gs);
  return rc;
} catch (...) { return plaidhip::on_exception(); }

// the device passes of plaid.roast on device pointers (kernels_roast.hip)
int plaidhip_dev_roast_rotate(plaidhip_ctx* ctx, const double* Rz, int64_t ldz, int32_t rows, int32_t n, const double* beta,
                              const double* rss, const double* W, int64_t ldw, int32_t nrot, double d, double df0, double s02,
                              int zscore, int32_t chunk, double* Z) try {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && n >= 0 && ldz >= rows && n <= PLAIDHIP_LIMMA_MAX_SAMPLES,
             "roast_rotate: bad shape rows=%d n=%d ldz=%lld (n <= %d)", rows, n, (long long)ldz, PLAIDHIP_LIMMA_MAX_SAMPLES);
  PH_REQUIRE(nrot >= 1 && nrot <= PLAIDHIP_ROAST_MAX_ROTATIONS, "roast_rotate: nrot = %d (1 <= nrot <= %d)", nrot,
             PLAIDHIP_ROAST_MAX_ROTATIONS);
  PH_REQUIRE(ldw % 16 == 0 && ldw >= nrot, "roast_rotate: ldw = %lld (a multiple of 16, at least nrot = %d)", (long long)ldw, nrot);
  PH_REQUIRE(chunk >= 0 && chunk % 64 == 0, "roast_rotate: chunk = %d rotations (a multiple of 64, or 0: all)", chunk);
  PH_REQUIRE(zscore >= 0 && zscore <= 1, "roast_rotate: zscore = %d (0 hill, 1 none)", zscore);
  PH_REQUIRE(d >= 1.0, "roast_rotate: df.residual = %g", d);
  if (rows == 0) return PLAIDHIP_OK;
  PH_REQUIRE(beta && rss && W && Z && (n == 0 || Rz), "roast_rotate: null argument");
  const RoastFit rf = roast_fit(d, df0, s02);
  const int32_t step = chunk == 0 ? (nrot + 63) / 64 * 64 : chunk;
  for (int32_t k0 = 0; k0 < nrot; k0 += step)
    PH_TRY(launch_roast_rotate(ctx, Rz, ldz, rows, n, beta, rss, W, ldw, k0, std::min(nrot, k0 + step), rf, zscore,
                               Z + (size_t)(k0 / 64) * rows * 64));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_roast_stats(plaidhip_ctx* ctx, const double* Z, int32_t rows, const int32_t* Gp, const int32_t* Gi, int32_t m,
                             int set_statistic, int32_t nrot, double* stat, const double* obs, int32_t* cnt) try {
  PH_CTX(ctx);
  PH_REQUIRE(rows >= 0 && m >= 0, "roast_stats: bad dims rows=%d m=%d", rows, m);
  PH_REQUIRE(set_statistic >= 0 && set_statistic <= 3, "roast_stats: set_statistic = %d (0 mean, 1 floormean, 2 msq, 3 mean50)",
             set_statistic);
  PH_REQUIRE(nrot >= 1 && nrot <= PLAIDHIP_ROAST_MAX_ROTATIONS, "roast_stats: nrot = %d (1 <= nrot <= %d)", nrot,
             PLAIDHIP_ROAST_MAX_ROTATIONS);
  PH_REQUIRE((obs == nullptr) == (cnt == nullptr), "roast_stats: obs and cnt go together");
  if (m == 0) return PLAIDHIP_OK;
  PH_REQUIRE(Z && Gp && Gi && (stat || cnt), "roast_stats: null argument");
  int32_t cls_cnt[3] = {0, 0, 0};
  DevBuf dsel;
  std::vector<int32_t> gp, sel;
  if (set_statistic == PLAIDHIP_ROAST_STAT_MEAN50) {   // the size classes need the set sizes on the host
    gp.resize((size_t)m + 1);
    sel.resize((size_t)m);
    PH_HIP(hipMemcpyAsync(gp.data(), Gp, ((size_t)m + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    size_t at = 0;
    for (int cls = 0; cls < 3; ++cls)
      for (int32_t s = 0; s < m; ++s)
        if (roast_mean50_class(gp[(size_t)s + 1] - gp[(size_t)s]) == cls) {
          sel[at++] = s;
          ++cls_cnt[cls];
        }
    PH_TRY(dsel.alloc((size_t)m * 4));
    PH_HIP(hipMemcpyAsync(dsel.p, sel.data(), (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  PH_TRY(launch_roast_stats(ctx, Z, rows, Gp, Gi, m, set_statistic, 0, nrot, nrot, dsel.as<int32_t>(), cls_cnt, stat, obs, cnt));
  PH_HIP(hipStreamSynchronize(ctx->stream));   // (dsel is released on return)
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// the generated placements of plaid.gsea themselves, slab by slab as gsea_worker generates them
int plaidhip_gsea_permutations(plaidhip_ctx* ctx, int32_t g, int32_t nperm, uint64_t seed, int32_t* P_out) try {
  PH_REQUIRE(g >= 1 && nperm >= 1, "gsea_permutations: bad dims g=%d nperm=%d", g, nperm);
  if (g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("gsea_permutations: %d genes (at most %d)", g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(P_out != nullptr, "gsea_permutations: null P_out");
  PH_CTX(ctx);
  const int32_t slab = std::min(nperm, gsea_slab_perms(g));
  DevBuf dY, dR, dP;
  PH_TRY(dY.alloc((size_t)g * slab * 8));
  PH_TRY(dR.alloc((size_t)g * slab * 8));
  PH_TRY(dP.alloc((size_t)g * slab * 4));
  for (int64_t b0 = 0; b0 < nperm; b0 += slab) {
    const int32_t nb = (int32_t)std::min<int64_t>(slab, nperm - b0);
    PH_TRY(launch_gsea_placements(ctx, g, b0, nb, seed, dY.as<double>(), dR.as<double>(), dP.as<int32_t>()));
    PH_HIP(hipMemcpyAsync(P_out + b0 * g, dP.p, (size_t)g * nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
  }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// GSVA's Gaussian kernel CDF estimate alone (the row transform "gauss" of replaid.gsva.exact): V, g x n
int plaidhip_gsva_kcdf(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                       double* V_out) try {
  PH_REQUIRE(g >= 0 && n >= 0, "gsva_kcdf: bad dims g=%d n=%d", g, n);
  PH_REQUIRE(n >= 2, "gsva_kcdf: the kernel CDF estimate needs at least 2 samples (got %d)", n);
  PH_REQUIRE(X_or_x != nullptr || g == 0 || (Xp != nullptr && Xp[n] == 0), "null X");
  if (Xp != nullptr) PH_TRY(check_host_csc(Xp, Xi, g, n));
  if (g == 0) return PLAIDHIP_OK;
  PH_REQUIRE(V_out != nullptr, "null V_out");
  PH_CTX(ctx);
  DevBuf dV;
  PH_TRY(dV.alloc((size_t)g * n * 8));
  PH_TRY(gsva_kcdf_columns(ctx, Xp, Xi, X_or_x, g, n, 0, n, dV.as<double>()));
  return copy_home(ctx, V_out, dV.p, (size_t)g * n * 8);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsva_kcdf_table(double* out) try {
  PH_REQUIRE(out != nullptr, "gsva_kcdf_table: null out");
  gsva_kcdf_table(out);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// Test hooks (not part of include/plaidhip.h): how kcdf_sum_kernel finds its table index (0 the fast index, 1 the exact
// operations for every term, 2 the fast index with the terms it left to the exact operations counted), and that count
int plaidhip_debug_gsva_kcdf_set_mode(int mode) try {
  PH_REQUIRE(mode >= 0 && mode <= 2, "debug_gsva_kcdf_set_mode: mode = %d", mode);
  debug_gsva_kcdf_set_mode(mode);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_gsva_kcdf_width(int32_t nj) { return nj >= 1 ? debug_gsva_kcdf_width(nj) : 0; }

// the bandwidths h of the rows of a dense host matrix X (g x n), as the kernel CDF estimate computes them: H_out, g doubles
int plaidhip_debug_gsva_kcdf_bandwidths(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, double* H_out) try {
  PH_REQUIRE(g >= 1 && n >= 2 && X != nullptr && H_out != nullptr, "debug_gsva_kcdf_bandwidths: bad arguments");
  PH_CTX(ctx);
  DevBuf dX, dH;
  PH_TRY(dX.alloc((size_t)g * n * 8));
  PH_TRY(dH.alloc((size_t)g * 8));
  PH_TRY(upload_host(ctx, dX.p, (size_t)g * 8, X, (size_t)g * 8, n));
  PH_TRY(launch_gsva_kcdf_bandwidths(ctx, dX.as<double>(), g, g, n, dH.as<double>()));
  PH_HIP(hipMemcpyAsync(H_out, dH.p, (size_t)g * 8, hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_gsva_kcdf_slow_terms(unsigned long long* out) try {
  PH_REQUIRE(out != nullptr, "debug_gsva_kcdf_slow_terms: null out");
  *out = debug_gsva_kcdf_slow_terms();
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// replaid.sing.exact: the one-device form of the sharded engine (shard_exact.cpp: sing_exact_worker)
int plaidhip_sing_exact(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                        const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di, int32_t m, int center,
                        double* total, double* up, double* down, double* total_disp, double* up_disp, double* down_disp) try {
  return dispatch(on_context(ctx), sing_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Dp, Di, center, total, up, down, total_disp, up_disp,
                                                   down_disp));
} catch (...) { return plaidhip::on_exception(); }

// replaid.ucell.exact / replaid.aucell.exact: the one-device forms of the sharded engine (shard_exact.cpp: truncated_exact_worker)
int plaidhip_ucell_exact(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                         const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di, int32_t m, double max_rank,
                         double w_neg, int impute, const double* k_full, const double* k_full_down, double* total, double* up,
                         double* down) try {
  PH_REQUIRE(!impute || k_full != nullptr || m == 0, "ucell_exact: impute needs k_full");
  return dispatch(on_context(ctx), ucell_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Dp, Di, max_rank, w_neg,
                                                    impute ? k_full : nullptr, impute ? k_full_down : nullptr, total, up, down));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_aucell_exact(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                          const int32_t* Gp, const int32_t* Gi, int32_t m, double auc_max_rank, double* S_out) try {
  return dispatch(on_context(ctx), aucell_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, auc_max_rank, S_out));
} catch (...) { return plaidhip::on_exception(); }

// the truncated-rank stage on device operands (kernels_trunc.hip), stream-ordered
static int check_truncated_dev(const char* who, int32_t g, int32_t n, int mode, int64_t T) {
  PH_REQUIRE(g > 0 && n >= 0 && g < (1 << 26), "%s: bad dims g=%d n=%d (at most 2^26 - 1 rows)", who, g, n);
  PH_REQUIRE(mode == PLAIDHIP_TRUNC_UCELL || mode == PLAIDHIP_TRUNC_AUCELL, "%s: bad mode %d", who, mode);
  PH_REQUIRE(T >= 1 && T <= g, "%s: T = %lld outside 1..%d", who, (long long)T, g);
  return PLAIDHIP_OK;
}

int plaidhip_dev_truncated_ranks_f64(plaidhip_ctx* ctx, const void* X, int64_t ldx, int32_t g, int32_t n, int mode, int64_t T,
                                     void* R_scratch, void* colnan, void* counts, void* Wp, void* Wi, void* Wx,
                                     int64_t capacity) try {
  PH_CTX(ctx);
  PH_TRY(check_truncated_dev("truncated_ranks", g, n, mode, T));
  PH_REQUIRE(ldx >= g, "truncated_ranks: ldx = %lld < g", (long long)ldx);
  if (n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(X && R_scratch && colnan && counts && Wp && Wi && Wx, "truncated_ranks: null X/R_scratch/colnan/counts/Wp/Wi/Wx");
  const int64_t need = truncated_bound(mode, T, g, g, false) * n;
  PH_REQUIRE(capacity >= need && need < ((int64_t)1 << 31), "truncated_ranks: capacity %lld, the columns may take %lld entries",
             (long long)capacity, (long long)need);
  return truncated_ranks_stage(ctx, mode, T, static_cast<const double*>(X), ldx, nullptr, nullptr, g, n, 0, 0,
                               static_cast<double*>(R_scratch), static_cast<uint32_t*>(colnan), static_cast<int32_t*>(counts),
                               static_cast<int32_t*>(Wp), static_cast<int32_t*>(Wi), static_cast<double*>(Wx), capacity, nullptr);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_dev_truncated_ranks_csc_f64(plaidhip_ctx* ctx, const void* Xp, const void* Xi, const void* Xx, int32_t g, int32_t n,
                                         int32_t max_col_nnz, int64_t nnz, int mode, int64_t T, void* scratch, void* colnan,
                                         void* counts, void* u0, void* Wp, void* Wi, void* Wx, int64_t capacity) try {
  PH_CTX(ctx);
  PH_TRY(check_truncated_dev("truncated_ranks_csc", g, n, mode, T));
  PH_REQUIRE(max_col_nnz >= 0 && max_col_nnz <= g && nnz >= 0, "truncated_ranks_csc: max_col_nnz = %d, nnz = %lld", max_col_nnz,
             (long long)nnz);
  if (n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(Xp && (nnz == 0 || (Xi && Xx)) && scratch && colnan && counts && u0 && Wp && Wi && Wx,
             "truncated_ranks_csc: null Xp/Xi/Xx/scratch/colnan/counts/u0/Wp/Wi/Wx");
  const int64_t need = mode == PLAIDHIP_TRUNC_UCELL ? nnz : truncated_bound(mode, T, g, 0, true) * n;
  PH_REQUIRE(capacity >= need && need < ((int64_t)1 << 31), "truncated_ranks_csc: capacity %lld, the columns may take %lld entries",
             (long long)capacity, (long long)need);
  if (mode == PLAIDHIP_TRUNC_AUCELL) PH_HIP(hipMemsetAsync(u0, 0, (size_t)n * 8, ctx->stream));
  return truncated_ranks_stage(ctx, mode, T, static_cast<const double*>(Xx), 0, static_cast<const int32_t*>(Xp),
                               static_cast<const int32_t*>(Xi), g, n, max_col_nnz, nnz, static_cast<double*>(scratch),
                               static_cast<uint32_t*>(colnan), static_cast<int32_t*>(counts), static_cast<int32_t*>(Wp),
                               static_cast<int32_t*>(Wi), static_cast<double*>(Wx), capacity, static_cast<double*>(u0));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsva(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi,
                  int32_t m, double tau, int rowtf, double* S_out) try {
  return dispatch(on_context(ctx), gsva_call({nullptr, nullptr, X, g, n, Gp, Gi, m}, tau, rowtf, S_out));
} catch (...) { return plaidhip::on_exception(); }

// dgCMatrix input for replaid.gsva and plaid.test: the slots go to the device as they are, where their row view
// (kernels_csr.hip) gives the rows' moments, ecdf counts and group sums; no dense X on the host or the link
int plaidhip_gsva_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                      const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf, double* S_out) try {
  PH_REQUIRE(Xp != nullptr, "gsva_csc: null Xp");
  return dispatch(on_context(ctx), gsva_call({Xp, Xi, Xx, g, n, Gp, Gi, m}, tau, rowtf, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plaid_test_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                            const int32_t* y, const int32_t* Gp, const int32_t* Gi, int32_t m, const double* gsetX,
                            int tests, int metap_method, double* out) try {
  PH_REQUIRE(Xp != nullptr, "plaid_test: null X / y");
  return dispatch(on_context(ctx), plaid_test_call({Xp, Xi, Xx, g, n, Gp, Gi, m}, y, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

}  // extern "C"
