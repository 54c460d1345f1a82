// GSVA's Gaussian kernel CDF estimate, the row transform "gauss" of replaid.gsva.exact (include/plaidhip.h:
// plaidhip_gsva_kcdf pins every operation).  Per gene the work grows with n^2:
//
//   kcdf_row_moments_kernel   h = sd / 4 of every gene, one thread per gene walking the samples in order
//   kcdf_sum_kernel           V_ij = sum_k c(x_ij - x_ik) over all n samples in order, for a range of test columns j
//
// The sums are sequential in sample order and no product is contracted into an add (fp contraction is off for the whole
// file; the divisions and the square root expand to their correctly rounded sequences, which use fused operations of their own).
// Vector stores only.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <mutex>

#include "common.h"

#pragma clang fp contract(off)

namespace plaidhip {

namespace {

constexpr int kKcdfTable = PLAIDHIP_GSVA_KCDF_TABLE;   // 10,001 values of Phi on [0, 10]
constexpr int kKcdfThreads = 1024;                     // one workgroup per CU: the table takes 80,008 B of its LDS
// LDS of kcdf_sum_kernel: the table, then two buffers of kKcdfThreads staged samples
constexpr size_t kKcdfLds = (size_t)kKcdfTable * 8 + 2 * (size_t)kKcdfThreads * 8;
// the fast index leaves a term to the exact operations when its estimate lies this close to an integer (the estimate and
// the pinned value each carry three roundings: they differ by less than 1e-11 below 10,000.5)
constexpr double kKcdfSeam = 1.0 / 1048576.0;

std::atomic<int> g_kcdf_mode{0};                        // test hook: 0 fast index | 1 exact operations only | 2 fast, counting
std::atomic<unsigned long long> g_kcdf_slow_terms{0};   // mode 2: terms of the last launch that took the exact operations

// Phi on the grid of the table, built once on the host
const double* kcdf_host_table() {
  static double table[kKcdfTable];
  static std::once_flag once;
  std::call_once(once, [] {
    for (int i = 0; i < kKcdfTable; ++i) {
      const double t = 10.0 * (double)i / 10000.0;
      table[i] = 0.5 * std::erfc(-t / std::sqrt(2.0));
      if (i > 0 && table[i] < table[i - 1]) table[i] = table[i - 1];   // (a libm whose erfc wobbles in the last bit)
    }
  });
  return table;
}

__global__ void __launch_bounds__(256)
kcdf_row_moments_kernel(const double* __restrict__ X, int64_t ld, int32_t g, int32_t n, double* __restrict__ H) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g) return;
  const double* xr = X + i;
  double s = 0.0;
#pragma unroll 8
  for (int32_t k = 0; k < n; ++k) s = s + xr[(int64_t)k * ld];
  const double mean = s / (double)n;
  double ss = 0.0;
#pragma unroll 8
  for (int32_t k = 0; k < n; ++k) {
    const double d = xr[(int64_t)k * ld] - mean;
    const double p = d * d;
    ss = ss + p;
  }
  H[i] = sqrt(ss / (double)(n - 1)) / 4.0;
}

// the pinned term, operation for operation
__device__ __forceinline__ double kcdf_exact_term(double d, double h, const double* sT) {
  const double v = d / h;
  if (v < -10.0) return 0.0;
  if (v > 10.0) return 1.0;
  const double u = fabs(v) / 10.0 * 10000.0;   // at most 10,000
  const int idx = u == u ? (int)u : 0;         // v = 0 / 0 (h == 0) reads T[0]
  const double t = sT[idx];
  return v < 0.0 ? 1.0 - t : t;
}

// The same value from a reciprocal: a = |d| (1 / h) 1000 estimates u within 1e-11, so floor(a) is the pinned index unless
// a lies within kKcdfSeam of an integer or of the range's end; there `ok` comes back false and the caller runs the exact
// operations.  d < 0 decides the side as v < 0 does (h > 0; a quotient that underflows to zero reads T[0] = 0.5 = 1 - T[0]).
// No branch: four of these are in flight per thread.
__device__ __forceinline__ double kcdf_fast_term(double d, double rh, bool fast, const double* sT, bool& ok) {
  const double a = fabs(d) * rh * 1000.0;
  const double f = floor(a);
  const double r = a - f;
  const bool out = a >= 10000.5;   // |v| > 10 for certain (an infinite d included)
  const bool in = a <= 9999.5 && r < 1.0 - kKcdfSeam && (r > kKcdfSeam || f == 0.0);
  ok = fast && (out || in);
  const double t = sT[in ? (int)f : 0];
  const double tt = out ? 1.0 : t;
  return d < 0.0 ? 1.0 - tt : tt;
}

// A workgroup holds 1024 / W sub-groups of W threads (W a power of two >= 64); a sub-group takes one item = (gene, tile of
// W test columns) and each of its threads one test sample j, with x_ij and the running sum in registers.  The gene's
// samples pass through LDS in chunks of W, double-buffered: one barrier per chunk, and every thread of the workgroup
// runs the same number of chunks.  Items are numbered gene-major, so neighbouring workgroups read the same rows of X.
template <int kMode>
__global__ void __launch_bounds__(kKcdfThreads)
kcdf_sum_kernel(const double* __restrict__ X, int64_t ldx, int32_t g, int32_t n, int32_t j0, int32_t nj,
                const double* __restrict__ H, const double* __restrict__ Tg, int32_t wshift, int32_t ntiles,
                double* __restrict__ V, int64_t ldv, unsigned long long* __restrict__ slow_out) {
  extern __shared__ double kcdf_lds[];
  double* sT = kcdf_lds;
  double* sx = kcdf_lds + kKcdfTable;
  const int tid = threadIdx.x;
  for (int i = tid; i < kKcdfTable; i += kKcdfThreads) sT[i] = Tg[i];
  const int32_t W = 1 << wshift;
  const int32_t gb = kKcdfThreads >> wshift;
  const int32_t sub = tid >> wshift, lj = tid & (W - 1);
  const int64_t items = (int64_t)g * ntiles;
  const int32_t nchunks = (n + W - 1) >> wshift;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  uint32_t slow = 0;
  for (int64_t base = (int64_t)blockIdx.x * gb; base < items; base += (int64_t)gridDim.x * gb) {
    const int64_t item = base + sub;
    const bool active = item < items;
    const int32_t gene = active ? (int32_t)(item / ntiles) : 0;
    const int32_t j = (int32_t)(active ? item - (int64_t)gene * ntiles : 0) * W + lj;
    const bool have = active && j < nj;
    const double* xr = X + gene;
    const double xj = have ? xr[(int64_t)(j0 + j) * ldx] : 0.0;
    const double h = H[gene];
    const double rh = 1.0 / h;
    // normal h and 1 / h: the error bound of the estimate holds
    const bool fast = h >= 2.2250738585072014e-308 && h <= 1.7976931348623157e308 && rh >= 2.2250738585072014e-308;
    double acc = 0.0;
    sx[tid] = lj < n ? xr[(int64_t)lj * ldx] : 0.0;
    __syncthreads();
    for (int32_t c = 0; c < nchunks; ++c) {
      const int32_t kn = ((c + 1) << wshift) + lj;
      const double nx = (c + 1 < nchunks && kn < n) ? xr[(int64_t)kn * ldx] : 0.0;
      const int32_t cnt = min(W, n - (c << wshift));
      const double* s = sx + (c & 1) * kKcdfThreads + (sub << wshift);
      int32_t kk = 0;
      for (; kk + 4 <= cnt; kk += 4) {
        double d[4], t[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          d[u] = xj - s[kk + u];
          t[u] = kcdf_fast_term(d[u], rh, kMode != 1 && fast, sT, ok[u]);
        }
        if (!(ok[0] && ok[1] && ok[2] && ok[3])) {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (!ok[u]) {
              t[u] = kcdf_exact_term(d[u], h, sT);
              if (kMode == 2) ++slow;
            }
        }
        acc = acc + t[0];
        acc = acc + t[1];
        acc = acc + t[2];
        acc = acc + t[3];
      }
      for (; kk < cnt; ++kk) {
        const double d = xj - s[kk];
        bool ok;
        double t = kcdf_fast_term(d, rh, kMode != 1 && fast, sT, ok);
        if (!ok) {
          t = kcdf_exact_term(d, h, sT);
          if (kMode == 2) ++slow;
        }
        acc = acc + t;
      }
      sx[((c + 1) & 1) * kKcdfThreads + tid] = nx;
      __syncthreads();
    }
    if (have) V[gene + (int64_t)j * ldv] = h != h ? nan : acc;   // a NaN or an infinity in the row
  }
  if (kMode == 2 && slow != 0) atomicAdd(slow_out, (unsigned long long)slow);
}

// width of a sub-group: the largest power of two in [64, 1024] that pads the nj test columns by at most 4 % more than
// the best of them
int kcdf_width_shift(int32_t nj) {
  int64_t best = INT64_MAX;
  for (int s = 6; s <= 10; ++s) best = std::min<int64_t>(best, (((int64_t)nj + (1 << s) - 1) >> s) << s);
  int pick = 6;
  for (int s = 6; s <= 10; ++s)
    if (((((int64_t)nj + (1 << s) - 1) >> s) << s) * 100 <= best * 104) pick = s;
  return pick;
}

}  // namespace

void gsva_kcdf_table(double* out) { std::copy(kcdf_host_table(), kcdf_host_table() + kKcdfTable, out); }

void debug_gsva_kcdf_set_mode(int mode) { g_kcdf_mode.store(mode); }
int debug_gsva_kcdf_width(int32_t nj) { return 1 << kcdf_width_shift(nj); }

int launch_gsva_kcdf_bandwidths(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t n, double* H) {
  PH_REQUIRE(g >= 0 && n >= 2 && ldx >= g, "gsva_kcdf: bad dims g=%d n=%d ldx=%lld", g, n, (long long)ldx);
  if (g == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(kcdf_row_moments_kernel, dim3((unsigned)((g + 255) / 256)), dim3(256), 0, ctx->stream, X, ldx, g, n, H);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}
unsigned long long debug_gsva_kcdf_slow_terms() { return g_kcdf_slow_terms.load(); }

int launch_gsva_kcdf(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t n, int32_t j0, int32_t j1, double* H,
                     double* V, int64_t ldv) {
  PH_REQUIRE(g >= 0 && n >= 2 && j0 >= 0 && j0 <= j1 && j1 <= n && ldx >= g && ldv >= g,
             "gsva_kcdf: bad dims g=%d n=%d columns [%d, %d) ldx=%lld ldv=%lld", g, n, j0, j1, (long long)ldx, (long long)ldv);
  const int32_t nj = j1 - j0;
  if (g == 0 || nj == 0) return PLAIDHIP_OK;
  if (ctx->kcdf_table == nullptr) {   // once per context
    PH_HIP(hipMalloc(&ctx->kcdf_table, (size_t)kKcdfTable * 8 + 8));
    PH_HIP(hipMemcpyAsync(ctx->kcdf_table, kcdf_host_table(), (size_t)kKcdfTable * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  const double* T = static_cast<const double*>(ctx->kcdf_table);
  unsigned long long* d_slow = reinterpret_cast<unsigned long long*>(static_cast<double*>(ctx->kcdf_table) + kKcdfTable);
  const int rc_h = launch_gsva_kcdf_bandwidths(ctx, X, ldx, g, n, H);
  if (rc_h != PLAIDHIP_OK) return rc_h;
  const int wshift = kcdf_width_shift(nj);
  const int32_t ntiles = (int32_t)(((int64_t)nj + (1 << wshift) - 1) >> wshift);
  const int64_t groups = ((int64_t)g * ntiles + (kKcdfThreads >> wshift) - 1) / (kKcdfThreads >> wshift);
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(groups, ctx->num_cu)));
  const int mode = g_kcdf_mode.load();
  if (mode == 1) {
    PH_FULL_LDS(ctx, kcdf_sum_kernel<1>);
    hipLaunchKernelGGL(kcdf_sum_kernel<1>, grid, dim3(kKcdfThreads), kKcdfLds, ctx->stream, X, ldx, g, n, j0, nj, H, T, wshift,
                       ntiles, V, ldv, d_slow);
  } else if (mode == 2) {
    PH_FULL_LDS(ctx, kcdf_sum_kernel<2>);
    PH_HIP(hipMemsetAsync(d_slow, 0, 8, ctx->stream));
    hipLaunchKernelGGL(kcdf_sum_kernel<2>, grid, dim3(kKcdfThreads), kKcdfLds, ctx->stream, X, ldx, g, n, j0, nj, H, T, wshift,
                       ntiles, V, ldv, d_slow);
    unsigned long long cnt = 0;
    PH_HIP(hipMemcpyAsync(&cnt, d_slow, 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    g_kcdf_slow_terms.store(cnt);
  } else {
    PH_FULL_LDS(ctx, kcdf_sum_kernel<0>);
    hipLaunchKernelGGL(kcdf_sum_kernel<0>, grid, dim3(kKcdfThreads), kKcdfLds, ctx->stream, X, ldx, g, n, j0, nj, H, T, wshift,
                       ntiles, V, ldv, d_slow);
  }
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
