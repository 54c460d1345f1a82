// The whole-matrix passes of normalize_medians() (R/plaid.R:554-575) around its medians, and the small reductions and
// element-wise passes a sample-sharded host and the rank-transform callers need.  gfx950 / wave64 only.
//
//   minflags : min(x, na.rm=TRUE) == 0  <=>  HAS_ZERO && !HAS_NEG            (R/plaid.R:556-557)
//   (the per-sample medians between the two: kernels_medians.hip)
//   sum      : {sum, count} of the medians, mean(medx, na.rm=TRUE)
//   shift    : (x - med[col]) + add, add = mean(medx)                         (R/plaid.R:572)
//   max, minmax, nonneg_range, colsum, map, affine, col_abs_sums: what replaid.ucell / aucell / scse and the sharded
//   callers reduce or rewrite between their phases
#include <cmath>
#include <cstdlib>

#include "common.h"

// A/B knob for `make variant DEFS=...` (tools/ab_norm.sh); the product carries no run-time switch.
//   PLAIDHIP_SHIFT_CACHED_BYTES: shift_columns_kernel stores plainly and walks from the last column down while S is no
//     larger than this many bytes (0: never, the behaviour before); see launch_shift_columns.
#ifndef PLAIDHIP_SHIFT_CACHED_BYTES
#define PLAIDHIP_SHIFT_CACHED_BYTES (4ll * 256 * 1024 * 1024)
#endif

namespace plaidhip {

__global__ void __launch_bounds__(256)
minflags_kernel(const double* __restrict__ S, int64_t count, uint32_t* flags) {
  uint32_t f = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const double v = S[i];
    f |= (v < 0.0) ? PLAIDHIP_FLAG_HAS_NEG : 0u;
    f |= (v == 0.0) ? PLAIDHIP_FLAG_HAS_ZERO : 0u;
    f |= (v != v) ? PLAIDHIP_FLAG_HAS_NAN : 0u;
  }
  for (int off = 32; off >= 1; off >>= 1) f |= __shfl_xor(f, off, 64);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
      if ((f >> b) & 1u) {
        if (__hip_atomic_load(&flags[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
          __hip_atomic_store(&flags[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
  }
}

// deterministic single-workgroup reductions (n samples: tiny)
__global__ void __launch_bounds__(1024)
sum_kernel(const double* __restrict__ v, int64_t count, double* out) {
  __shared__ double s_sum[1024];
  __shared__ double s_cnt[1024];
  const int tid = threadIdx.x;
  double s = 0.0, c = 0.0;
  for (int64_t i = tid; i < count; i += 1024) {
    const double x = v[i];
    if (x == x) { s += x; c += 1.0; }
  }
  s_sum[tid] = s;
  s_cnt[tid] = c;
  __syncthreads();
  for (int h = 512; h >= 1; h >>= 1) {
    if (tid < h) { s_sum[tid] += s_sum[tid + h]; s_cnt[tid] += s_cnt[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) { out[0] = s_sum[0]; out[1] = s_cnt[0]; }
}

__global__ void __launch_bounds__(1024)
max_kernel(const double* __restrict__ v, int64_t count, double* out) {
  __shared__ double s_max[1024];
  const int tid = threadIdx.x;
  double s = -INFINITY;
  for (int64_t i = tid; i < count; i += 1024) {
    const double x = v[i];
    s = (x > s) ? x : s;
  }
  s_max[tid] = s;
  __syncthreads();
  for (int h = 512; h >= 1; h >>= 1) {
    if (tid < h) s_max[tid] = (s_max[tid + h] > s_max[tid]) ? s_max[tid + h] : s_max[tid];
    __syncthreads();
  }
  if (tid == 0) out[0] = s_max[0];
}

// (x - med[col]) + mean(med): one streaming read + write of S.  16-byte accesses, four of them in flight per thread
// before the first is used, loads non-temporal.  CACHED = false: non-temporal stores, columns in ascending order (S fits
// no cache).  CACHED = true, for an S of the order of the Infinity Cache: plain stores, which find the line where the load
// left it, and columns from the last to the first, so that the pass ends on the columns the next crossprod writes first
// (DESIGN.md 4.3 has the measurements and where the size bound comes from).
template <bool CACHED>
__global__ void __launch_bounds__(256)
shift_columns_kernel(double* __restrict__ S, int64_t lds, int32_t m, int32_t n,
                     const double* __restrict__ med, double add, const double* __restrict__ red) {
  typedef double f64x2_s __attribute__((ext_vector_type(2)));
  constexpr int UN = 4;   // (measured with 2 / 4 / 8: 4 is the best or within 3 % of it at m = 5,000 and 50,000, aligned or not)
  if (red != nullptr) add = red[0] / red[1];   // mean(medx, na.rm=TRUE) from {sum, count}
  // grid.y walks columns (CACHED: from the last one down), grid.x * block walks the rows of a column
  for (int cy = blockIdx.y; cy < n; cy += gridDim.y) {
    const int c = CACHED ? n - 1 - cy : cy;
    double* sc = S + (int64_t)c * lds;
    const double md = med[c];
    const int head = (int)((reinterpret_cast<uintptr_t>(sc) >> 3) & 1u);   // first element not 16-byte aligned
    const int npairs = (m - head) >> 1;
    if (blockIdx.x == 0) {
      if (threadIdx.x == 0 && head) sc[0] = (sc[0] - md) + add;
      if (threadIdx.x == 1 && ((m - head) & 1)) sc[m - 1] = (sc[m - 1] - md) + add;
    }
    f64x2_s* p = reinterpret_cast<f64x2_s*>(sc + head);
    for (int base = blockIdx.x * 256 * UN; base < npairs; base += gridDim.x * 256 * UN) {
      f64x2_s v[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int i = base + u * 256 + (int)threadIdx.x;
        v[u] = __builtin_nontemporal_load(p + (i < npairs ? i : npairs - 1));
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int i = base + u * 256 + (int)threadIdx.x;
        if (i < npairs) {
          f64x2_s r;
          r.x = (v[u].x - md) + add;
          r.y = (v[u].y - md) + add;
          if constexpr (CACHED) p[i] = r;
          else __builtin_nontemporal_store(r, p + i);
        }
      }
    }
  }
}

// (x - med[col]) + mean(med) written as FLOAT into another matrix: the last step of normalize_medians (R/plaid.R:572) fused
// with the cast a sample-sharded job makes anyway before its scores travel to the root -- config 5's 1e6 x 50,000 result is
// 400 GB in fp64, more than one GPU holds, so the gather carries fp32 (sharded.gather_scores(dtype = float32)).  S itself
// stays as the crossprod wrote it: one read of S and a half-size write replace the read + write of the shift and the read +
// half-size write of the cast.  16-byte loads (two scores), 8-byte stores, four loads in flight per thread; the rounding
// is that of a plain fp64 -> fp32 conversion of the shifted value -- bit-identical to shift_columns followed by a cast.
__global__ void __launch_bounds__(256)
shift_columns_cast_f32_kernel(const double* __restrict__ S, int64_t lds, int32_t m, int32_t n, const double* __restrict__ med,
                              double add, const double* __restrict__ red, float* __restrict__ out, int64_t ldo) {
  typedef double f64x2_s __attribute__((ext_vector_type(2)));
  typedef float f32x2_s __attribute__((ext_vector_type(2)));
  constexpr int UN = 4;
  if (red != nullptr) add = red[0] / red[1];
  for (int c = blockIdx.y; c < n; c += gridDim.y) {
    const double* sc = S + (int64_t)c * lds;
    float* oc = out + (int64_t)c * ldo;
    const double md = med[c];
    // pairs are taken where BOTH the fp64 source (16 bytes) and the fp32 destination (8 bytes) are aligned; else by element
    const bool pairs_ok = ((reinterpret_cast<uintptr_t>(sc) & 15u) == 0u) && ((reinterpret_cast<uintptr_t>(oc) & 7u) == 0u);
    if (!pairs_ok) {
      for (int i = blockIdx.x * 256 + (int)threadIdx.x; i < m; i += gridDim.x * 256)
        oc[i] = (float)((sc[i] - md) + add);
      continue;
    }
    const int npairs = m >> 1;
    if (blockIdx.x == 0 && threadIdx.x == 0 && (m & 1)) oc[m - 1] = (float)((sc[m - 1] - md) + add);
    const f64x2_s* p = reinterpret_cast<const f64x2_s*>(sc);
    f32x2_s* q = reinterpret_cast<f32x2_s*>(oc);
    for (int base = blockIdx.x * 256 * UN; base < npairs; base += gridDim.x * 256 * UN) {
      f64x2_s v[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int i = base + u * 256 + (int)threadIdx.x;
        v[u] = __builtin_nontemporal_load(p + (i < npairs ? i : npairs - 1));
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int i = base + u * 256 + (int)threadIdx.x;
        if (i < npairs) {
          f32x2_s r;
          r.x = (float)((v[u].x - md) + add);
          r.y = (float)((v[u].y - md) + add);
          __builtin_nontemporal_store(r, q + i);
        }
      }
    }
  }
}

// ---- element-wise / column helpers for the rank-transform callers -------------------------
// (replaid.ucell R/plaid.R:276-282, replaid.aucell :304-309, replaid.scse :155-190)
__global__ void __launch_bounds__(256)
map_kernel(double* __restrict__ v, int64_t count, int op, double p0, const double* __restrict__ scalar) {
  if (op >= 4) {
    // replaid.scse's automatic removeLog2 (R/plaid.R:160-161), decided on the device from {min, max} at `scalar`
    // (p0 != 0: a sparse X whose implicit zeros take part): the transform runs iff min == 0 and max < 20
    double mn = scalar[0], mx = scalar[1];
    if (p0 != 0.0) { mn = mn < 0.0 ? mn : 0.0; mx = mx > 0.0 ? mx : 0.0; }
    if (!(mn == 0.0 && mx < 20.0)) return;
    op -= 2;
    scalar = nullptr;
  }
  const double sc = scalar != nullptr ? *scalar : 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    double x = v[i];
    if (op == 0) x = fmin(sc - x, p0);                                 // pmin(max(rX) - rX, rmax + 1)
    else if (op == 1) x = 1.08 * fmax((x - (sc - p0)) / p0, 0.0);      // 1.08 * pmax((rX - (max - K)) / K, 0)
    else if (op == 2) x = (x > 0.0) ? exp2(x) : x;                     // X[X > 0] <- 2 ** X[X > 0]
    else x = exp2(x);                                                  // X@x <- 2 ** X@x
    v[i] = x;
  }
}

// out[c] = sum |X[, c]| over a dense column (len rows) or the stored values of a CSC column
__global__ void __launch_bounds__(256)
col_abs_sums_kernel(const double* __restrict__ X, int64_t ldx, int32_t len, const int32_t* __restrict__ Xp,
                    int32_t n, double* __restrict__ out) {
  __shared__ double s_part[4];
  for (int c = blockIdx.x; c < n; c += gridDim.x) {
    const double* xc = Xp ? X + Xp[c] : X + (int64_t)c * ldx;
    const int cnt = Xp ? Xp[c + 1] - Xp[c] : len;
    double s = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 256) s += fabs(xc[i]);
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[c] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    __syncthreads();
  }
}

// S[j, c] = S[j, c] * mul / (col_div ? col_div[c] * div_scale + 1e-8 : 1) + (row_add ? row_add[j] : 0) + add
__global__ void __launch_bounds__(256)
affine_kernel(double* __restrict__ S, int64_t lds, int32_t m, int32_t n, double mul,
              const double* __restrict__ col_div, double div_scale, const double* __restrict__ row_add, double add) {
  for (int c = blockIdx.y; c < n; c += gridDim.y) {
    double* sc = S + (int64_t)c * lds;
    const double f = col_div ? mul / (col_div[c] * div_scale + 1e-8) : mul;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x)
      sc[i] = sc[i] * f + (row_add ? row_add[i] : 0.0) + add;
  }
}

// min / max over non-NaN values, two stages (deterministic): every workgroup of stage one reduces a slice of v to
// {min, max} (part[b], part[nb + b]); one workgroup folds the partials into out[0] = min, out[1] = max
__device__ __forceinline__ void block_minmax_1024(double mn, double mx, double* s_mn, double* s_mx, double& omn, double& omx) {
  const int tid = threadIdx.x;
  s_mn[tid] = mn; s_mx[tid] = mx;
  __syncthreads();
  for (int h = 512; h >= 1; h >>= 1) {
    if (tid < h) {
      s_mn[tid] = s_mn[tid + h] < s_mn[tid] ? s_mn[tid + h] : s_mn[tid];
      s_mx[tid] = s_mx[tid + h] > s_mx[tid] ? s_mx[tid + h] : s_mx[tid];
    }
    __syncthreads();
  }
  omn = s_mn[0]; omx = s_mx[0];
}

__global__ void __launch_bounds__(1024)
minmax_partial_kernel(const double* __restrict__ v, int64_t count, double* __restrict__ part) {
  __shared__ double s_mn[1024], s_mx[1024];
  double mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 1024) {
    const double x = v[i];
    if (x == x) { mn = x < mn ? x : mn; mx = x > mx ? x : mx; }
  }
  double omn, omx;
  block_minmax_1024(mn, mx, s_mn, s_mx, omn, omx);
  if (threadIdx.x == 0) { part[blockIdx.x] = omn; part[gridDim.x + blockIdx.x] = omx; }
}

__global__ void __launch_bounds__(1024)
minmax_final_kernel(const double* __restrict__ part, int nb, double* out) {
  __shared__ double s_mn[1024], s_mx[1024];
  double mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < nb; i += 1024) {
    const double a = part[i], b = part[nb + i];
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  double omn, omx;
  block_minmax_1024(mn, mx, s_mn, s_mx, omn, omx);
  if (threadIdx.x == 0) { out[0] = omn; out[1] = omx; }
}

// {0 if every stored value is finite and >= 0, else -1; max; smallest value > 0 (+inf if there is none)} over the stored
// values Xx[Xp[0] .. Xp[n]) of a dgCMatrix -- the range is read from Xp ON THE DEVICE, so a caller that does not know
// nnz(X) (or knows it only approximately: a shard of a larger matrix) cannot make the sweep read too much or too little.
// It decides whether the scatter crossprod may sum in fixed point (kernels_spmm.hip: scatter_fixed_ok).
__global__ void __launch_bounds__(1024)
nonneg_range_partial_kernel(const double* __restrict__ v, const int32_t* __restrict__ Xp, int32_t n,
                            double* __restrict__ part) {
  __shared__ double s_mn[1024], s_mx[1024];
  const int64_t begin = Xp[0], end = Xp[n];
  double ok = 0.0, mx = 0.0, mnz = INFINITY;
  for (int64_t i = begin + (int64_t)blockIdx.x * 1024 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 1024) {
    const double x = v[i];
    ok = ((x >= 0.0) && (x < INFINITY)) ? ok : -1.0;      // false for NaN, negatives and +inf
    mx = x > mx ? x : mx;
    mnz = (x > 0.0 && x < mnz) ? x : mnz;
  }
  double omn, omx;
  block_minmax_1024(ok, mx, s_mn, s_mx, omn, omx);
  if (threadIdx.x == 0) { part[blockIdx.x] = omn; part[gridDim.x + blockIdx.x] = omx; }
  __syncthreads();
  block_minmax_1024(mnz, 0.0, s_mn, s_mx, omn, omx);
  if (threadIdx.x == 0) part[2 * gridDim.x + blockIdx.x] = omn;
}

__global__ void __launch_bounds__(1024)
nonneg_range_final_kernel(const double* __restrict__ part, int nb, double* out) {
  __shared__ double s_mn[1024], s_mx[1024];
  double ok = 0.0, mx = 0.0, mnz = INFINITY;
  for (int i = threadIdx.x; i < nb; i += 1024) {
    const double a = part[i], b = part[nb + i], c = part[2 * nb + i];
    ok = a < ok ? a : ok;
    mx = b > mx ? b : mx;
    mnz = c < mnz ? c : mnz;
  }
  double omn, omx;
  block_minmax_1024(ok, mx, s_mn, s_mx, omn, omx);
  if (threadIdx.x == 0) { out[0] = omn; out[1] = omx; }
  __syncthreads();
  block_minmax_1024(mnz, 0.0, s_mn, s_mx, omn, omx);
  if (threadIdx.x == 0) { out[2] = omn; out[3] = INFINITY; }   // out[3]: the largest column sum, when launch_colsum_max follows
}

// the largest sum of a column's stored values (all >= 0 where it matters): no score can exceed it, whatever the size of its set
__global__ void __launch_bounds__(256)
colsum_kernel(const double* __restrict__ v, const int32_t* __restrict__ Xp, int32_t n, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * 4;
  for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += nw) {
    const int64_t q0 = Xp[c], q1 = Xp[c + 1];
    double s = 0.0;
    for (int64_t i = q0 + lane; i < q1; i += 64) s += v[i];
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) out[c] = s;
  }
}

// nnz_hint only sizes the grid (< 0: unknown); the swept range is Xx[Xp[0] .. Xp[n]) whatever it says
int launch_nonneg_range(plaidhip_ctx* ctx, const double* Xx, const int32_t* Xp, int32_t n, int64_t nnz_hint, double* out) {
  const int cap = ctx->num_cu * 2;
  int64_t nb64 = nnz_hint < 0 ? cap : (nnz_hint + 8 * 1024 - 1) / (8 * 1024);
  const int nb = nb64 < 1 ? 1 : (nb64 > cap ? cap : (int)nb64);
  int rc = ensure_workspace(ctx, (size_t)nb * 3 * sizeof(double));
  if (rc != PLAIDHIP_OK) return rc;
  double* part = reinterpret_cast<double*>(ctx->ws);
  hipLaunchKernelGGL(nonneg_range_partial_kernel, dim3(nb), dim3(1024), 0, ctx->stream, Xx, Xp, n, part);
  hipLaunchKernelGGL(nonneg_range_final_kernel, dim3(1), dim3(1024), 0, ctx->stream, part, nb, out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// out[0] = max over the columns of the sum of their stored values (per-column sums in the workspace, then one reduction)
int launch_colsum_max(plaidhip_ctx* ctx, const double* Xx, const int32_t* Xp, int32_t n, double* out) {
  if (n <= 0) return PLAIDHIP_OK;
  int rc = ensure_workspace(ctx, (size_t)n * sizeof(double));
  if (rc != PLAIDHIP_OK) return rc;
  double* sums = reinterpret_cast<double*>(ctx->ws);
  const int need = (n + 3) / 4, cap = ctx->num_cu * 16;
  hipLaunchKernelGGL(colsum_kernel, dim3(need < cap ? need : cap), dim3(256), 0, ctx->stream, Xx, Xp, n, sums);
  return launch_max(ctx, sums, n, out);
}

int launch_map(plaidhip_ctx* ctx, double* v, int64_t count, int op, double p0, const double* scalar) {
  if (count == 0) return PLAIDHIP_OK;
  int64_t blocks = (count + 256 * 8 - 1) / (256 * 8);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(map_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, v, count, op, p0, scalar);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_col_abs_sums(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t len, const int32_t* Xp,
                        int32_t n, double* out) {
  if (n == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(col_abs_sums_kernel, dim3(n < 8192 ? n : 8192), dim3(256), 0, ctx->stream, X, ldx, len, Xp, n, out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_affine(plaidhip_ctx* ctx, double* S, int64_t lds, int32_t m, int32_t n, double mul,
                  const double* col_div, double div_scale, const double* row_add, double add) {
  ctx->fmed.valid = false;
  if (n == 0 || m == 0) return PLAIDHIP_OK;
  int bx = (m + 255) / 256;
  if (bx > 64) bx = 64;
  hipLaunchKernelGGL(affine_kernel, dim3(bx, n < 32768 ? n : 32768), dim3(256), 0, ctx->stream, S, lds, m, n, mul,
                     col_div, div_scale, row_add, add);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_minmax(plaidhip_ctx* ctx, const double* v, int64_t count, double* out) {
  int64_t nb64 = (count + 8 * 1024 - 1) / (8 * 1024);
  const int cap = ctx->num_cu * 2;
  const int nb = nb64 < 1 ? 1 : (nb64 > cap ? cap : (int)nb64);
  int rc = ensure_workspace(ctx, (size_t)nb * 2 * sizeof(double));
  if (rc != PLAIDHIP_OK) return rc;
  double* part = reinterpret_cast<double*>(ctx->ws);
  hipLaunchKernelGGL(minmax_partial_kernel, dim3(nb), dim3(1024), 0, ctx->stream, v, count, part);
  hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(1024), 0, ctx->stream, part, nb, out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_minflags(plaidhip_ctx* ctx, const double* S, int64_t count, uint32_t* flags) {
  if (count == 0) return PLAIDHIP_OK;
  int64_t blocks = (count + 256 * 8 - 1) / (256 * 8);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(minflags_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, S, count, flags);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_sum(plaidhip_ctx* ctx, const double* v, int64_t count, double* out) {
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, v, count, out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_max(plaidhip_ctx* ctx, const double* v, int64_t count, double* out) {
  hipLaunchKernelGGL(max_kernel, dim3(1), dim3(1024), 0, ctx->stream, v, count, out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_shift_columns(plaidhip_ctx* ctx, double* S, int64_t lds, int32_t m, int32_t n,
                         const double* med, double add, const double* red) {
  ctx->fmed.valid = false;   // (S changes: the candidates of a fused crossprod are history)
  if (n == 0 || m == 0) return PLAIDHIP_OK;
  // workgroups per column: one trip of 2,048 values each, up to 32 -- a 50,000-set column is one trip for every workgroup.
  // One grid row per column while the grid allows it (65,535 rows); beyond that 2,048 rows that each walk ~n / 2,048
  // columns (with 65,535 rows a third of them would walk two columns and the rest one).  Measured, late round 4
  // (tools/bench_shift.py big, PLAIDHIP_SHIFT_BX / _BY in the tools build; it was 16 workgroups and 32,768 rows):
  // same box, old -> new: 100,000 x 50,000: 14.44 -> 14.23 ms (13.1 on another box); 8,192 x 50,000: 1.183 -> 1.14 ms;
  // 8,192 x 49,999 (every other column misaligned): 1.325 -> 1.16 ms; 10,000 x 61,459: 1.94 -> 1.82 ms; 10,000 x 5,000:
  // unchanged (three workgroups per column either way).
  int bx = (m / 2 + 256 * 4 - 1) / (256 * 4);
  if (bx < 1) bx = 1;
  int bx_cap = 32;
  int by = n <= 65535 ? n : 2048;
#ifdef PLAIDHIP_DIAG
  if (const char* e = getenv("PLAIDHIP_SHIFT_BX")) bx_cap = atoi(e);
  if (const char* e = getenv("PLAIDHIP_SHIFT_BY")) by = n < atoi(e) ? n : atoi(e);   // (rows = min(n, value))
#endif
  if (bx > bx_cap) bx = bx_cap;
  // plain stores and the descending walk while S is at most four times the 256 MiB Infinity Cache: what they gain is a
  // cache effect (measured at 400 MB); beyond, at most a quarter of S can be on the die when the pass or its successor
  // comes by, and the non-temporal ascending form measured at 3-40 GB stays as it was
  const bool cached = (int64_t)n * lds * 8 <= (int64_t)(PLAIDHIP_SHIFT_CACHED_BYTES);
  if (cached)
    hipLaunchKernelGGL(shift_columns_kernel<true>, dim3(bx, by), dim3(256), 0, ctx->stream, S, lds, m, n, med, add, red);
  else
    hipLaunchKernelGGL(shift_columns_kernel<false>, dim3(bx, by), dim3(256), 0, ctx->stream, S, lds, m, n, med, add, red);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_shift_columns_cast_f32(plaidhip_ctx* ctx, const double* S, int64_t lds, int32_t m, int32_t n, const double* med,
                                  double add, const double* red, float* out, int64_t ldo) {
  if (n == 0 || m == 0) return PLAIDHIP_OK;
  int bx = (m / 2 + 256 * 4 - 1) / (256 * 4);
  if (bx < 1) bx = 1;
  if (bx > 32) bx = 32;
  const int by = n <= 65535 ? n : 2048;
  hipLaunchKernelGGL(shift_columns_cast_f32_kernel, dim3(bx, by), dim3(256), 0, ctx->stream, S, lds, m, n, med, add, red, out, ldo);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
