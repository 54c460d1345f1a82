// GSVA's other two scorers, replaid.zscore and replaid.plage (include/plaidhip.h: plaidhip_zscore, plaidhip_plage pin every
// operation):
//
//   plage_row_moments_kernel     mean, sd and the flag of every gene, one thread per gene walking the samples in order
//                                (kcdf_row_moments_kernel's order)
//   plage_standardize_cm_kernel  Z of a column range, column-major, for the crossprod behind zscore
//   plage_standardize_gm_kernel  Z of all samples, gene-major (a gene's samples contiguous, rows padded with zeros to a
//                                multiple of 16 samples) through an LDS tile transpose, for plage
//   plage_compact_kernel         per set: the kept (non-constant) members in G's order, the effective size, the NaN flag
//   plage_gram_kernel            C = Z_s Z_s' in 32 x 32 tiles (the hot path): ROUNDED products added in sample order
//   plage_gram_mfma_kernel       the same in 16 x 16 tiles on v_mfma_f64_16x16x4_f64, which adds unrounded products: behind
//                                the test hook only (the pinned orthogonal pair needs an exactly zero C_01; DESIGN.md section
//                                22 has both times)
//   plage_eigen_kernel           one workgroup per set: the power iteration, the orientation, the per-set statistics
//   plage_project_kernel         v_j = sum_i u_i z_ij / sqrt(lambda) for a column range
//   zscore_epilogue_kernel       S / sqrt(k), NaN for k = 0 and for a set with a flagged member
//
// Contraction: off for the whole file, so no product written here fuses with an add; the divisions and square roots
// expand to their correctly rounded sequences.  The one exception is the matrix instruction of plage_gram_mfma_kernel,
// whose four products per step are accumulated inside the instruction; the product does not launch it.  The order of every sum is fixed by the launch geometry
// alone: no atomics, no split over samples.  Vector stores only.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <numeric>
#include <vector>

#include "common.h"

#pragma clang fp contract(off)

#define PH_TRY(expr)                      \
  do {                                    \
    int rc_ = (expr);                     \
    if (rc_ != PLAIDHIP_OK) return rc_;   \
  } while (0)

namespace plaidhip {

namespace {

constexpr int kPlageThreads = 256;          // the eigen workgroup, and four Gram wavefronts
constexpr int kGramWaves = kPlageThreads / 64;   // tiles of one Gram workgroup
constexpr int kGramTile = 16;               // rows and columns of a tile of C on the matrix instruction; the padding of C's rows
constexpr int kVecTile = 32;                // rows and columns of a tile of C in the product's form
constexpr int kGramChunk = 16;              // samples per trip of the Gram K loop (four MFMA steps of four samples)
constexpr int kVecPad = kGramChunk + 1;     // doubles between the rows of a staged operand tile
constexpr int kMaxBatchSets = 65535;        // gridDim.y of the Gram launch

using d4 = __attribute__((ext_vector_type(4))) double;

std::atomic<int> g_plage_gram{0};   // test hook: 0 the product's Gram kernel (rounded products) | 1 the MFMA form

__device__ __forceinline__ double plage_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// flag: 0 kept, 1 constant (sd == 0), 2 sd not finite (a NaN or an infinity in the row, or an overflow)
__global__ void __launch_bounds__(256)
plage_row_moments_kernel(const double* __restrict__ X, int64_t ld, int32_t g, int32_t n, double* __restrict__ mean_out,
                         double* __restrict__ sd_out, int32_t* __restrict__ flag_out) {
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
  const double sd = sqrt(ss / (double)(n - 1));
  mean_out[i] = mean;
  sd_out[i] = sd;
  flag_out[i] = sd == 0.0 ? 1 : (sd > 0.0 && sd < INFINITY ? 0 : 2);
}

__device__ __forceinline__ double plage_z(double x, double mean, double sd, int32_t flag) {
  if (flag == 0) return (x - mean) / sd;
  return flag == 1 ? 0.0 : plage_nan();
}

// Z[i + j ldz] of the columns j0 .. j0 + nj - 1 of X
__global__ void __launch_bounds__(256)
plage_standardize_cm_kernel(const double* __restrict__ X, int64_t ldx, int32_t g, int32_t j0, int32_t nj,
                            const double* __restrict__ mean, const double* __restrict__ sd, const int32_t* __restrict__ flag,
                            double* __restrict__ Z, int64_t ldz) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  const int32_t j = blockIdx.y;
  if (i >= g || j >= nj) return;
  Z[i + (int64_t)j * ldz] = plage_z(X[i + (int64_t)(j0 + j) * ldx], mean[i], sd[i], flag[i]);
}

// Zg[i ldz + j], j < ldz (a multiple of 16): z for j < n, 0.0 behind it.  32 x 32 tiles through LDS: the reads run along
// the genes, the writes along the samples
__global__ void __launch_bounds__(256)
plage_standardize_gm_kernel(const double* __restrict__ X, int64_t ldx, int32_t g, int32_t n, const double* __restrict__ mean,
                            const double* __restrict__ sd, const int32_t* __restrict__ flag, double* __restrict__ Zg,
                            int64_t ldz) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int32_t i0 = blockIdx.x * 32, jt = blockIdx.y * 32;
  const int32_t i = i0 + tx;
  double mu = 0.0, s = 1.0;
  int32_t f = 1;
  if (i < g) { mu = mean[i]; s = sd[i]; f = flag[i]; }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int32_t j = jt + ty + 8 * r;
    tile[ty + 8 * r][tx] = (i < g && j < n) ? plage_z(X[i + (int64_t)j * ldx], mu, s, f) : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int32_t ii = i0 + ty + 8 * r, j = jt + tx;
    if (ii < g && j < ldz) Zg[(int64_t)ii * ldz + j] = tile[tx][ty + 8 * r];
  }
}

// one wavefront per set: Ci (the kept members' rows, in the set's own segment, G's order), Cpos (their positions in the
// segment), keff, nanflag
__global__ void __launch_bounds__(64)
plage_compact_kernel(const int32_t* __restrict__ Gp, const int32_t* __restrict__ Gi, int32_t m, const int32_t* __restrict__ flag,
                     int32_t* __restrict__ Ci, int32_t* __restrict__ Cpos, int32_t* __restrict__ keff,
                     int32_t* __restrict__ nanflag) {
  const int32_t s = blockIdx.x;
  if (s >= m) return;
  const int lane = threadIdx.x;
  const int32_t p0 = Gp[s], k = Gp[s + 1] - p0;
  int32_t cnt = 0;
  bool anynan = false;
  for (int32_t base = 0; base < k; base += 64) {
    const int32_t e = base + lane;
    const bool valid = e < k;
    const int32_t gene = valid ? Gi[p0 + e] : 0;
    const int32_t f = valid ? flag[gene] : 1;
    const bool keep = valid && f != 1;
    const unsigned long long mask = __ballot(keep);
    anynan = anynan || __ballot(valid && f == 2) != 0ull;
    if (keep) {
      const int32_t pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
      Ci[p0 + pos] = gene;
      Cpos[p0 + pos] = e;
    }
    cnt += __popcll(mask);
  }
  if (lane == 0) {
    keff[s] = cnt;
    nanflag[s] = anynan ? 1 : 0;
  }
}

// The tiles of the upper triangle of a set's C are numbered column by column: t = tj (tj + 1) / 2 + ti, ti <= tj
__device__ __forceinline__ void plage_tile(int32_t t, int32_t* ti, int32_t* tj) {
  int32_t c = (int32_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (c * (c + 1) / 2 > t) --c;
  while ((c + 1) * (c + 2) / 2 <= t) ++c;
  *tj = c;
  *ti = t - c * (c + 1) / 2;
}

// C_s = Z_s Z_s' of the sets order[0 .. nb), the product's form: every C_ab is the sum over the samples 0, 1, ..., in order
// from 0.0, of the ROUNDED products z_a z_b (no contraction).  Wavefront w of workgroup (x, y) takes the 32 x 32 tile
// t = 4 x + w of set order[y].  Per trip of 16 samples lane l reads the samples 8 (l >> 5) .. + 7 of row 32 ti + (l & 31)
// and of row 32 tj + (l & 31), 64 contiguous bytes each (the rows are padded with zeros to whole trips: no remainder), and
// the two 32 x 16 operand tiles pass through the wavefront's own LDS (rows 17 doubles apart: the eight row groups a
// wavefront reads at once fall into different banks); lane l = 8 q + r then holds the sixteen results of rows 4 q .. 4 q + 3,
// columns 4 r .. 4 r + 3: eight LDS reads per sixteen multiply-adds.  C is written at [i + j ld] and mirrored, ld = the
// set's nominal size rounded up to 16; only i <= j is taken from a diagonal tile.
__global__ void __launch_bounds__(kPlageThreads)
plage_gram_kernel(const double* __restrict__ Zg, int64_t ldz, const int32_t* __restrict__ Gp, const int32_t* __restrict__ Ci,
                  const int32_t* __restrict__ keff, const int32_t* __restrict__ nanflag, const int32_t* __restrict__ order,
                  const int64_t* __restrict__ coff, double* __restrict__ ws) {
  __shared__ double stage[kGramWaves * 2 * kVecTile * kVecPad];
  const int32_t s = order[blockIdx.y];
  const int32_t k = keff[s];
  const int32_t T = (k + kVecTile - 1) / kVecTile;
  const int32_t ntile = nanflag[s] != 0 ? 0 : T * (T + 1) / 2;
  const int wave = threadIdx.x >> 6;
  if ((int32_t)blockIdx.x * kGramWaves >= ntile) return;   // (the whole workgroup: before any barrier)
  const int32_t t = (int32_t)blockIdx.x * kGramWaves + wave;
  const bool active = t < ntile;                           // (uniform over a wavefront)
  int32_t ti, tj;
  plage_tile(t, &ti, &tj);
  const int lane = threadIdx.x & 63, lr = lane & 31, lh = lane >> 5, q = lane >> 3, r = lane & 7;
  const int32_t p0 = Gp[s];
  const int64_t ld = ((int64_t)(Gp[s + 1] - p0) + kGramTile - 1) / kGramTile * kGramTile;
  const int32_t ra = ti * kVecTile + lr, rb = tj * kVecTile + lr;
  const bool va = active && ra < k, vb = active && rb < k;
  const double* pa = Zg + (va ? (int64_t)Ci[p0 + ra] * ldz : 0) + 8 * lh;
  const double* pb = Zg + (vb ? (int64_t)Ci[p0 + rb] * ldz : 0) + 8 * lh;
  double* sa = stage + wave * 2 * kVecTile * kVecPad;
  double* sb = sa + kVecTile * kVecPad;
  double acc[4][4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[e][f] = 0.0;
  for (int64_t kk = 0; kk < ldz; kk += kGramChunk) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      double2 a = {0.0, 0.0}, b = {0.0, 0.0};
      if (va) a = *reinterpret_cast<const double2*>(pa + kk + 2 * h);
      if (vb) b = *reinterpret_cast<const double2*>(pb + kk + 2 * h);
      sa[lr * kVecPad + 8 * lh + 2 * h] = a.x;
      sa[lr * kVecPad + 8 * lh + 2 * h + 1] = a.y;
      sb[lr * kVecPad + 8 * lh + 2 * h] = b.x;
      sb[lr * kVecPad + 8 * lh + 2 * h + 1] = b.y;
    }
    __syncthreads();
#pragma unroll 4
    for (int sm = 0; sm < kGramChunk; ++sm) {
      double av[4], bv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        av[e] = sa[(4 * q + e) * kVecPad + sm];
        bv[e] = sb[(4 * r + e) * kVecPad + sm];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const double p = av[e] * bv[f];
          acc[e][f] = acc[e][f] + p;
        }
    }
    __syncthreads();
  }
  if (!active) return;
  double* C = ws + coff[blockIdx.y];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int32_t i = ti * kVecTile + 4 * q + e, j = tj * kVecTile + 4 * r + f;
      if (i < k && j < k && i <= j) {
        C[i + j * ld] = acc[e][f];
        C[j + i * ld] = acc[e][f];
      }
    }
}

// The same matrices on v_mfma_f64_16x16x4_f64, behind the test hook only: one wavefront per 16 x 16 tile.  Lane l = 16 q + r
// reads, per trip of 16 samples, the samples 4 q .. 4 q + 3 of row 16 ti + r (the A operand) and of row 16 tj + r (the B
// operand) and feeds sample 4 q + e to step e, so step e multiplies the samples {e, 4 + e, 8 + e, 12 + e} of the trip (the same
// assignment for both operands) and adds the four products to the running sum inside the instruction, WITHOUT rounding a
// product first: rows whose products cancel term by term leave a rounding residue, which is why the product does not launch it.
__global__ void __launch_bounds__(kPlageThreads)
plage_gram_mfma_kernel(const double* __restrict__ Zg, int64_t ldz, const int32_t* __restrict__ Gp, const int32_t* __restrict__ Ci,
                       const int32_t* __restrict__ keff, const int32_t* __restrict__ nanflag, const int32_t* __restrict__ order,
                       const int64_t* __restrict__ coff, double* __restrict__ ws) {
  const int32_t s = order[blockIdx.y];
  const int32_t k = keff[s];
  const int32_t T = (k + kGramTile - 1) / kGramTile;
  const int32_t ntile = nanflag[s] != 0 ? 0 : T * (T + 1) / 2;
  const int32_t t = (int32_t)blockIdx.x * kGramWaves + (int32_t)(threadIdx.x >> 6);
  if (t >= ntile) return;   // (uniform over the wavefront; the kernel has no barrier)
  int32_t ti, tj;
  plage_tile(t, &ti, &tj);
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int32_t p0 = Gp[s];
  const int64_t ld = ((int64_t)(Gp[s + 1] - p0) + kGramTile - 1) / kGramTile * kGramTile;
  const int32_t ra = ti * kGramTile + r, rb = tj * kGramTile + r;
  const bool va = ra < k, vb = rb < k;
  const double* pa = Zg + (va ? (int64_t)Ci[p0 + ra] * ldz : 0) + 4 * q;
  const double* pb = Zg + (vb ? (int64_t)Ci[p0 + rb] * ldz : 0) + 4 * q;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int64_t kk = 0; kk < ldz; kk += kGramChunk) {
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
    if (va) {
      const double2 a01 = *reinterpret_cast<const double2*>(pa + kk);
      const double2 a23 = *reinterpret_cast<const double2*>(pa + kk + 2);
      a[0] = a01.x; a[1] = a01.y; a[2] = a23.x; a[3] = a23.y;
    }
    if (vb) {
      const double2 b01 = *reinterpret_cast<const double2*>(pb + kk);
      const double2 b23 = *reinterpret_cast<const double2*>(pb + kk + 2);
      b[0] = b01.x; b[1] = b01.y; b[2] = b23.x; b[3] = b23.y;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], b[e], acc, 0, 0, 0);
  }
  double* C = ws + coff[blockIdx.y];
#pragma unroll
  for (int e = 0; e < 4; ++e) {   // result e of a lane: row q + 4 e of the tile, column r
    const int32_t i = ti * kGramTile + q + 4 * e, j = tj * kGramTile + r;
    if (i < k && j < k && i <= j) {
      C[i + j * ld] = acc[e];
      C[j + i * ld] = acc[e];
    }
  }
}

// the fixed tree of every reduction of plage_eigen_kernel: thread t brings the sum of its own elements t, t + 256, ... in
// ascending order from 0.0; red[t] += red[t + s] for s = 128, 64, ..., 1
__device__ __forceinline__ double plage_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = kPlageThreads / 2; s >= 1; s >>= 1) {
    if (t < s) red[t] = red[t] + red[t + s];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

// the power iteration of include/plaidhip.h on C (k x k, leading dimension ld, symmetric bit for bit), one workgroup per
// set.  LDS: u[kmax], y[kmax], red[256], redi[256].
__global__ void __launch_bounds__(kPlageThreads)
plage_eigen_kernel(const int32_t* __restrict__ Gp, const int32_t* __restrict__ Cpos, const int32_t* __restrict__ keff,
                   const int32_t* __restrict__ nanflag, const int32_t* __restrict__ order, const int64_t* __restrict__ coff,
                   const double* __restrict__ ws, int32_t kmax, int32_t m, double tol, int32_t maxit, double* __restrict__ U,
                   double* __restrict__ stats, double* __restrict__ L) {
  extern __shared__ double plage_lds[];
  double* u = plage_lds;
  double* y = u + kmax;
  double* red = y + kmax;
  int32_t* redi = reinterpret_cast<int32_t*>(red + kPlageThreads);
  const int t = threadIdx.x;
  const int32_t s = order[blockIdx.x];
  const int32_t k = keff[s], p0 = Gp[s], knom = Gp[s + 1] - p0;
  const double nan = plage_nan();
  if (L != nullptr)
    for (int32_t e = t; e < knom; e += kPlageThreads) L[p0 + e] = 0.0;   // (a dropped constant member keeps this 0)
  __syncthreads();
  if (k == 0 || nanflag[s] != 0) {
    for (int32_t i = t; i < k; i += kPlageThreads) {
      U[p0 + i] = nan;
      if (L != nullptr) L[p0 + Cpos[p0 + i]] = nan;   // (positions of kept members: none of them is written twice)
    }
    if (t == 0) {
      stats[s] = (double)k;
      stats[s + (int64_t)m] = nan;
      stats[s + 2 * (int64_t)m] = nan;
      stats[s + 3 * (int64_t)m] = 0.0;
      stats[s + 4 * (int64_t)m] = nan;
      stats[s + 5 * (int64_t)m] = 0.0;
    }
    return;
  }
  const double* C = ws + coff[blockIdx.x];
  const int64_t ld = ((int64_t)knom + kGramTile - 1) / kGramTile * kGramTile;

  // the start: the column of largest squared 2-norm, lowest index at a tie
  double best = -1.0;
  int32_t bi = 0;
  double tr = 0.0;
  for (int32_t i = t; i < k; i += kPlageThreads) {
    double nn = 0.0;
    for (int32_t j = 0; j < k; ++j) {
      const double c = C[i + j * ld];   // (= C[j + i ld]: column i, read along the threads)
      const double p = c * c;
      nn = nn + p;
    }
    if (nn > best) { best = nn; bi = i; }
    tr = tr + C[i + i * ld];
  }
  red[t] = best;
  redi[t] = bi;
  __syncthreads();
  for (int h = kPlageThreads / 2; h >= 1; h >>= 1) {
    if (t < h) {
      const double o = red[t + h];
      const int32_t oi = redi[t + h];
      if (o > red[t] || (o == red[t] && oi < redi[t])) { red[t] = o; redi[t] = oi; }
    }
    __syncthreads();
  }
  const int32_t c0 = redi[0];
  const double n0 = sqrt(red[0]);
  __syncthreads();
  const double trace = plage_block_sum(tr, red);
  for (int32_t i = t; i < k; i += kPlageThreads) u[i] = C[i + c0 * ld] / n0;
  __syncthreads();

  double lambda = 0.0, r = 0.0;
  int32_t it = 0, conv = 0;
  for (it = 1; it <= maxit; ++it) {
    for (int32_t i = t; i < k; i += kPlageThreads) {
      double acc = 0.0;
      for (int32_t j = 0; j < k; ++j) {
        const double p = C[i + j * ld] * u[j];
        acc = acc + p;
      }
      y[i] = acc;
    }
    __syncthreads();
    double pl = 0.0;
    for (int32_t i = t; i < k; i += kPlageThreads) {
      const double p = u[i] * y[i];
      pl = pl + p;
    }
    lambda = plage_block_sum(pl, red);
    double pr = 0.0;
    for (int32_t i = t; i < k; i += kPlageThreads) {
      const double lu = lambda * u[i];
      const double d = y[i] - lu;
      const double p = d * d;
      pr = pr + p;
    }
    r = sqrt(plage_block_sum(pr, red));
    if (r <= tol * lambda) { conv = 1; break; }
    if (it == maxit) break;
    double pn = 0.0;
    for (int32_t i = t; i < k; i += kPlageThreads) {
      const double p = y[i] * y[i];
      pn = pn + p;
    }
    const double ny = sqrt(plage_block_sum(pn, red));
    for (int32_t i = t; i < k; i += kPlageThreads) u[i] = y[i] / ny;
    __syncthreads();
  }

  // the orientation
  double ps = 0.0, pa = 0.0, pm = 0.0;
  for (int32_t i = t; i < k; i += kPlageThreads) {
    ps = ps + u[i];
    pa = pa + fabs(u[i]);
    pm = fmax(pm, fabs(u[i]));
  }
  const double su = plage_block_sum(ps, red);
  const double au = plage_block_sum(pa, red);
  red[t] = pm;
  __syncthreads();
  for (int h = kPlageThreads / 2; h >= 1; h >>= 1) {
    if (t < h) red[t] = fmax(red[t], red[t + h]);
    __syncthreads();
  }
  const double mx = red[0];
  __syncthreads();
  bool flip;
  if (fabs(su) > au * (1.0 / 1048576.0)) {
    flip = su < 0.0;
  } else {
    int32_t first = k;
    for (int32_t i = t; i < k; i += kPlageThreads)
      if (fabs(u[i]) >= mx * 0.5) { first = i; break; }
    redi[t] = first;
    __syncthreads();
    for (int h = kPlageThreads / 2; h >= 1; h >>= 1) {
      if (t < h) redi[t] = min(redi[t], redi[t + h]);
      __syncthreads();
    }
    first = redi[0];
    flip = first < k && u[first] < 0.0;
  }
  for (int32_t i = t; i < k; i += kPlageThreads) {
    const double v = flip ? -u[i] : u[i];
    U[p0 + i] = v;
    if (L != nullptr) L[p0 + Cpos[p0 + i]] = v;
  }
  if (t == 0) {
    stats[s] = (double)k;
    stats[s + (int64_t)m] = lambda;
    stats[s + 2 * (int64_t)m] = lambda / trace;
    stats[s + 3 * (int64_t)m] = (double)it;
    stats[s + 4 * (int64_t)m] = r / lambda;
    stats[s + 5 * (int64_t)m] = (double)conv;
  }
}

// S[s + j lds] = (sum_i u_i z_i,j0+j, the kept members in G's order from 0.0) / sqrt(lambda), one thread per (set, sample)
__global__ void __launch_bounds__(256)
plage_project_kernel(const double* __restrict__ Zg, int64_t ldz, const int32_t* __restrict__ Gp, const int32_t* __restrict__ Ci,
                     const int32_t* __restrict__ keff, const int32_t* __restrict__ nanflag, const double* __restrict__ U,
                     const double* __restrict__ stats, int32_t m, int32_t j0, int32_t nj, double* __restrict__ S, int64_t lds) {
  const int32_t s = blockIdx.y;
  const int32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nj) return;
  const int32_t k = keff[s], p0 = Gp[s];
  double out = plage_nan();
  if (k > 0 && nanflag[s] == 0) {
    const double sq = sqrt(stats[s + (int64_t)m]);
    double acc = 0.0;
    for (int32_t i = 0; i < k; ++i) {
      const double p = U[p0 + i] * Zg[(int64_t)Ci[p0 + i] * ldz + j0 + j];
      acc = acc + p;
    }
    out = acc / sq;
  }
  S[s + (int64_t)j * lds] = out;
}

__global__ void __launch_bounds__(256)
zscore_epilogue_kernel(double* __restrict__ S, int64_t lds, int32_t m, int32_t n, const int32_t* __restrict__ keff,
                       const int32_t* __restrict__ nanflag) {
  const int32_t s = blockIdx.x * 256 + threadIdx.x;
  const int32_t j = blockIdx.y;
  if (s >= m || j >= n) return;
  const int32_t k = keff[s];
  const double v = S[s + (int64_t)j * lds];
  S[s + (int64_t)j * lds] = (k == 0 || nanflag[s] != 0) ? plage_nan() : v / sqrt((double)k);
}

}  // namespace

void debug_plage_set_gram(int mode) { g_plage_gram.store(mode); }

int64_t plage_row_ld(int32_t n) { return ((int64_t)n + kGramChunk - 1) / kGramChunk * kGramChunk; }

int launch_plage_moments(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t n, double* mean, double* sd,
                         int32_t* flag) {
  PH_REQUIRE(g >= 0 && n >= 2 && ldx >= g, "plage: bad dims g=%d n=%d ldx=%lld", g, n, (long long)ldx);
  if (g == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(plage_row_moments_kernel, dim3((unsigned)((g + 255) / 256)), dim3(256), 0, ctx->stream, X, ldx, g, n, mean,
                     sd, flag);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_plage_standardize_columns(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t j0, int32_t nj,
                                     const double* mean, const double* sd, const int32_t* flag, double* Z, int64_t ldz) {
  PH_REQUIRE(g >= 0 && j0 >= 0 && nj >= 0 && ldx >= g && ldz >= g, "plage: bad dims g=%d columns [%d, %d)", g, j0, j0 + nj);
  if (g == 0 || nj == 0) return PLAIDHIP_OK;
  for (int32_t c0 = 0; c0 < nj; c0 += 65535) {   // (gridDim.y)
    const int32_t nc = std::min<int32_t>(65535, nj - c0);
    hipLaunchKernelGGL(plage_standardize_cm_kernel, dim3((unsigned)((g + 255) / 256), (unsigned)nc), dim3(256), 0, ctx->stream, X,
                       ldx, g, j0 + c0, nc, mean, sd, flag, Z + (int64_t)c0 * ldz, ldz);
  }
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_plage_standardize_rows(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t n, const double* mean,
                                  const double* sd, const int32_t* flag, double* Zg, int64_t ldz) {
  PH_REQUIRE(g >= 0 && n >= 2 && ldx >= g && ldz == plage_row_ld(n), "plage: bad dims g=%d n=%d ldz=%lld", g, n, (long long)ldz);
  PH_REQUIRE((ldz + 31) / 32 <= 65535, "plage: %d samples (at most %d)", n, 65535 * 32);
  if (g == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(plage_standardize_gm_kernel, dim3((unsigned)((g + 31) / 32), (unsigned)((ldz + 31) / 32)), dim3(256), 0,
                     ctx->stream, X, ldx, g, n, mean, sd, flag, Zg, ldz);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_plage_compact(plaidhip_ctx* ctx, const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* flag, int32_t* Ci,
                         int32_t* Cpos, int32_t* keff, int32_t* nanflag) {
  if (m <= 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(plage_compact_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream, Gp, Gi, m, flag, Ci, Cpos, keff, nanflag);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// The Gram matrices and eigenvectors of every set, in batches of sets whose matrices fit a workspace sized from the free
// memory.  The sets are taken by decreasing nominal size (their own order among equals), so a batch's tile counts are
// close to its first set's, which sizes the launch.  A set's results depend on that set alone: the batches, and with them
// the free memory, decide nothing.  hGp: the host's Gp; the other pointers are device pointers.
int launch_plage_sets(plaidhip_ctx* ctx, const double* Zg, int64_t ldz, const int32_t* hGp, const int32_t* Gp, const int32_t* Ci,
                      const int32_t* Cpos, const int32_t* keff, const int32_t* nanflag, int32_t m, double tol, int32_t maxit,
                      double* U, double* stats, double* L) {
  if (m <= 0) return PLAIDHIP_OK;
  std::vector<int32_t> order((size_t)m);
  std::iota(order.begin(), order.end(), 0);
  auto nominal = [&](int32_t s) { return hGp[s + 1] - hGp[s]; };
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return nominal(a) > nominal(b); });
  auto padded = [&](int32_t s) { return ((int64_t)nominal(s) + kGramTile - 1) / kGramTile * kGramTile; };
  size_t free_b = 0, total_b = 0;
  PH_HIP(hipMemGetInfo(&free_b, &total_b));
  const int64_t largest = padded(order[0]) * padded(order[0]);
  const int64_t budget = std::max<int64_t>(largest, (int64_t)std::min<size_t>(free_b / 2, (size_t)2 << 30) / 8);
  // the batches: [b0, b1) of `order`, and every set's offset (in doubles) into the workspace of its batch
  std::vector<int64_t> coff((size_t)m);
  std::vector<int32_t> starts{0};
  int64_t used = 0, ws_doubles = 1;
  for (int32_t q = 0; q < m; ++q) {
    const int64_t need = padded(order[(size_t)q]) * padded(order[(size_t)q]);
    if (q > starts.back() && (used + need > budget || q - starts.back() >= kMaxBatchSets)) {
      starts.push_back(q);
      used = 0;
    }
    coff[(size_t)q] = used;
    used += need;
    ws_doubles = std::max(ws_doubles, used);
  }
  starts.push_back(m);
  DevBuf dorder, dcoff, dws;
  PH_TRY(dorder.alloc((size_t)m * 4));
  PH_TRY(dcoff.alloc((size_t)m * 8));
  PH_TRY(dws.alloc((size_t)ws_doubles * 8));
  PH_HIP(hipMemcpyAsync(dorder.p, order.data(), (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
  PH_HIP(hipMemcpyAsync(dcoff.p, coff.data(), (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
  PH_FULL_LDS(ctx, plage_eigen_kernel);
  for (size_t b = 0; b + 1 < starts.size(); ++b) {
    const int32_t b0 = starts[b], nb = starts[b + 1] - b0;
    const int32_t kmax = (int32_t)padded(order[(size_t)b0]);
    const bool mfma = g_plage_gram.load() == 1;
    const int64_t side = mfma ? kGramTile : kVecTile;
    const int64_t T = (kmax + side - 1) / side, tiles = T * (T + 1) / 2;
    if (tiles > 0) {
      const dim3 grid((unsigned)((tiles + kGramWaves - 1) / kGramWaves), (unsigned)nb);
      hipLaunchKernelGGL(mfma ? plage_gram_mfma_kernel : plage_gram_kernel, grid, dim3(kPlageThreads), 0, ctx->stream, Zg, ldz, Gp,
                         Ci, keff, nanflag, dorder.as<int32_t>() + b0, dcoff.as<int64_t>() + b0, dws.as<double>());
      PH_HIP(hipGetLastError());
    }
    const size_t lds = ((size_t)2 * std::max(kmax, 1) + kPlageThreads) * 8 + (size_t)kPlageThreads * 4;
    hipLaunchKernelGGL(plage_eigen_kernel, dim3((unsigned)nb), dim3(kPlageThreads), lds, ctx->stream, Gp, Cpos, keff, nanflag,
                       dorder.as<int32_t>() + b0, dcoff.as<int64_t>() + b0, dws.as<double>(), std::max(kmax, 1), m, tol, maxit, U,
                       stats, L);
    PH_HIP(hipGetLastError());
  }
  PH_HIP(hipStreamSynchronize(ctx->stream));   // (order, coff and the buffers above live until here)
  return PLAIDHIP_OK;
}

int launch_plage_project(plaidhip_ctx* ctx, const double* Zg, int64_t ldz, const int32_t* Gp, const int32_t* Ci,
                         const int32_t* keff, const int32_t* nanflag, const double* U, const double* stats, int32_t m, int32_t j0,
                         int32_t nj, double* S, int64_t lds) {
  PH_REQUIRE(m >= 0 && j0 >= 0 && nj >= 0 && j0 + (int64_t)nj <= ldz && lds >= m, "plage: bad dims m=%d columns [%d, %d)", m, j0,
             j0 + nj);
  if (m == 0 || nj == 0) return PLAIDHIP_OK;
  for (int32_t s0 = 0; s0 < m; s0 += 65535) {   // (gridDim.y)
    const int32_t ns = std::min<int32_t>(65535, m - s0);
    hipLaunchKernelGGL(plage_project_kernel, dim3((unsigned)((nj + 255) / 256), (unsigned)ns), dim3(256), 0, ctx->stream, Zg, ldz,
                       Gp + s0, Ci, keff + s0, nanflag + s0, U, stats + s0, m, j0, nj, S + s0, lds);
  }
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_zscore_epilogue(plaidhip_ctx* ctx, double* S, int64_t lds, int32_t m, int32_t n, const int32_t* keff,
                           const int32_t* nanflag) {
  if (m <= 0 || n <= 0) return PLAIDHIP_OK;
  for (int32_t c0 = 0; c0 < n; c0 += 65535) {
    const int32_t nc = std::min<int32_t>(65535, n - c0);
    hipLaunchKernelGGL(zscore_epilogue_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)nc), dim3(256), 0, ctx->stream,
                       S + (int64_t)c0 * lds, lds, m, nc, keff, nanflag);
  }
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
