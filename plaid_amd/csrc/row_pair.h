// The two-row column walk of the dense row passes, once: row_group_shifted_partials_kernel
// (kernels_stats.hip), row_contrast_partials_kernel (kernels_contrasts.hip), row_design_rss_kernel (kernels_lmfit.hip),
// row_design_w_sums_kernel and row_design_w_rss_kernel (kernels_lmfit_w.hip), camera_residual_kernel (kernels_camera.hip),
// fry_residual_kernel (kernels_fry.hip) and roast_rotate_kernel (kernels_roast.hip).  row_design_effects_kernel
// (kernels_lmfit.hip) takes the geometry and the load from here and keeps the loop in its own body: on row_pair_walk it was
// 4 to 8 % slower than its parent at small shapes (profiles/row_pair_walk.md).
//
// A thread owns two adjacent rows of a column-major matrix and walks a range of columns in ascending order -- the block of
// kRowColBlock columns of blockIdx.y, or all of them.  kUn columns are loaded before the first of them is used (the matrices
// are far larger than the Infinity Cache: the loads of a wave must overlap), a scalar tail follows the last full kUn.  kWide
// (rows and every leading dimension even, every base 16-byte aligned: row_pair_wide) reads both rows of a column with one
// 16-byte load, otherwise with two 8-byte ones.  What is done with a column is the kernel's visitor, in the kernel's own
// file: those files differ in fp contraction, and this header holds no floating-point expression other than the fma written
// out in row_pair_chain, so it means the same under both.  Included by .hip files only (no host translation unit sees it);
// the launchers' helpers -- row_pair_wide, dispatch_flag, dispatch_p -- stand after the walk.
#pragma once

#include <initializer_list>
#include <type_traits>

#include "common.h"

namespace plaidhip {

// The one column block of every row pass: launch_reduce_blocks_flat and the column cuts of shard.h count in it.
constexpr int kRowColBlock = 128;

typedef double row_pair_f64x2 __attribute__((ext_vector_type(2)));

struct RowPair {
  int r;        // the first of the thread's two rows (the kernel returns when r >= rows)
  bool two;     // false only for the last row of an odd `rows`: never wide
  int c0, c1;   // its columns
};

// rows 2 t and 2 t + 1 of thread t = blockIdx.x * 256 + threadIdx.x, over the columns [c0, c1)
__device__ __forceinline__ RowPair row_pair_columns(int32_t rows, int c0, int c1) {
  RowPair g;
  g.r = 2 * (blockIdx.x * 256 + threadIdx.x);
  g.two = g.r + 1 < rows;
  g.c0 = c0;
  g.c1 = c1;
  return g;
}

// ... over column block blockIdx.y of n columns
__device__ __forceinline__ RowPair row_pair_block(int32_t rows, int32_t n) {
  const int c0 = blockIdx.y * kRowColBlock;
  return row_pair_columns(rows, c0, c0 + kRowColBlock < n ? c0 + kRowColBlock : n);
}

// Both rows of one column, q = its address of row r.  kNonTemporal: a matrix that is streamed through once per launch.
template <bool kWide, bool kNonTemporal>
__device__ __forceinline__ void row_pair_load(const double* q, bool two, double& xa, double& xb) {
  if (kWide) {
    const row_pair_f64x2* q2 = reinterpret_cast<const row_pair_f64x2*>(q);
    const row_pair_f64x2 v = kNonTemporal ? __builtin_nontemporal_load(q2) : *q2;
    xa = v.x;
    xb = v.y;
  } else if (kNonTemporal) {
    xa = __builtin_nontemporal_load(q);
    xb = two ? __builtin_nontemporal_load(q + 1) : 0.0;
  } else {
    xa = q[0];
    xb = two ? q[1] : 0.0;
  }
}

template <bool kWide>
__device__ __forceinline__ void row_pair_store(double* o, bool two, double za, double zb) {
  if (kWide) {
    row_pair_f64x2 v;
    v.x = za;
    v.y = zb;
    *reinterpret_cast<row_pair_f64x2*>(o) = v;
  } else {
    o[0] = za;
    if (two) o[1] = zb;
  }
}

// visit(c, xa, xb) for every column of g, ascending, x from A
template <bool kWide, int kUn, bool kNonTemporal = true, class Visit>
__device__ __forceinline__ void row_pair_walk(const double* __restrict__ A, int64_t ld, const RowPair& g, Visit visit) {
  int c = g.c0;
  for (; c + kUn <= g.c1; c += kUn) {
    double xa[kUn], xb[kUn];
#pragma unroll
    for (int u = 0; u < kUn; ++u) row_pair_load<kWide, kNonTemporal>(A + (int64_t)(c + u) * ld + g.r, g.two, xa[u], xb[u]);
#pragma unroll
    for (int u = 0; u < kUn; ++u) visit(c + u, xa[u], xb[u]);
  }
  for (; c < g.c1; ++c) {
    double xa, xb;
    row_pair_load<kWide, kNonTemporal>(A + (int64_t)c * ld + g.r, g.two, xa, xb);
    visit(c, xa, xb);
  }
}

// The walk with a second matrix beside A: visit(c, xa, xb, wa, wb), w from Wt (A's leading dimension) or, without kWt,
// 1.0 and Wt is not read
template <bool kWide, int kUn, bool kWt, class Visit>
__device__ __forceinline__ void row_pair_walk2(const double* __restrict__ A, const double* __restrict__ Wt, int64_t ld,
                                               const RowPair& g, Visit visit) {
  int c = g.c0;
  for (; c + kUn <= g.c1; c += kUn) {
    double xa[kUn], xb[kUn], wa[kUn], wb[kUn];
#pragma unroll
    for (int u = 0; u < kUn; ++u) {
      row_pair_load<kWide, true>(A + (int64_t)(c + u) * ld + g.r, g.two, xa[u], xb[u]);
      if (kWt) row_pair_load<kWide, true>(Wt + (int64_t)(c + u) * ld + g.r, g.two, wa[u], wb[u]);
      else wa[u] = wb[u] = 1.0;
    }
#pragma unroll
    for (int u = 0; u < kUn; ++u) visit(c + u, xa[u], xb[u], wa[u], wb[u]);
  }
  for (; c < g.c1; ++c) {
    double xa, xb, wa = 1.0, wb = 1.0;
    row_pair_load<kWide, true>(A + (int64_t)c * ld + g.r, g.two, xa, xb);
    if (kWt) row_pair_load<kWide, true>(Wt + (int64_t)c * ld + g.r, g.two, wa, wb);
    visit(c, xa, xb, wa, wb);
  }
}

// The host's side of kWide (a null pointer counts as aligned: an operand that is not there)
inline bool row_pair_wide(int32_t rows, std::initializer_list<int64_t> lds, std::initializer_list<const void*> bases) {
  bool wide = (rows & 1) == 0;
  for (const int64_t ld : lds) wide = wide && (ld & 1) == 0;
  for (const void* b : bases) wide = wide && (reinterpret_cast<uintptr_t>(b) & 15u) == 0;
  return wide;
}

// launch(std::bool_constant<flag>{}): a run-time flag as a template argument
template <class Launch>
inline void dispatch_flag(bool flag, Launch&& launch) {
  if (flag) launch(std::true_type{});
  else launch(std::false_type{});
}

// ---- the residual kernels: a thread's p effects of one fit in registers, r = x - sum_k Q_f[c, k] e_k ------------------------

// launch(std::integral_constant<int, kP>{}) with p rounded up to kP = 4, 8, 16 or 32 effects in registers per row.  Where p is
// capped (PLAIDHIP_LIMMA_NA_MAX_COEF) kMax is the last instance, 16 or the cap itself, and none is made past it.
template <int kMax = 32, class Launch>
inline void dispatch_p(int p, Launch&& launch) {
  static_assert((kMax > 8 && kMax <= 16) || kMax == 32, "4, 8 and then kMax, or 16 and 32");
  if (p <= 4) launch(std::integral_constant<int, 4>{});
  else if (p <= 8) launch(std::integral_constant<int, 8>{});
  else if (kMax <= 16 || p <= 16) launch(std::integral_constant<int, (kMax < 16 ? kMax : 16)>{});
  else if constexpr (kMax == 32) launch(std::integral_constant<int, 32>{});
}

// "sample c is used by the fit": the bit of the fit's mean column jm in the masks of launch_lmfit_masks / launch_lmfit_w_table
// (n columns, tiles of PLAIDHIP_LIMMA_TILE); wave-uniform
struct RowPairFitBit {
  const uint32_t* __restrict__ mk;
  int bit;
  __device__ __forceinline__ bool operator()(int c) const { return ((mk[c] >> bit) & 1u) != 0; }
};
__device__ __forceinline__ RowPairFitBit row_pair_fit_bit(const uint32_t* __restrict__ masks, int64_t jm, int32_t n) {
  return RowPairFitBit{masks + (jm / PLAIDHIP_LIMMA_TILE) * n, (int)(jm % PLAIDHIP_LIMMA_TILE)};
}

// ea, eb = the p effects of fit f at the thread's rows, from E [nfit (p + 1)][rows]; 0.0 past p and for a row that is not there
template <int kP>
__device__ __forceinline__ void row_pair_effects(const double* __restrict__ E, int f, int p, int32_t rows, const RowPair& g,
                                                 double (&ea)[kP], double (&eb)[kP]) {
#pragma unroll
  for (int k = 0; k < kP; ++k) {
    ea[k] = eb[k] = 0.0;
    if (k < p) {
      const double* e = E + ((int64_t)f * (p + 1) + k) * rows;
      ea[k] = e[g.r];
      if (g.two) eb[k] = e[g.r + 1];
    }
  }
}

// The chain of step 2 of plaidhip_limma: r = fma(-Q_f[c, k], e_k, r) in ascending k, from ra = xa and rb = xb.  The expression
// is camera_chain_step's (camera.h), which the host references of plaid.camera and plaid.fry call; it is written out here
// because kernels_lmfit.hip and kernels_lmfit_w.hip, which wrote it out before, do not include camera.h.  Qf: the fit's n x p basis; its entries of a column are wave-uniform.
// Steps k, k + 1, ... are written out by recursion, not as a loop that leaves at k == p: as a function of its own that loop
// has min(kP, p) trips, which is no constant, and past kP = 8 it is no longer unrolled in full (ea and eb go to scratch).
template <int kP, int k = 0>
__device__ __forceinline__ void row_pair_chain(const double* __restrict__ Qf, int32_t n, int c, int p, const double (&ea)[kP],
                                               const double (&eb)[kP], double& ra, double& rb) {
  if constexpr (k < kP) {
    if (k >= p) return;
    const double nq = -Qf[(int64_t)k * n + c];
    ra = __builtin_fma(nq, ea[k], ra);
    rb = __builtin_fma(nq, eb[k], rb);
    row_pair_chain<kP, k + 1>(Qf, n, c, p, ea, eb, ra, rb);
  }
}

// The residual store of plaid.camera and plaid.fry: Z[r, c] = standardise(residual, the gene's scale, "c is used by fit f")
// for the rows x n matrix A, written as genes x n column-major (leading dimension ldz), the layout the dense crossprod reads.
// E [W][rows]: the effects of ALL samples; masks: launch_lmfit_masks of the same n and W.  gene_scale(r): the divisor of gene
// r, taken once per (thread, column block); it and standardise(residual, scale, used) are the including file's.
template <int kP, bool kWide, class GeneScale, class Standardise>
__device__ __forceinline__ void row_pair_residual_store(const double* __restrict__ A, int64_t ld, int32_t rows, int32_t n,
                                                        const double* __restrict__ Q, const uint32_t* __restrict__ masks,
                                                        int32_t p, int32_t f, const double* __restrict__ E,
                                                        double* __restrict__ Z, int64_t ldz, GeneScale gene_scale,
                                                        Standardise standardise) {
  const RowPair g = row_pair_block(rows, n);
  const RowPairFitBit used = row_pair_fit_bit(masks, (int64_t)f * (p + 1) + p, n);
  const double* __restrict__ Qf = Q + (int64_t)f * p * n;
  if (g.r >= rows) return;
  double ea[kP], eb[kP];
  row_pair_effects<kP>(E, f, p, rows, g, ea, eb);
  const double sa = gene_scale(g.r);
  const double sb = g.two ? gene_scale(g.r + 1) : __builtin_nan("");
  const int r = g.r;   // (copies for the visitor: with g captured, the 8-byte instances take two registers more)
  const bool two = g.two;
  row_pair_walk<kWide, 8>(A, ld, g, [&](int c, double xa, double xb) {
    const bool in = used(c);
    double ra = xa, rb = xb;
    row_pair_chain<kP>(Qf, n, c, p, ea, eb, ra, rb);
    const double za = standardise(ra, sa, in), zb = standardise(rb, sb, in);
    row_pair_store<kWide>(Z + (int64_t)c * ldz + r, two, za, zb);
  });
}

}  // namespace plaidhip
