// Device loops the exact scorers share (kernels_rank / _walk / _ks / _sing / _trunc.hip): the items of rank columns, the
// m x n scores, and the {min, max, any NaN} partial of a workgroup.  Integer index arithmetic and selects only: a kernel's
// floating-point work stays in its own file, under that file's contraction setting.
#pragma once

#include <algorithm>

#include "common.h"

namespace plaidhip {

// 2^26: (a rank, a row) -> one exact double, y = rank-like * 2^26 + row-like, for columns of fewer than 2^26 values.  The
// tie-free columns of ties.method = "first" / "last" / "dense" and of launch_last_ranks are built on it.
constexpr double kTieFreeShift = 67108864.0;

inline dim3 rank_cols_grid(const RankCols& t) {   // RankCols: common.h
  return dim3((unsigned)std::min<int64_t>(((int64_t)t.g + 255) / 256, 64), (unsigned)std::min(t.n, 16384));
}

struct RankItem {
  int c;                   // column
  int64_t x, r, s;         // where item i of the column sits in the input, in the ranks and in the scratch columns
  int32_t i, cnt;          // item i of the column's cnt
};

template <typename F>
__device__ __forceinline__ void for_each_rank_item(const RankCols& t, F f) {   // grid: rank_cols_grid, 256 threads
  for (int c = blockIdx.y; c < t.n; c += gridDim.y) {
    int64_t xb, rb, sb;
    int32_t cnt;
    if (t.Xp != nullptr) { xb = rb = sb = t.Xp[c]; cnt = t.Xp[c + 1] - t.Xp[c]; }
    else { xb = (int64_t)c * t.ldx; rb = (int64_t)c * t.ldr; sb = (int64_t)c * t.lds; cnt = t.g; }
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x)
      f(RankItem{c, xb + i, rb + i, sb + i, i, cnt});
  }
}

// f(c, j, at) for every score (set j, column c) of an m x n block, at = c lds + j; a one-dimensional grid
template <typename F>
__device__ __forceinline__ void for_each_score(int32_t m, int32_t n, int64_t lds, F f) {
  const int64_t total = (int64_t)m * n;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = e / m, j = e - c * m;
    f(c, j, c * lds + j);
  }
}

// one value into a thread's {min, max, any NaN}; start from {INFINITY, -INFINITY, 0.0}
__device__ __forceinline__ void score_range_take(double es, double& mn, double& mx, double& nf) {
  if (es != es) nf = 1.0;
  else { mn = es < mn ? es : mn; mx = es > mx ? es : mx; }
}

// the workgroup's (256 threads) partial into part[3 blockIdx.x ..]; every thread calls it.  min / max select: any order
// gives the same values.
__device__ __forceinline__ void score_range_block(double mn, double mx, double nf, double* __restrict__ part) {
  __shared__ double s_mn[4], s_mx[4], s_nf[4];
  for (int o = 32; o >= 1; o >>= 1) {
    const double a = __shfl_xor(mn, o), b = __shfl_xor(mx, o), f = __shfl_xor(nf, o);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
    nf = f > nf ? f : nf;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; s_nf[wave] = nf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      mn = s_mn[w] < mn ? s_mn[w] : mn;
      mx = s_mx[w] > mx ? s_mx[w] : mx;
      nf = s_nf[w] > nf ? s_nf[w] : nf;
    }
    part[3 * (int64_t)blockIdx.x] = mn;
    part[3 * (int64_t)blockIdx.x + 1] = mx;
    part[3 * (int64_t)blockIdx.x + 2] = nf;
  }
}

}  // namespace plaidhip
