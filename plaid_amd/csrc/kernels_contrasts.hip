// plaid.test.contrasts: the two-group row moments of kernels_stats.hip for C contrasts in one pass over the matrix.
//
// A contrast is a label per sample column: 0, 1, or "takes no part" (-1).  What differs between the contrasts is only
// which accumulator a column's value is added to, and that is the same for every row of the column -- wavefront-uniform.
// So the matrix (the score rows S, or dense X) is read once per tile of kContrastTile contrasts, not once per contrast:
// a thread owns two adjacent rows, walks a block of kRowColBlock columns in ascending order (row_pair.h), and keeps the
// two group accumulators of every contrast of its tile in registers.
//
// The labels of a tile are two bit masks per column ("in group 0", "in group 1", bit t = contrast tile * T + t), built
// once per call by contrast_masks_kernel and read through scalar loads; the bit positions are compile-time after
// unrolling.  Every accumulator performs exactly the additions of row_group_sums_kernel / row_group_ssd_kernel /
// row_group_shifted_partials_kernel, in their order:
//     s += in_group ? v : 0.0          per column of the block, ascending
//     part[block][contrast][group][row]
//     blocks added in ascending order, from an optional seed (reduce_blocks_flat_kernel)
// so a contrast without an excluded sample has the bits of the one-label kernels.  The select form matters: an excluded
// column adds +0.0 whatever it holds (NaN, Inf).
#include "common.h"
#include "row_pair.h"

namespace plaidhip {

constexpr int kContrastTile = PLAIDHIP_CONTRAST_TILE;

// masks[tile][c] = {bits of "Y[c, tile * T + t] == 0", bits of "== 1"}; Y: n x C column-major, leading dimension ldy
__global__ void __launch_bounds__(256)
contrast_masks_kernel(const int32_t* __restrict__ Y, int64_t ldy, int32_t n, int32_t C, uint2* __restrict__ masks) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int tile = blockIdx.y;
  if (c >= n) return;
  uint32_t b0 = 0, b1 = 0;
  for (int t = 0; t < kContrastTile; ++t) {
    const int j = tile * kContrastTile + t;
    if (j >= C) break;
    const int lab = Y[(int64_t)j * ldy + c];
    b0 |= (lab == 0 ? 1u : 0u) << t;
    b1 |= (lab == 1 ? 1u : 0u) << t;
  }
  masks[(int64_t)tile * n + c] = make_uint2(b0, b1);
}

// The block partials of the sums (kSsd false) or of the sums of squared deviations from mean ([C][2][rows]) of every
// contrast of tile blockIdx.z, over the rows of S (rows x n, leading dimension ld) with v = (S[r, c] - med[c]) + add
// applied on load (med == nullptr: v = S[r, c]).  part: [nblk][C][2][rows].  The walk is row_pair.h's (kUn = 8).
template <bool kSsd, bool kWide>
__global__ void __launch_bounds__(256)
row_contrast_partials_kernel(const double* __restrict__ S, int64_t ld, int32_t rows, int32_t n,
                             const uint2* __restrict__ masks, int32_t C, const double* __restrict__ med, double add,
                             const double* __restrict__ mean, double* __restrict__ part) {
  constexpr int T = kContrastTile;
  const RowPair g = row_pair_block(rows, n);
  const int r = g.r;
  const int j0 = blockIdx.z * T;                      // the tile's first contrast
  const int nt = C - j0 < T ? C - j0 : T;             // its live contrasts (the others' masks are 0, nothing is written)
  const uint2* __restrict__ mk = masks + (int64_t)blockIdx.z * n;
  if (r >= rows) return;
  const bool two = g.two;
  const bool shift = med != nullptr;
  double m0a[T], m1a[T], m0b[T], m1b[T];
  double s0a[T], s1a[T], s0b[T], s1b[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    m0a[t] = m1a[t] = m0b[t] = m1b[t] = 0.0;
    s0a[t] = s1a[t] = s0b[t] = s1b[t] = 0.0;
    if (kSsd && t < nt) {
      const double* mj = mean + (int64_t)(j0 + t) * 2 * rows;
      m0a[t] = mj[r];
      m1a[t] = mj[rows + r];
      if (two) { m0b[t] = mj[r + 1]; m1b[t] = mj[rows + r + 1]; }
    }
  }
  auto accumulate = [&](int c, double xa, double xb) {
    const uint2 k = mk[c];   // wave-uniform
    double va = xa, vb = xb;
    if (shift) {
      const double md = med[c];
      va = (xa - md) + add;
      vb = (xb - md) + add;
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const bool in0 = ((k.x >> t) & 1u) != 0, in1 = ((k.y >> t) & 1u) != 0;
      if (kSsd) {
        const double d0a = va - m0a[t], d1a = va - m1a[t], d0b = vb - m0b[t], d1b = vb - m1b[t];
        s0a[t] += in0 ? d0a * d0a : 0.0;
        s1a[t] += in1 ? d1a * d1a : 0.0;
        s0b[t] += in0 ? d0b * d0b : 0.0;
        s1b[t] += in1 ? d1b * d1b : 0.0;
      } else {
        s0a[t] += in0 ? va : 0.0;
        s1a[t] += in1 ? va : 0.0;
        s0b[t] += in0 ? vb : 0.0;
        s1b[t] += in1 ? vb : 0.0;
      }
    }
  };
  row_pair_walk<kWide, 8>(S, ld, g, accumulate);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t >= nt) break;
    double* p = part + ((int64_t)blockIdx.y * C + (j0 + t)) * 2 * rows;
    p[r] = s0a[t];
    p[rows + r] = s1a[t];
    if (two) {
      p[r + 1] = s0b[t];
      p[rows + r + 1] = s1b[t];
    }
  }
}

// out[i] = seed[i] (0 without a seed) + part[0][i] + part[1][i] + ..., i over the len = C * 2 * rows sums of a block:
// reduce_blocks_kernel's additions (scale 1) and reduce_blocks_seeded_kernel's, for every contrast and group at once
__global__ void __launch_bounds__(256)
reduce_blocks_flat_kernel(const double* __restrict__ part, int64_t len, int32_t nblk, const double* __restrict__ seed,
                          double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  double s = seed != nullptr ? seed[i] : 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * len + i];
  out[i] = s;
}

// fold_change_kernel for every contrast: mean [C][2][rows] -> F [C][2][ld2] = [fc_j, fc_j^2]
__global__ void __launch_bounds__(256)
fold_change_contrasts_kernel(const double* __restrict__ mean, int32_t rows, int64_t ld2, double* __restrict__ F) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const double* mj = mean + (int64_t)blockIdx.y * 2 * rows;
  double* Fj = F + (int64_t)blockIdx.y * 2 * ld2;
  const double fc = mj[rows + r] - mj[r];
  Fj[r] = fc;
  Fj[ld2 + r] = fc * fc;
}

int64_t contrast_tiles(int32_t C) { return ((int64_t)C + kContrastTile - 1) / kContrastTile; }

// doubles of the block partials [nblk][C][2][rows]
int64_t row_contrast_ws_doubles(int32_t rows, int32_t n, int32_t C) {
  const int64_t nblk = (n + kRowColBlock - 1) / kRowColBlock;
  return 2 * (int64_t)rows * C * (nblk > 0 ? nblk : 1);
}

// bytes of the label masks of n columns and C contrasts
int64_t contrast_mask_bytes(int32_t n, int32_t C) {
  return contrast_tiles(C) * (int64_t)(n > 0 ? n : 1) * (int64_t)sizeof(uint2);
}

int launch_contrast_masks(plaidhip_ctx* ctx, const int32_t* d_Y, int64_t ldy, int32_t n, int32_t C, void* d_masks) {
  if (n == 0 || C == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(contrast_masks_kernel, dim3((n + 255) / 256, (unsigned)contrast_tiles(C)), dim3(256), 0, ctx->stream,
                     d_Y, ldy, n, C, static_cast<uint2*>(d_masks));
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// launch_row_group_shifted_partials for C contrasts (d_masks: launch_contrast_masks of the same n and C); ws:
// row_contrast_ws_doubles(rows, n, C) doubles
int launch_row_contrast_partials(plaidhip_ctx* ctx, const double* S, int64_t ld, int32_t rows, int32_t n,
                                 const void* d_masks, int32_t C, const double* d_med, double add, const double* d_mean,
                                 double* ws) {
  if (rows == 0 || n == 0 || C == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 511) / 512, nblk, (unsigned)contrast_tiles(C));
  const uint2* mk = static_cast<const uint2*>(d_masks);
  dispatch_flag(d_mean != nullptr, [&](auto ssd) {
    dispatch_flag(row_pair_wide(rows, {ld}, {S}), [&](auto wide) {
      hipLaunchKernelGGL((row_contrast_partials_kernel<decltype(ssd)::value, decltype(wide)::value>), grid, dim3(256), 0, ctx->stream,
                         S, ld, rows, n, mk, C, d_med, add, d_mean, ws);
    });
  });
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// d_out[i] = d_seed[i] (0 when null) + the partials of ws over the blocks of n columns, in order; len sums per block
int launch_reduce_blocks_flat(plaidhip_ctx* ctx, const double* ws, int64_t len, int32_t n, const double* d_seed,
                              double* d_out) {
  if (len == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  hipLaunchKernelGGL(reduce_blocks_flat_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, ctx->stream, ws, len, nblk,
                     d_seed, d_out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_fold_change_contrasts(plaidhip_ctx* ctx, const double* d_mean, int32_t rows, int32_t C, int64_t ld2, double* d_F) {
  if (rows == 0 || C == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(fold_change_contrasts_kernel, dim3((rows + 255) / 256, C), dim3(256), 0, ctx->stream, d_mean, rows, ld2,
                     d_F);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
