// plaid.roast: the device passes (include/plaidhip.h: plaidhip_roast).
//
// roast_rotate_kernel: a thread holds two genes and 16 rotations.  It runs the walk of row_pair.h once over the raw residuals
// ([n][ldz], genes contiguous; kernels_fry.hip's residual pass with a divisor of 1.0), B = fma chain ascending from
// beta r0, and fuses steps 3 and 4 (roast.h): z goes out as [tile of 64 rotations][gene][64], the layout whose 64
// rotations of one gene the statistic kernels read with one 512-byte request.  The weights W ((n + 1) x ldw, row 0 = r0) are
// wave-uniform: scalar loads.
// roast_stat_kernel (mean, floormean, msq): a workgroup per (set, four tiles), a lane per rotation, the members in the
// order of Gi, one accumulator per side from 0.0.
// roast_mean50_kernel: a workgroup per set gathers the members' z of as many rotations as fit its LDS, selects the h-th
// largest key of every (rotation, side) bit by bit on order-preserving 64-bit keys (a wave per problem: one ballot and
// one population count per 64 members and bit), then sums the keys above it in the order of Gi.
// Both statistic kernels write the statistic as [set][rotation][4] (down, up, upordown, mixed) and/or add the exact counts
// #{stat_k >= stat_obs} with integer atomics.
#include "common.h"
#include "roast.h"
#include "row_pair.h"

#pragma clang fp contract(off)

namespace plaidhip {

constexpr int kRotTile = 64;    // rotations of a z tile
constexpr int kRotPer = 16;     // rotations a thread of the rotate kernel holds

template <bool kWide>
__global__ void __launch_bounds__(256)
roast_rotate_kernel(const double* __restrict__ Rz, int64_t ldz, int32_t rows, int32_t n, const double* __restrict__ beta,
                    const double* __restrict__ rss, const double* __restrict__ W, int64_t ldw, int32_t k0, int32_t k1,
                    RoastFit fit, int zscore, double* __restrict__ Z) {
  const RowPair g = row_pair_columns(rows, 0, n);
  const int r = g.r;
  const int kb = k0 + kRotPer * blockIdx.y;   // (k0 is a multiple of 64; ldw covers kb + 15)
  if (r >= rows) return;
  const bool two = g.two;
  const double ba = beta[r], bb = two ? beta[r + 1] : 0.0;
  double a[kRotPer], b[kRotPer];
  const double* __restrict__ w0 = W + kb;
#pragma unroll
  for (int t = 0; t < kRotPer; ++t) {
    const double r0 = w0[t];
    a[t] = ba * r0;
    b[t] = bb * r0;
  }
  auto step = [&](int c, double xa, double xb) {
    const double* __restrict__ wc = W + (int64_t)(c + 1) * ldw + kb;
#pragma unroll
    for (int t = 0; t < kRotPer; ++t) {
      const double w = wc[t];
      a[t] = roast_chain_step(xa, w, a[t]);
      b[t] = roast_chain_step(xb, w, b[t]);
    }
  };
  row_pair_walk<kWide, 4, false>(Rz, ldz, g, step);   // plain loads: every blockIdx.y reads Rz again
  const double ra = rss[r], rb = two ? rss[r + 1] : 0.0;
  const int64_t tile = (kb - k0) / kRotTile;
  double* __restrict__ o = Z + (tile * rows + r) * kRotTile + (kb - k0) % kRotTile;
#pragma unroll
  for (int t = 0; t < kRotPer; ++t) {
    if (kb + t < k1) {   // (the padding of the last tile is not written)
      o[t] = roast_zscore(roast_moderated_t(a[t], ba, ra, fit), fit.nu, zscore);
      if (two) o[kRotTile + t] = roast_zscore(roast_moderated_t(b[t], bb, rb, fit), fit.nu, zscore);
    }
  }
}

// z of rotations k0 .. k1 - 1 (k0 a multiple of 64) into Z [tile][rows][64], tile counted from k0 / 64.  ldw: a multiple of
// 16 that covers the rotations.
int launch_roast_rotate(plaidhip_ctx* ctx, const double* Rz, int64_t ldz, int32_t rows, int32_t n, const double* d_beta,
                        const double* d_rss, const double* d_W, int64_t ldw, int32_t k0, int32_t k1, RoastFit fit, int zscore,
                        double* Z) {
  if (rows == 0 || k1 <= k0) return PLAIDHIP_OK;
  const dim3 grid((rows + 511) / 512, (k1 - k0 + kRotPer - 1) / kRotPer);
  dispatch_flag(row_pair_wide(rows, {ldz}, {Rz}), [&](auto wide) {
    hipLaunchKernelGGL((roast_rotate_kernel<decltype(wide)::value>), grid, dim3(256), 0, ctx->stream, Rz, ldz, rows, n, d_beta, d_rss,
                       d_W, ldw, k0, k1, fit, zscore, Z);
  });
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// the observed column: z of plaid.limma's moderated t itself, as a one-rotation tile [rows][64] (entry 0 of every gene)
__global__ void __launch_bounds__(256)
roast_observed_kernel(const double* __restrict__ t, int32_t rows, double nu, int zscore, double* __restrict__ Z) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < rows) Z[(int64_t)r * kRotTile] = roast_zscore(t[r], nu, zscore);
}

int launch_roast_observed(plaidhip_ctx* ctx, const double* d_t, int32_t rows, double nu, int zscore, double* Z) {
  if (rows == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(roast_observed_kernel, dim3((rows + 255) / 256), dim3(256), 0, ctx->stream, d_t, rows, nu, zscore, Z);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// what a lane does with its four sides: the statistic to [set][rotation][4], the counts against the observed statistic
__device__ inline void roast_emit(int32_t s, int32_t k, int32_t nrot, bool valid, double down, double up, double mixed,
                                  double* __restrict__ stat, const double* __restrict__ obs, int32_t* __restrict__ cnt) {
  const double both = up > down ? up : down;
  const double v[4] = {down, up, both, mixed};
  if (stat != nullptr && valid) {
    double* o = stat + ((int64_t)s * nrot + k) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = v[e];
  }
  if (cnt != nullptr) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ge = valid && v[e] >= obs[(int64_t)s * 4 + e];
      const int c = __popcll(__ballot(ge));
      if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(cnt + (int64_t)s * 4 + e, c);
    }
  }
}

template <int kStat>
__global__ void __launch_bounds__(256)
roast_stat_kernel(const double* __restrict__ Z, int32_t rows, const int32_t* __restrict__ Gp, const int32_t* __restrict__ Gi,
                  int32_t k0, int32_t k1, int32_t nrot, double* __restrict__ stat, const double* __restrict__ obs,
                  int32_t* __restrict__ cnt) {
  const int s = blockIdx.x, lane = threadIdx.x & 63;
  const int tile = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (k0 + tile * kRotTile >= k1) return;   // (the whole wave: nothing below meets another wave)
  const int k = k0 + tile * kRotTile + lane;
  const bool valid = k < k1;
  const int g0 = Gp[s], g1 = Gp[s + 1];
  const double* __restrict__ zt = Z + (int64_t)tile * rows * kRotTile + lane;
  double sa = 0.0, sb = 0.0, sc = 0.0;
  auto take = [&](double z) {
    if (kStat == PLAIDHIP_ROAST_STAT_MEAN) {
      sa += z;
      sc += fabs(z);
    } else if (kStat == PLAIDHIP_ROAST_STAT_FLOORMEAN) {
      const double nz = -z;
      sa += nz > 0.0 ? nz : 0.0;
      sb += z > 0.0 ? z : 0.0;
      const double az = fabs(z);
      sc += az > PLAIDHIP_ROAST_SQRT_Q ? az : PLAIDHIP_ROAST_SQRT_Q;
    } else {
      const double zz = z * z;
      sa += z < 0.0 ? zz : 0.0;
      sb += z > 0.0 ? zz : 0.0;
      sc += zz;
    }
  };
  int h = g0;
  for (; h + 4 <= g1; h += 4) {
    double z[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) z[u] = valid ? zt[(int64_t)Gi[h + u] * kRotTile] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) take(z[u]);
  }
  for (; h < g1; ++h) take(valid ? zt[(int64_t)Gi[h] * kRotTile] : 0.0);
  const double mm = (double)(g1 - g0);   // (0 members: 0 / 0 = NaN on every side)
  double down, up;
  if (kStat == PLAIDHIP_ROAST_STAT_MEAN) {
    up = sa / mm;
    down = -sa / mm;
  } else {
    down = sa / mm;
    up = sb / mm;
  }
  roast_emit(s, k, nrot, valid, down, up, sc / mm, stat, obs, cnt);
}

constexpr int kM50Fixed = 384;   // doubles of LDS beside z: the thresholds and the sides of 64 rotations x 3

__global__ void __launch_bounds__(256)
roast_mean50_kernel(const double* __restrict__ Z, int32_t rows, const int32_t* __restrict__ Gp, const int32_t* __restrict__ Gi,
                    const int32_t* __restrict__ sel, int32_t zdoubles, int32_t k0, int32_t k1, int32_t nrot,
                    double* __restrict__ stat, const double* __restrict__ obs, int32_t* __restrict__ cnt) {
  extern __shared__ double roast_lds[];
  double* stau = roast_lds;          // [3][nr]
  double* sval = stau + 192;         // [3][nr]
  double* zs = roast_lds + kM50Fixed;   // [nr][stride], stride odd
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = sel[blockIdx.x];
  const int g0 = Gp[s], ms = Gp[s + 1] - g0;
  const int nk = k1 - k0;
  const double nan = __builtin_nan("");
  if (ms == 0 || ms > PLAIDHIP_ROAST_MEAN50_MAX) {   // no member, or a set above the cap: NaN, and no count
    if (stat != nullptr && blockIdx.y == 0)
      for (int t = tid; t < nk * 4; t += 256) stat[((int64_t)s * nrot + k0) * 4 + t] = nan;
    return;
  }
  const int stride = ms | 1;
  const int R = zdoubles / stride < kRotTile ? zdoubles / stride : kRotTile;   // (>= 1: the launcher sized the LDS for its sets)
  const int hsel = ms / 2 + 1;
  for (int klo = blockIdx.y * R; klo < nk; klo += gridDim.y * R) {
    const int nr = nk - klo < R ? nk - klo : R;
    __syncthreads();
    for (int idx = tid; idx < nr * ms; idx += 256) {
      const int i = idx / nr, rr = idx - i * nr, kk = klo + rr;
      zs[rr * stride + i] = Z[((int64_t)(kk / kRotTile) * rows + Gi[g0 + i]) * kRotTile + kk % kRotTile];
    }
    __syncthreads();
    // the h-th largest key of (rotation rr, side): a wave per problem, the bits from the top
    for (int pr = wave; pr < 3 * nr; pr += 4) {
      const int side = __builtin_amdgcn_readfirstlane(pr / nr), rr = pr - side * nr;   // (wave-uniform: said so)
      const double* zr = zs + rr * stride;
      uint64_t prefix = 0;
      int rem = hsel;
      if (ms <= 64) {
        const bool in = lane < ms;
        const uint64_t key = in ? roast_order_key(roast_mean50_key(zr[lane], side)) : 0;
        for (int bit = 63; bit >= 0; --bit) {
          const uint64_t cand = prefix | (1ull << bit);
          const int c = __popcll(__ballot(in && (key >> bit) == (cand >> bit)));
          if (c >= rem) prefix = cand;
          else rem -= c;
        }
      } else {
        for (int bit = 63; bit >= 0; --bit) {
          const uint64_t cand = prefix | (1ull << bit);
          int c = 0;
          for (int i0 = 0; i0 < ms; i0 += 64) {
            const int i = i0 + lane;
            const bool in = i < ms;
            const uint64_t key = in ? roast_order_key(roast_mean50_key(zr[i], side)) : 0;
            c += __popcll(__ballot(in && (key >> bit) == (cand >> bit)));
          }
          if (c >= rem) prefix = cand;
          else rem -= c;
        }
      }
      if (lane == 0) stau[pr] = roast_key_value(prefix);
    }
    __syncthreads();
    // (the keys above tau in the order of Gi) + (h - their number) tau, over h: a thread per problem
    if (tid < 3 * nr) {
      const int side = tid / nr, rr = tid - side * nr;
      const double* zr = zs + rr * stride;
      const double tau = stau[tid];
      double sum = 0.0;
      int above = 0;
      bool bad = false;
      for (int i = 0; i < ms; ++i) {
        const double key = roast_mean50_key(zr[i], side);
        bad = bad || key != key;
        if (key > tau) {
          sum += key;
          ++above;
        }
      }
      const double rest = (double)(hsel - above) * tau;
      sval[tid] = bad ? nan : (sum + rest) / (double)hsel;
    }
    __syncthreads();
    if (tid < kRotTile) {   // (one whole wave: roast_emit's ballots)
      const bool valid = tid < nr;
      const double up = valid ? sval[tid] : 0.0, down = valid ? sval[nr + tid] : 0.0, mixed = valid ? sval[2 * nr + tid] : 0.0;
      roast_emit(s, k0 + klo + tid, nrot, valid, down, up, mixed, stat, obs, cnt);
    }
  }
}

// The four sides of `set_statistic` for every (set, rotation k0 .. k1 - 1) from Z [tile][rows][64] (tile from k0 / 64).
// d_stat ([m][nrot][4], may be null) takes the statistic at its rotation; d_cnt ([m][4] int32, may be null) is raised by
// #{stat >= d_obs [m][4]}.  mean50 runs the sets in up to three size classes: d_sel (m set numbers, the classes one after the
// other), their counts and the LDS doubles each class needs for z (roast_mean50_classes).
int launch_roast_stats(plaidhip_ctx* ctx, const double* Z, int32_t rows, const int32_t* d_Gp, const int32_t* d_Gi, int32_t m,
                       int set_statistic, int32_t k0, int32_t k1, int32_t nrot, const int32_t* d_sel, const int32_t* class_cnt,
                       double* d_stat, const double* d_obs, int32_t* d_cnt) {
  if (m == 0 || k1 <= k0) return PLAIDHIP_OK;
  const int ntile = (k1 - k0 + kRotTile - 1) / kRotTile;
  const dim3 grid(m, (ntile + 3) / 4);
  switch (set_statistic) {
    case PLAIDHIP_ROAST_STAT_MEAN:
      hipLaunchKernelGGL((roast_stat_kernel<PLAIDHIP_ROAST_STAT_MEAN>), grid, dim3(256), 0, ctx->stream, Z, rows, d_Gp, d_Gi, k0,
                         k1, nrot, d_stat, d_obs, d_cnt);
      break;
    case PLAIDHIP_ROAST_STAT_FLOORMEAN:
      hipLaunchKernelGGL((roast_stat_kernel<PLAIDHIP_ROAST_STAT_FLOORMEAN>), grid, dim3(256), 0, ctx->stream, Z, rows, d_Gp, d_Gi,
                         k0, k1, nrot, d_stat, d_obs, d_cnt);
      break;
    case PLAIDHIP_ROAST_STAT_MSQ:
      hipLaunchKernelGGL((roast_stat_kernel<PLAIDHIP_ROAST_STAT_MSQ>), grid, dim3(256), 0, ctx->stream, Z, rows, d_Gp, d_Gi, k0, k1,
                         nrot, d_stat, d_obs, d_cnt);
      break;
    default: {
      int32_t off = 0;
      for (int cls = 0; cls < 3; ++cls) {
        const int32_t ns = class_cnt[cls];
        if (ns == 0) continue;
        const int32_t zd = roast_mean50_class_doubles(cls);
        const size_t lds = (size_t)(zd + kM50Fixed) * 8;
        if (lds > 48 * 1024) PH_FULL_LDS(ctx, roast_mean50_kernel);
        hipLaunchKernelGGL(roast_mean50_kernel, dim3(ns, ntile), dim3(256), lds, ctx->stream, Z, rows, d_Gp, d_Gi, d_sel + off, zd,
                           k0, k1, nrot, d_stat, d_obs, d_cnt);
        off += ns;
      }
    }
  }
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
