// plaid.romer: the device passes after the rotation (include/plaidhip.h: plaidhip_romer).  The rotated
// moderated t comes from roast_rotate_kernel (kernels_roast.hip, z-score "none") as [tile of 64 rotations][gene][64].
//
// romer_key_kernel: a workgroup takes 64 genes of the universe x one tile of 64 rotations.  It gathers the genes' 512-byte
// rows of t by the universe's index list (a lane per rotation: whole requests), turns the tile through LDS (rows padded by
// one double) and writes the two or three keys (romer.h) as columns [rotation][ldu] (a lane per gene: whole requests), the
// layout the rankers take.  Neither the padding of a last partial tile nor the tail of a column beyond U is written.
// The columns are ranked by the rank kernels (launch_colranks_dense_f64: average ranks, half-integers in doubles).
// mean and floormean: the sums of a set's ranks are the existing rank crossprod (exact integer sums); romer_count_kernel
// doubles them into the int64 sides and counts.  mean50: romer_mean50_kernel takes a wave per (set, rotation), holds the
// members' 2 r in LDS and selects the h-th largest bit by bit (19 bits: 2 r <= 2^18), as roast_mean50_kernel does on
// 64-bit keys.  The sides go out as [set][rotation][3] (Up, Down, Mixed) and/or are counted against the observed sides.
#include "common.h"
#include "romer.h"

#pragma clang fp contract(off)

namespace plaidhip {

constexpr int kRmTile = 64;   // rotations of a t tile (roast_rotate_kernel's)
constexpr int kRmPad = 65;    // doubles of an LDS row of the transpose

template <int kStat>
__global__ void __launch_bounds__(256)
romer_key_kernel(const double* __restrict__ Z, int32_t rows, const int32_t* __restrict__ uidx, int32_t U, int64_t ldu,
                 int32_t nk, double* __restrict__ Ka, double* __restrict__ Kb, double* __restrict__ Kc,
                 uint32_t* __restrict__ flag) {
  __shared__ double tile[kRmTile * kRmPad];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u0 = blockIdx.x * 64, tl = blockIdx.y;
  const int kin = tl * kRmTile;   // the tile's first rotation inside the chunk
  // gather: wave w takes genes u0 + 16 w .. + 15, a lane per rotation
  const bool krd = kin + lane < nk;
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int uu = wave * 16 + i, u = u0 + uu;
    double v = 0.0;
    if (u < U && krd) v = Z[((int64_t)tl * rows + uidx[u]) * kRmTile + lane];
    tile[lane * kRmPad + uu] = v;
  }
  __syncthreads();
  // write: wave w takes rotations 16 w .. + 15 of the tile, a lane per gene
  const int u = u0 + lane;
  bool bad = false;
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int r = wave * 16 + i, k = kin + r;
    if (u < U && k < nk) {
      double a, b, c;
      bool nan;
      romer_keys(tile[r * kRmPad + lane], kStat, &a, &b, &c, &nan);
      bad = bad || nan;
      const int64_t o = (int64_t)k * ldu + u;
      Ka[o] = a;
      if (kStat == PLAIDHIP_ROMER_STAT_FLOORMEAN) Kb[o] = b;
      Kc[o] = c;
    }
  }
  if (bad && flag != nullptr) *flag = 1u;
}

// keys of the nk rotations of one chunk (Z: the chunk's tiles; K*: the chunk's first column)
int launch_romer_keys(plaidhip_ctx* ctx, const double* Z, int32_t rows, const int32_t* d_uidx, int32_t U, int64_t ldu,
                      int set_statistic, int32_t nk, double* Ka, double* Kb, double* Kc, uint32_t* d_flag) {
  if (U == 0 || nk <= 0) return PLAIDHIP_OK;
  const dim3 grid((U + 63) / 64, (nk + kRmTile - 1) / kRmTile);
  if (set_statistic == PLAIDHIP_ROMER_STAT_FLOORMEAN)
    hipLaunchKernelGGL((romer_key_kernel<PLAIDHIP_ROMER_STAT_FLOORMEAN>), grid, dim3(256), 0, ctx->stream, Z, rows, d_uidx, U, ldu,
                       nk, Ka, Kb, Kc, d_flag);
  else
    hipLaunchKernelGGL((romer_key_kernel<PLAIDHIP_ROMER_STAT_MEAN>), grid, dim3(256), 0, ctx->stream, Z, rows, d_uidx, U, ldu, nk,
                       Ka, Kb, Kc, d_flag);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

__device__ inline int64_t romer_wave_sum(int64_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// what the lane that holds the three sides of (set s, rotation k) does with them: the sides to [set][rotation][3], the count
// against the observed sides into c3
__device__ inline void romer_emit(int32_t s, int32_t k, int32_t nrot, const int64_t* side, int64_t* __restrict__ stat,
                                  const int64_t* o3, int* c3) {
  if (stat != nullptr) {
    int64_t* o = stat + ((int64_t)s * nrot + k) * 3;
#pragma unroll
    for (int e = 0; e < 3; ++e) o[e] = side[e];
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) c3[e] += side[e] >= o3[e] ? 1 : 0;
}

// mean and floormean: the sums of the average ranks are the rank crossprod (launch_spmm_dense_f64 with PLAIDHIP_X_RANKS:
// exact, S [key][rotation][m] doubles, half-integers).  A thread per set doubles them into the int64 sides of every rotation
// of the chunk and counts; one thread owns a set's counts, so they are plain additions.
__global__ void __launch_bounds__(256)
romer_count_kernel(const double* __restrict__ Sa, const double* __restrict__ Sb, const double* __restrict__ Sc, int32_t m,
                   int32_t U, const int32_t* __restrict__ Gp, int set_statistic, int32_t nk, int32_t kbase, int32_t nrot,
                   int64_t* __restrict__ stat, const int64_t* __restrict__ obs, int32_t* __restrict__ cnt) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= m) return;
  const int ms = Gp[s + 1] - Gp[s];
  if (ms == 0) return;   // (no member: no statistic and no count)
  const int64_t flip = 2 * ((int64_t)U + 1);
  int64_t o3[3] = {0, 0, 0};
  if (obs != nullptr) {
#pragma unroll
    for (int e = 0; e < 3; ++e) o3[e] = obs[(int64_t)s * 3 + e];
  }
  int c3[3] = {0, 0, 0};
  for (int k = 0; k < nk; ++k) {
    const int64_t at = (int64_t)k * m + s;
    int64_t side[3];
    side[0] = (int64_t)(2.0 * Sa[at]);   // (a sum of half-integers below 2^52: exact)
    side[1] = set_statistic == PLAIDHIP_ROMER_STAT_FLOORMEAN ? (int64_t)(2.0 * Sb[at]) : (int64_t)ms * flip - side[0];
    side[2] = (int64_t)(2.0 * Sc[at]);
    romer_emit(s, kbase + k, nrot, side, stat, o3, c3);
  }
  if (cnt != nullptr) {
#pragma unroll
    for (int e = 0; e < 3; ++e) cnt[(int64_t)s * 3 + e] += c3[e];
  }
}

// mean50: the three sides of every (set of the list, rotation 0 .. nk - 1 of the chunk), a wave per (set, rotation), `cap`
// LDS entries a wave.  Ra, Rc: the average ranks [nk][ldu] (doubles), held as 2 r.  stat: [m][nrot][3] int64 at rotation
// kbase + k (or null); obs [m][3] int64 and cnt [m][3] int32 go together (or null).
__global__ void __launch_bounds__(256)
romer_mean50_kernel(const double* __restrict__ Ra, const double* __restrict__ Rc, int64_t ldu, int32_t U,
                    const int32_t* __restrict__ Gp, const int32_t* __restrict__ Gi, const int32_t* __restrict__ sel, int32_t cap,
                    int32_t nk, int32_t kbase, int32_t nrot, int64_t* __restrict__ stat, const int64_t* __restrict__ obs,
                    int32_t* __restrict__ cnt) {
  extern __shared__ uint32_t romer_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int s = sel[blockIdx.x];
  const int g0 = Gp[s], ms = Gp[s + 1] - g0;
  if (ms == 0 || ms > cap) return;   // (no member, or above the cap: no statistic and no count; the whole workgroup)
  const int64_t flip = 2 * ((int64_t)U + 1);
  const int h = ms / 2 + 1;
  uint32_t* keys = romer_lds + wave * cap;
  int64_t o3[3] = {0, 0, 0};
  if (obs != nullptr) {
#pragma unroll
    for (int e = 0; e < 3; ++e) o3[e] = obs[(int64_t)s * 3 + e];
  }
  int c3[3] = {0, 0, 0};
  const int stride = gridDim.y * nw;
  const int trips = (nk + stride - 1) / stride;   // (the same for every wave: the barriers below are met by all)
  for (int it = 0; it < trips; ++it) {
    const int k = it * stride + blockIdx.y * nw + wave;
    const bool valid = k < nk;
    int64_t side[3];
#pragma unroll 1
    for (int e = 0; e < 3; ++e) {
      __syncthreads();
      if (valid) {
        const double* r = (e == 2 ? Rc : Ra) + (int64_t)k * ldu;
        for (int i = lane; i < ms; i += 64) {
          const uint32_t v = (uint32_t)(2.0 * r[Gi[g0 + i]]);   // (a half-integer in [1, U]: exact)
          keys[i] = e == 1 ? (uint32_t)(flip - v) : v;
        }
      }
      __syncthreads();
      uint32_t prefix = 0;
      int rem = h;
      for (int bit = 18; bit >= 0; --bit) {
        const uint32_t cand = prefix | (1u << bit);
        int c = 0;
        for (int i0 = 0; i0 < ms; i0 += 64) {
          const int i = i0 + lane;
          const bool in = valid && i < ms;
          const uint32_t key = in ? keys[i] : 0u;
          c += __popcll(__ballot(in && (key >> bit) == (cand >> bit)));
        }
        if (c >= rem) prefix = cand;
        else rem -= c;
      }
      int64_t sum = 0;
      int above = 0;
      if (valid)
        for (int i = lane; i < ms; i += 64) {
          const uint32_t key = keys[i];
          if (key > prefix) {
            sum += key;
            ++above;
          }
        }
      sum = romer_wave_sum(sum);
      above = (int)romer_wave_sum((int64_t)above);
      side[e] = sum + (int64_t)(h - above) * prefix;   // the sum of the h largest keys
    }
    if (valid && lane == 0) romer_emit(s, kbase + k, nrot, side, stat, o3, c3);
  }
  if (cnt != nullptr && lane == 0) {
#pragma unroll
    for (int e = 0; e < 3; ++e)
      if (c3[e] != 0) atomicAdd(cnt + (int64_t)s * 3 + e, c3[e]);
  }
}

// The sides of rotations kbase .. kbase + nk - 1 from the chunk's average-rank matrices ([nk][ldu] doubles; Rb under
// floormean only).  mean and floormean: gs is the prepared collection of the pattern (d_Gp, d_Gi by place in the universe)
// and S takes the crossprods (2 or 3 x m x nk doubles).  mean50: the sets run in two size classes: d_sel (the set numbers,
// class 0 then class 1; the sets above the cap are in neither) and their counts class_cnt[2]; gs and S are not used.
int launch_romer_sides(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const double* Ra, const double* Rb, const double* Rc,
                       int64_t ldu, int32_t U, const int32_t* d_Gp, const int32_t* d_Gi, int32_t m, int set_statistic, int32_t nk,
                       int32_t kbase, int32_t nrot, const int32_t* d_sel, const int32_t* class_cnt, double* S, int64_t* d_stat,
                       const int64_t* d_obs, int32_t* d_cnt) {
  if (m == 0 || nk <= 0 || U == 0) return PLAIDHIP_OK;
  if (set_statistic != PLAIDHIP_ROMER_STAT_MEAN50) {
    const bool floor = set_statistic == PLAIDHIP_ROMER_STAT_FLOORMEAN;
    const size_t one = (size_t)m * nk;
    double *Sa = S, *Sc = S + one, *Sb = floor ? S + 2 * one : nullptr;
    const double* src[3] = {Ra, Rc, Rb};
    double* dst[3] = {Sa, Sc, Sb};
    for (int e = 0; e < (floor ? 3 : 2); ++e) {
      const int rc = launch_spmm_dense_f64(ctx, gs, src[e], ldu, nk, PLAIDHIP_STAT_SUM, 1.0, nullptr, 0.0, dst[e], m, nullptr,
                                           PLAIDHIP_X_RANKS);
      if (rc != PLAIDHIP_OK) return rc;
    }
    hipLaunchKernelGGL(romer_count_kernel, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, Sa, Sb, Sc, m, U, d_Gp, set_statistic,
                       nk, kbase, nrot, d_stat, d_obs, d_cnt);
  } else {
    int32_t off = 0;
    for (int cls = 0; cls < 2; ++cls) {
      const int32_t ns = class_cnt[cls];
      if (ns == 0) continue;
      const int32_t cap = romer_mean50_class_cap(cls);
      const int threads = cls == 0 ? 256 : 64, nw = threads / 64;
      const size_t lds = (size_t)cap * nw * 4;
      if (lds > 48 * 1024) PH_FULL_LDS(ctx, romer_mean50_kernel);
      const int gy = std::max(1, std::min(64, (nk + 8 * nw - 1) / (8 * nw)));
      hipLaunchKernelGGL(romer_mean50_kernel, dim3(ns, gy), dim3(threads), lds, ctx->stream, Ra, Rc, ldu, U, d_Gp, d_Gi,
                         d_sel + off, cap, nk, kbase, nrot, d_stat, d_obs, d_cnt);
      off += ns;
    }
  }
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
