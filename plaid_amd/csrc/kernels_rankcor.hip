// plaid.rankcor: the correlation of c lists of gene statistics, or of their ranks, with the membership column of m sets
// (include/plaidhip.h: plaidhip_rankcor).  A list is a column of stat (g x c doubles); a NaN row takes
// no part in that list, so the ranks, the universe n and every set's effective size k differ from list to list.
//
// rankcor_center_kernel (value mode only): one workgroup of 256 per list.  Pass one sums the rows that are not NaN (thread
// h takes rows h, h + 256, ...; the partials are folded in LDS, [h] += [h + s], s = 128 .. 1), counts them and looks for an
// infinity and for max == min; pass two writes d = x - mu over the column (NaN kept) and sums d and d * d the same way.
// The order depends on nothing but these 256 threads.
//
// rankcor_pack_kernel<ACC>: the lists are taken kRcListTile at a time.  A thread owns one gene of one tile and writes the
// tile's eight values of that gene side by side -- [tile][gene][8] -- so that a member row costs the gather kernel ONE
// 32-byte load (uint32 z = 2 rank, 0 outside V) or one 64-byte load and a mask byte (doubles, 0.0 outside V) whatever the
// number of lists.  The loads run along the genes of one list (coalesced).  In rank mode n, T1 = sum z and T2 = sum z^2 of
// every list are reduced over the wavefront and added with 64-bit integer atomics: exact in any order.
//
// rankcor_gather_kernel<ACC>: one wavefront per (set, tile of lists), lanes along the set's members, as fisher_count_kernel.
// k of a list is the popcount of a ballot per pass of 64 members (a scalar).  A accumulates per lane: uint32 in rank mode (a
// lane meets at most 2,048 members of z <= 2^18) and is widened to 64 bits for the butterfly; doubles in value mode, member
// positions ascending per lane and the butterfly s = 32 .. 1, the order include/plaidhip.h pins.
//
// The epilogues and Benjamini-Hochberg run on the host (stats.cpp).  Compiled with fp contraction off.
#include <algorithm>

#include "common.h"

#pragma clang fp contract(off)

namespace plaidhip {

namespace {

constexpr int kRcListTile = PLAIDHIP_RANKCOR_LIST_TILE;
constexpr int kRcWaves = 4;    // wavefronts per workgroup of the gather kernel
constexpr int kRcUnroll = 2;   // passes of 64 members whose loads are in flight together
static_assert(kRcListTile == 8, "a tile row is 8 values: two 16-byte words of z, one mask byte");

// partial[h] += partial[h + s], s = 128 .. 1 (256 threads); the sum is partial[0] for every thread afterwards
template <typename T>
__device__ __forceinline__ T fold256(T v, T* sh, int tid) {
  __syncthreads();   // (the previous fold's readers are done)
  sh[tid] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) sh[tid] = sh[tid] + sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

// D: g x c (leading dimension g) <- stat - mu, NaN kept; vs: [c][4] = {n, T1, T2, flag (1: an infinity, 2: max == min)}
__global__ void __launch_bounds__(256)
rankcor_center_kernel(const double* __restrict__ X, int32_t g, int32_t c, double* __restrict__ D, double* __restrict__ vs) {
  __shared__ double sh_d[256];
  __shared__ int sh_i[256];
  const int tid = threadIdx.x;
  for (int32_t l = blockIdx.x; l < c; l += gridDim.x) {
    const double* __restrict__ x = X + (int64_t)l * g;
    double* __restrict__ d = D + (int64_t)l * g;
    double s = 0.0, mn = INFINITY, mx = -INFINITY;
    int cnt = 0, inf = 0;
    for (int32_t i = tid; i < g; i += 256) {
      const double v = x[i];
      if (v == v) {
        s = s + v;
        ++cnt;
        inf |= (v == INFINITY || v == -INFINITY) ? 1 : 0;
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
      }
    }
    const double sum = fold256(s, sh_d, tid);
    const int n = fold256(cnt, sh_i, tid);
    const int anyinf = fold256(inf, sh_i, tid);
    // min / max: the same fold with another operation
    __syncthreads();
    sh_d[tid] = mn;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
      if (tid < st) sh_d[tid] = sh_d[tid + st] < sh_d[tid] ? sh_d[tid + st] : sh_d[tid];
      __syncthreads();
    }
    const double gmn = sh_d[0];
    __syncthreads();
    sh_d[tid] = mx;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
      if (tid < st) sh_d[tid] = sh_d[tid + st] > sh_d[tid] ? sh_d[tid + st] : sh_d[tid];
      __syncthreads();
    }
    const double gmx = sh_d[0];
    const int flag = anyinf != 0 ? 1 : ((n > 0 && gmx == gmn) ? 2 : 0);
    const double mu = sum / (double)n;
    double t1 = 0.0, t2 = 0.0;
    for (int32_t i = tid; i < g; i += 256) {
      const double v = x[i];
      double dv = v - mu;                           // (a NaN stays a NaN)
      if (flag == 1) dv = (v == v) ? 0.0 : v;       // a list with an infinity is NaN by rule: keep its V for the sizes
      d[i] = dv;
      if (v == v) {
        t1 = t1 + dv;
        t2 = t2 + dv * dv;
      }
    }
    const double T1 = fold256(t1, sh_d, tid);
    const double T2 = fold256(t2, sh_d, tid);
    if (tid == 0) {
      vs[4 * (int64_t)l] = (double)n;
      vs[4 * (int64_t)l + 1] = T1;
      vs[4 * (int64_t)l + 2] = T2;
      vs[4 * (int64_t)l + 3] = (double)flag;
    }
    __syncthreads();
  }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// R: g x c doubles (leading dimension g): the ranks (ACC = uint32_t) or the centred values (ACC = double), NaN outside V.
// tiles: [ntile][g][8] ACC; vmask (doubles only): [ntile][g] bytes, bit t: in V of list tile * 8 + t; sums (ranks only):
// [c][3] u64 = {n, T1, T2}, zero on entry.  grid.x covers the genes, grid.y strides the tiles.
template <typename ACC>
__global__ void __launch_bounds__(256)
rankcor_pack_kernel(const double* __restrict__ R, int32_t g, int32_t c, ACC* __restrict__ tiles, uint8_t* __restrict__ vmask,
                    unsigned long long* __restrict__ sums) {
  constexpr int T = kRcListTile;
  const int32_t ntile = (c + T - 1) / T;
  const int lane = threadIdx.x & 63;
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < g;   // (every lane stays for the reductions)
  for (int32_t tile = blockIdx.y; tile < ntile; tile += gridDim.y) {
    const int32_t l0 = tile * T;
    const int nt = c - l0 < T ? c - l0 : T;
    ACC val[T];
    uint32_t mk = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      val[t] = (ACC)0;
      if (t >= nt) continue;   // (wave-uniform)
      const double r = in ? R[(int64_t)(l0 + t) * g + i] : __builtin_nan("");
      const bool ok = r == r;
      mk |= (ok ? 1u : 0u) << t;
      if constexpr (sizeof(ACC) == 4) {
        const uint32_t z = ok ? (uint32_t)(2.0 * r) : 0u;   // (a rank is a half-integer <= g: 2 r is an exact integer)
        val[t] = z;
        const unsigned long long nv = (unsigned long long)__popcll(__ballot(ok));
        const unsigned long long s1 = wave_sum_u64((unsigned long long)z);
        const unsigned long long s2 = wave_sum_u64((unsigned long long)z * (unsigned long long)z);
        if (lane == 0 && nv != 0ull) {
          atomicAdd(&sums[3 * (int64_t)(l0 + t)], nv);
          atomicAdd(&sums[3 * (int64_t)(l0 + t) + 1], s1);
          atomicAdd(&sums[3 * (int64_t)(l0 + t) + 2], s2);
        }
      } else {
        val[t] = ok ? (ACC)r : (ACC)0;
      }
    }
    if (in) {
      ACC* __restrict__ o = tiles + ((int64_t)tile * g + i) * T;
#pragma unroll
      for (int t = 0; t < T; ++t) o[t] = val[t];
      if constexpr (sizeof(ACC) == 8) vmask[(int64_t)tile * g + i] = (uint8_t)mk;
    }
  }
}

template <typename ACC> struct RcWide;
template <> struct RcWide<uint32_t> { using type = long long; };
template <> struct RcWide<double> { using type = double; };

// kout: [c][m] int32; Aout: [c][m] int64 (ranks) or double (values)
template <typename ACC>
__global__ void __launch_bounds__(64 * kRcWaves)
rankcor_gather_kernel(const ACC* __restrict__ tiles, const uint8_t* __restrict__ vmask, int32_t g, int32_t c,
                      const int32_t* __restrict__ Gp, const int32_t* __restrict__ Gi, int32_t m, int32_t* __restrict__ kout,
                      typename RcWide<ACC>::type* __restrict__ Aout) {
  constexpr int T = kRcListTile;
  constexpr bool kInt = sizeof(ACC) == 4;
  const int lane = threadIdx.x & 63;
  const int32_t ntile = (c + T - 1) / T;
  const int64_t items = (int64_t)m * ntile, nwave = (int64_t)gridDim.x * kRcWaves;
  for (int64_t item = (int64_t)blockIdx.x * kRcWaves + (threadIdx.x >> 6); item < items; item += nwave) {
    const int32_t j = (int32_t)(item % m), tile = (int32_t)(item / m);
    const int32_t l0 = tile * T;
    const int nt = c - l0 < T ? c - l0 : T;
    const ACC* __restrict__ tl = tiles + (int64_t)tile * g * T;
    const uint8_t* __restrict__ mk_of = kInt ? nullptr : vmask + (int64_t)tile * g;
    const int32_t b = Gp[j], e = Gp[j + 1];
    ACC acc[T];
    int32_t kk[T];
#pragma unroll
    for (int t = 0; t < T; ++t) { acc[t] = (ACC)0; kk[t] = 0; }
    for (int32_t q0 = b; q0 < e; q0 += 64 * kRcUnroll) {
      int32_t r[kRcUnroll];
      ACC v[kRcUnroll][T];
      uint32_t mk[kRcUnroll];
#pragma unroll
      for (int u = 0; u < kRcUnroll; ++u) {
        const int32_t q = q0 + u * 64 + lane;
        r[u] = q < e ? Gi[q] : -1;
      }
#pragma unroll
      for (int u = 0; u < kRcUnroll; ++u) {
        mk[u] = 0;
        if (r[u] >= 0) {
          const ACC* __restrict__ row = tl + (int64_t)r[u] * T;
          if constexpr (kInt) {
            const uint4 a = *reinterpret_cast<const uint4*>(row), bb = *reinterpret_cast<const uint4*>(row + 4);
            v[u][0] = a.x; v[u][1] = a.y; v[u][2] = a.z; v[u][3] = a.w;
            v[u][4] = bb.x; v[u][5] = bb.y; v[u][6] = bb.z; v[u][7] = bb.w;
          } else {
#pragma unroll
            for (int h = 0; h < T; h += 2) {
              const double2 a = *reinterpret_cast<const double2*>(row + h);
              v[u][h] = a.x;
              v[u][h + 1] = a.y;
            }
            mk[u] = (uint32_t)mk_of[r[u]];
          }
        } else {
#pragma unroll
          for (int t = 0; t < T; ++t) v[u][t] = (ACC)0;
        }
      }
#pragma unroll
      for (int u = 0; u < kRcUnroll; ++u) {
        if (q0 + u * 64 >= e) break;   // (wave-uniform)
#pragma unroll
        for (int t = 0; t < T; ++t) {
          if (t >= nt) break;          // (wave-uniform)
          acc[t] = acc[t] + v[u][t];   // (a row outside V holds 0: the sum is that of the members in V, in position order)
          const bool ok = kInt ? v[u][t] != (ACC)0 : ((mk[u] >> t) & 1u) != 0u;
          kk[t] += __popcll(__ballot(ok));
        }
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if (t >= nt) break;
      typename RcWide<ACC>::type s = (typename RcWide<ACC>::type)acc[t];
#pragma unroll
      for (int st = 32; st >= 1; st >>= 1) s = s + __shfl_xor(s, st);
      if (lane == 0) {
        kout[(int64_t)(l0 + t) * m + j] = kk[t];
        Aout[(int64_t)(l0 + t) * m + j] = s;
      }
    }
  }
}

#ifdef PLAIDHIP_RANKCOR_LANES8
// The other mapping, for the A/B builds of tools/ only (make variant NAME=rclanes8 DEFS=-DPLAIDHIP_RANKCOR_LANES8; rank mode):
// 8 lanes per member, one list each -- lane = 8 * slot + t reads the 4 bytes of list t of the member in slot `slot`, so a
// wavefront takes 8 members a pass and a single list keeps 8 of its 64 lanes busy.  Measured: at
// c = 1, the commonest call, 12.0 against 8.6 us at 5,000 sets and 196 against 82 us at 61,459; at c = 64 it is the faster
// one, 38 against 50 us -- of a host call of 8 ms.  The product holds the one mapping that wins at c = 1.
__global__ void __launch_bounds__(64 * kRcWaves)
rankcor_gather_lanes8_kernel(const uint32_t* __restrict__ tiles, int32_t g, int32_t c, const int32_t* __restrict__ Gp,
                             const int32_t* __restrict__ Gi, int32_t m, int32_t* __restrict__ kout, long long* __restrict__ Aout) {
  constexpr int T = kRcListTile, U = 8;
  const int lane = threadIdx.x & 63, t = lane & 7, slot = lane >> 3;
  const int32_t ntile = (c + T - 1) / T;
  const int64_t items = (int64_t)m * ntile, nwave = (int64_t)gridDim.x * kRcWaves;
  for (int64_t item = (int64_t)blockIdx.x * kRcWaves + (threadIdx.x >> 6); item < items; item += nwave) {
    const int32_t j = (int32_t)(item % m), tile = (int32_t)(item / m);
    const int32_t l0 = tile * T;
    const int nt = c - l0 < T ? c - l0 : T;
    const uint32_t* __restrict__ tl = tiles + (int64_t)tile * g * T;
    const int32_t b = Gp[j], e = Gp[j + 1];
    uint32_t acc = 0;
    int32_t kk = 0;
    for (int32_t q0 = b; q0 < e; q0 += 8 * U) {
      int32_t r[U];
      uint32_t z[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t q = q0 + u * 8 + slot;
        r[u] = (q < e && t < nt) ? Gi[q] : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) z[u] = r[u] >= 0 ? tl[(int64_t)r[u] * T + t] : 0u;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc += z[u];
        kk += __popcll(__ballot(z[u] != 0u) & (0x0101010101010101ull << t));
      }
    }
    long long s = (long long)acc;
#pragma unroll
    for (int st = 32; st >= 8; st >>= 1) s = s + __shfl_xor(s, st);
    if (slot == 0 && t < nt) {
      kout[(int64_t)(l0 + t) * m + j] = kk;
      Aout[(int64_t)(l0 + t) * m + j] = s;
    }
  }
}
#endif

inline unsigned grid_for(int64_t items, int64_t per_block) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, 1 << 20));
}

}  // namespace

int launch_rankcor_center(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t c, double* D, double* vs) {
  if (c <= 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(rankcor_center_kernel, dim3((unsigned)std::min(c, 65535)), dim3(256), 0, ctx->stream, X, g, c, D, vs);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_rankcor_pack(plaidhip_ctx* ctx, int use_rank, const double* R, int32_t g, int32_t c, void* tiles, uint8_t* vmask,
                        unsigned long long* sums) {
  if (g <= 0 || c <= 0) return PLAIDHIP_OK;
  const int32_t ntile = (c + kRcListTile - 1) / kRcListTile;
  const dim3 grid((unsigned)((g + 255) / 256), (unsigned)std::min(ntile, 4096));
  if (use_rank) {
    PH_HIP(hipMemsetAsync(sums, 0, (size_t)c * 3 * 8, ctx->stream));
    hipLaunchKernelGGL(rankcor_pack_kernel<uint32_t>, grid, dim3(256), 0, ctx->stream, R, g, c, static_cast<uint32_t*>(tiles),
                       static_cast<uint8_t*>(nullptr), sums);
  } else {
    hipLaunchKernelGGL(rankcor_pack_kernel<double>, grid, dim3(256), 0, ctx->stream, R, g, c, static_cast<double*>(tiles), vmask,
                       static_cast<unsigned long long*>(nullptr));
  }
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_rankcor_gather(plaidhip_ctx* ctx, int use_rank, const void* tiles, const uint8_t* vmask, int32_t g, int32_t c,
                          const int32_t* Gp, const int32_t* Gi, int32_t m, int32_t* kout, void* Aout) {
  if (m <= 0 || c <= 0) return PLAIDHIP_OK;
  const int64_t items = (int64_t)m * ((c + kRcListTile - 1) / kRcListTile);
  const dim3 grid(grid_for(items, kRcWaves)), block(64 * kRcWaves);
  if (use_rank)
#ifdef PLAIDHIP_RANKCOR_LANES8
    hipLaunchKernelGGL(rankcor_gather_lanes8_kernel, grid, block, 0, ctx->stream, static_cast<const uint32_t*>(tiles), g, c, Gp, Gi,
                       m, kout, static_cast<long long*>(Aout));
#else
    hipLaunchKernelGGL(rankcor_gather_kernel<uint32_t>, grid, block, 0, ctx->stream, static_cast<const uint32_t*>(tiles),
                       static_cast<const uint8_t*>(nullptr), g, c, Gp, Gi, m, kout, static_cast<long long*>(Aout));
#endif
  else
    hipLaunchKernelGGL(rankcor_gather_kernel<double>, grid, block, 0, ctx->stream, static_cast<const double*>(tiles), vmask, g, c,
                       Gp, Gi, m, kout, static_cast<double*>(Aout));
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
