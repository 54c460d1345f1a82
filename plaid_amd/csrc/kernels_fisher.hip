// plaid.fisher: over-representation (Fisher's exact / hypergeometric) tests of c gene lists against m sets
// (include/plaidhip.h: plaidhip_fisher).
//
// A list is a column of sig (g x c int8: -1 down, 0, +1 up).  Everything before the tail is integer counting:
//
// fisher_pack_kernel: the lists are taken kFsListTile at a time.  A thread owns one gene of one tile and packs the tile's
// signs of that gene into a 16-bit mask (bit t: up in list tile * T + t, bit 8 + t: down), so that a member row costs the
// count kernel ONE 2-byte load per tile whatever the number of lists.  The int8 loads run along the genes of one list
// (coalesced); a ballot per list and direction gives the wavefront's share of nUp / nDn, added with integer atomics (exact
// in any order).  A tile's masks are 2 g bytes (40 KB at 20,000 genes): they stay in L2 while the sets walk them.
//
// fisher_count_kernel: one wavefront per (set, tile of lists).  Lanes run along the set's members, so a single list (the
// commonest call) keeps all 64 lanes on members; a member row and its mask are read once per tile.  The counts never sit in
// lanes: per pass of 64 members, popcount(ballot(bit t of the mask)) is the pass's overlap with list t, a scalar, so there
// is no cross-lane reduction at the end and the 2 T counters live in scalar registers.  Four passes' loads are issued
// before the first ballot.
//
// fisher_tail_kernel: one thread per (set, list, direction) runs hyper_tail.h's pinned form and the odds ratio; lanes run
// along neighbouring sets of one list and direction, which gmt2mat orders by decreasing size (similar trip counts).
//
// fisher_overlap_kernel (only when the overlap lists are asked for): one wavefront per (set, list), members in order; a
// ballot of sig != 0 and the popcount of the lanes below give each hit its slot, so every slot has one writer; the rest of
// the set's segment is filled with -1.
//
// Benjamini-Hochberg runs on the host.  This file is compiled with fp contraction off (the pragma below and the Makefile).
#include <algorithm>

#include "common.h"
#include "hyper_tail.h"

#pragma clang fp contract(off)

namespace plaidhip {

namespace {

constexpr int kFsListTile = PLAIDHIP_FISHER_LIST_TILE;   // lists per mask (8 up bits, 8 down bits)
constexpr int kFsWaves = 4;                              // wavefronts per workgroup of the wavefront-per-item kernels
constexpr int kFsUnroll = 4;                             // passes of 64 members whose loads are in flight together
static_assert(kFsListTile == 8, "a mask is 16 bits: 8 lists up, 8 lists down");

// masks: [ntile][g]; tot: [c][2] = {nUp, nDn}, zero on entry.  grid.x covers the genes, grid.y strides the tiles.
__global__ void __launch_bounds__(256)
fisher_pack_kernel(const int8_t* __restrict__ sig, int32_t g, int32_t c, uint16_t* __restrict__ masks, int32_t* __restrict__ tot) {
  const int32_t ntile = (c + kFsListTile - 1) / kFsListTile;
  const int lane = threadIdx.x & 63;
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < g;   // (every lane stays for the ballots)
  for (int32_t tile = blockIdx.y; tile < ntile; tile += gridDim.y) {
    const int32_t l0 = tile * kFsListTile;
    const int nt = c - l0 < kFsListTile ? c - l0 : kFsListTile;
    uint32_t mk = 0;
    for (int t = 0; t < nt; ++t) {
      const int s = in ? (int)sig[(int64_t)(l0 + t) * g + i] : 0;
      const unsigned long long bu = __ballot(s > 0), bd = __ballot(s < 0);
      mk |= (s > 0 ? 1u : 0u) << t;
      mk |= (s < 0 ? 1u : 0u) << (8 + t);
      if (lane == 0) {
        if (bu != 0ull) atomicAdd(&tot[2 * (l0 + t)], __popcll(bu));
        if (bd != 0ull) atomicAdd(&tot[2 * (l0 + t) + 1], __popcll(bd));
      }
    }
    if (in) masks[(int64_t)tile * g + i] = (uint16_t)mk;
  }
}

// ov: [c][2][m] = ovUp, ovDn of every (list, set)
__global__ void __launch_bounds__(64 * kFsWaves)
fisher_count_kernel(const uint16_t* __restrict__ masks, int32_t g, int32_t c, const int32_t* __restrict__ Gp,
                    const int32_t* __restrict__ Gi, int32_t m, int32_t* __restrict__ ov) {
  constexpr int T = kFsListTile;
  const int lane = threadIdx.x & 63;
  const int32_t ntile = (c + T - 1) / T;
  const int64_t items = (int64_t)m * ntile, nwave = (int64_t)gridDim.x * kFsWaves;
  for (int64_t item = (int64_t)blockIdx.x * kFsWaves + (threadIdx.x >> 6); item < items; item += nwave) {
    const int32_t j = (int32_t)(item % m), tile = (int32_t)(item / m);
    const int32_t l0 = tile * T;
    const int nt = c - l0 < T ? c - l0 : T;
    const uint16_t* __restrict__ mk_of = masks + (int64_t)tile * g;
    const int32_t b = Gp[j], e = Gp[j + 1];
    int32_t up[T], dn[T];
#pragma unroll
    for (int t = 0; t < T; ++t) up[t] = dn[t] = 0;
    for (int32_t q0 = b; q0 < e; q0 += 64 * kFsUnroll) {
      int32_t r[kFsUnroll];
      uint32_t mk[kFsUnroll];
#pragma unroll
      for (int u = 0; u < kFsUnroll; ++u) {
        const int32_t q = q0 + u * 64 + lane;
        r[u] = q < e ? Gi[q] : -1;
      }
#pragma unroll
      for (int u = 0; u < kFsUnroll; ++u) mk[u] = r[u] >= 0 ? (uint32_t)mk_of[r[u]] : 0u;
#pragma unroll
      for (int u = 0; u < kFsUnroll; ++u) {
        if (q0 + u * 64 >= e) break;   // (wave-uniform)
#pragma unroll
        for (int t = 0; t < T; ++t) {
          if (t >= nt) break;          // (wave-uniform: one list costs two ballots a pass)
          up[t] += __popcll(__ballot((mk[u] >> t) & 1u));
          dn[t] += __popcll(__ballot((mk[u] >> (8 + t)) & 1u));
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if (t >= nt) break;
        ov[((int64_t)(l0 + t) * 2) * m + j] = up[t];
        ov[((int64_t)(l0 + t) * 2 + 1) * m + j] = dn[t];
      }
    }
  }
}

// out: [c][12][m] (the columns of include/plaidhip.h; the three padj columns are NaN here, the host fills them)
__global__ void __launch_bounds__(256)
fisher_tail_kernel(const int32_t* __restrict__ tot, const int32_t* __restrict__ ov, const int32_t* __restrict__ Gp, int32_t g,
                   int32_t c, int32_t m, double* __restrict__ out) {
  const double kNaN = __builtin_nan("");
  const int64_t items = (int64_t)m * c * 3;
  for (int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x; item < items; item += (int64_t)gridDim.x * 256) {
    const int32_t j = (int32_t)(item % m);
    const int64_t ld = item / m;
    const int32_t l = (int32_t)(ld % c);
    const int d = (int)(ld / c);   // 0 up, 1 down, 2 any
    const int64_t N = g, k = Gp[j + 1] - Gp[j];
    const int64_t nU = tot[2 * l], nD = tot[2 * l + 1];
    const int64_t oU = ov[((int64_t)l * 2) * m + j], oD = ov[((int64_t)l * 2 + 1) * m + j];
    const int64_t K = d == 0 ? nU : (d == 1 ? nD : nU + nD);
    const int64_t x = d == 0 ? oU : (d == 1 ? oD : oU + oD);
    double* __restrict__ o = out + (int64_t)l * 12 * m + j;
    if (d == 0) {
      o[0] = (double)k;
      o[(int64_t)m] = (double)oU;
      o[2 * (int64_t)m] = (double)oD;
    }
    const bool none = k == 0 || k == N;
    o[(int64_t)(3 + d) * m] = none ? kNaN : hyper_tail(N, K, k, x);
    o[(int64_t)(6 + d) * m] = kNaN;
    o[(int64_t)(9 + d) * m] = none ? kNaN : fisher_odds(N, K, k, x);
  }
}

// len: [c][m]; idx: [c][nnz], nnz = Gp[m]
__global__ void __launch_bounds__(64 * kFsWaves)
fisher_overlap_kernel(const int8_t* __restrict__ sig, int32_t g, int32_t c, const int32_t* __restrict__ Gp,
                      const int32_t* __restrict__ Gi, int32_t m, int32_t* __restrict__ len, int32_t* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int64_t nnz = Gp[m];
  const int64_t items = (int64_t)m * c, nwave = (int64_t)gridDim.x * kFsWaves;
  for (int64_t item = (int64_t)blockIdx.x * kFsWaves + (threadIdx.x >> 6); item < items; item += nwave) {
    const int32_t j = (int32_t)(item % m), l = (int32_t)(item / m);
    const int8_t* __restrict__ s = sig + (int64_t)l * g;
    int32_t* __restrict__ seg = idx + (int64_t)l * nnz;
    const int32_t b = Gp[j], e = Gp[j + 1];
    int32_t base = 0;
    for (int32_t q0 = b; q0 < e; q0 += 64) {
      const int32_t q = q0 + lane;
      const int32_t r = q < e ? Gi[q] : 0;
      const bool hit = q < e && s[r] != 0;
      const unsigned long long bal = __ballot(hit);
      if (hit) seg[b + base + __popcll(bal & ((1ull << lane) - 1ull))] = r;
      base += __popcll(bal);
    }
    for (int32_t q = b + base + lane; q < e; q += 64) seg[q] = -1;
    if (lane == 0) len[(int64_t)l * m + j] = base;
  }
}

inline unsigned grid_for(int64_t items, int64_t per_block) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, 1 << 20));
}

}  // namespace

int launch_fisher_pack(plaidhip_ctx* ctx, const int8_t* sig, int32_t g, int32_t c, uint16_t* masks, int32_t* tot) {
  if (g <= 0 || c <= 0) return PLAIDHIP_OK;
  const int32_t ntile = (c + kFsListTile - 1) / kFsListTile;
  PH_HIP(hipMemsetAsync(tot, 0, (size_t)c * 2 * 4, ctx->stream));
  hipLaunchKernelGGL(fisher_pack_kernel, dim3((unsigned)((g + 255) / 256), (unsigned)std::min(ntile, 4096)), dim3(256), 0,
                     ctx->stream, sig, g, c, masks, tot);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_fisher_count(plaidhip_ctx* ctx, const uint16_t* masks, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi,
                        int32_t m, int32_t* ov) {
  if (m <= 0 || c <= 0) return PLAIDHIP_OK;
  const int64_t items = (int64_t)m * ((c + kFsListTile - 1) / kFsListTile);
  hipLaunchKernelGGL(fisher_count_kernel, dim3(grid_for(items, kFsWaves)), dim3(64 * kFsWaves), 0, ctx->stream, masks, g, c, Gp,
                     Gi, m, ov);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_fisher_tail(plaidhip_ctx* ctx, const int32_t* tot, const int32_t* ov, const int32_t* Gp, int32_t g, int32_t c,
                       int32_t m, double* out) {
  if (m <= 0 || c <= 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(fisher_tail_kernel, dim3(grid_for((int64_t)m * c * 3, 256)), dim3(256), 0, ctx->stream, tot, ov, Gp, g, c, m,
                     out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_fisher_overlap(plaidhip_ctx* ctx, const int8_t* sig, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi,
                          int32_t m, int32_t* len, int32_t* idx) {
  if (m <= 0 || c <= 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(fisher_overlap_kernel, dim3(grid_for((int64_t)m * c, kFsWaves)), dim3(64 * kFsWaves), 0, ctx->stream, sig, g,
                     c, Gp, Gi, m, len, idx);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip

extern "C" {

// the pinned tail itself, on the host: no device is touched
int plaidhip_hyper_tail(int64_t N, int64_t K, int64_t k, int64_t x, double* p) try {
  if (N > PLAIDHIP_FISHER_MAX_GENES) {
    plaidhip::set_error("hyper_tail: N = %lld (at most %d)", (long long)N, PLAIDHIP_FISHER_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(N >= 0 && K >= 0 && K <= N && k >= 0 && k <= N, "hyper_tail: N = %lld, K = %lld, k = %lld (0 <= K, k <= N)",
             (long long)N, (long long)K, (long long)k);
  PH_REQUIRE(p != nullptr, "hyper_tail: null p");
  *p = plaidhip::hyper_tail(N, K, k, x);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

}
