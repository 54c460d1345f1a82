// Column medians: the middle phase of normalize_medians() (R/plaid.R:554-575).  gfx950 / wave64 only.
//
//   col_medians : per-sample median over gene sets; exact zeros masked when ignore_zero
//                 (R/plaid.R:562-565), all-masked column -> 0 (R/plaid.R:566).  Even count:
//                 mean of the two middle order statistics (matrixStats::colMedians).
//
// Every kernel here selects the two middle order statistics exactly, by radix selection on order-preserving 64-bit keys,
// with one wavefront per column and no workgroup barrier:
//   col_medians_wave_kernel   : m <= 6,144, the column in the wavefront's registers
//   col_medians_stream_kernel : larger m, the column swept from memory
//   colmean_predict / median_calibrate / median_select : the medians whose candidates the crossprod launch set aside
//                 while it wrote the scores (kernels_spmm.hip: MED); what they leave goes to the streaming kernel
// launch_col_medians picks between the first two from m alone.  The whole-matrix passes before and after (minflags, sum,
// shift) are in kernels_norm.hip; DESIGN.md 4.3 has the measurements, the superseded kernels among them.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"

#include <type_traits>
#include "device_sort.h"

// A/B knob for `make variant DEFS=...` (tools/ab_norm.sh); the product carries no run-time switch.
//   PLAIDHIP_MED_PAIR_LOADS: col_medians_wave_kernel reads the rows that every column of its class has with 16-byte loads
//     where the column is aligned.
#ifndef PLAIDHIP_MED_PAIR_LOADS
#define PLAIDHIP_MED_PAIR_LOADS 1
#endif

namespace plaidhip {

// ignore.zero resolved on the device: explicit 0/1, or (-1) min(x)==0 from the flag words
__device__ __forceinline__ int resolve_ignore_zero(int ignore_zero, const uint32_t* flags) {
  if (ignore_zero >= 0) return ignore_zero;
  return (flags[1] != 0u && flags[0] == 0u) ? 1 : 0;
}

// order-preserving key of v, or the all-ones key when v is masked (NaN: na.rm = TRUE; exact zero
// when ignore_zero).  Branch-free on purpose: with control flow hipcc waits for every load
// before issuing the next one and the column sweeps serialise on L2 latency.
__device__ __forceinline__ uint64_t masked_key(double v, int ignore_zero) {
  const uint64_t u = (uint64_t)__double_as_longlong(v + 0.0);          // -0 -> +0
  const uint64_t key = u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
  const bool masked = (v != v) | ((ignore_zero != 0) & (v == 0.0));
  return masked ? ~0ull : key;
}

// what stands where a workgroup kernel has a barrier: every wavefront here owns its histogram and its list in LDS
__device__ __forceinline__ void wave_lds_sync() {
  // LDS operations of one wavefront are executed in order; only the compiler must not reorder
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef double f64x2_t __attribute__((ext_vector_type(2)));

// Wave-level scan and reductions on the DPP network (row_shr 1 / 2 / 4 / 8 inside the 16-lane rows, then row_bcast 15 and
// 31 across them: the gfx9 sequence) instead of __shfl_up / __shfl_xor, which hipcc lowers to ds_bpermute_b32 -- a round
// trip through the LDS crossbar per step, six to twelve of them in a dependent chain per scan or 64-bit reduction, in
// kernels whose wavefronts have nothing else to issue meanwhile.
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t old, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, BANK_MASK, false);
}
#define PH_DPP_STEPS(STEP) STEP(0x111, 0xf, 0xf) STEP(0x112, 0xf, 0xf) STEP(0x114, 0xf, 0xe) STEP(0x118, 0xf, 0xc) \
                           STEP(0x142, 0xa, 0xf) STEP(0x143, 0xc, 0xf)
// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ uint32_t wave_scan_add_u32(uint32_t v) {
#define PH_STEP(C, R, B) v += dpp_u32<C, R, B>(0u, v);
  PH_DPP_STEPS(PH_STEP)
#undef PH_STEP
  return v;
}
// reductions: the result of all 64 lanes, wave-uniform (read from lane 63)
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#define PH_STEP(C, R, B) { const uint32_t t = dpp_u32<C, R, B>(0xffffffffu, v); v = t < v ? t : v; }
  PH_DPP_STEPS(PH_STEP)
#undef PH_STEP
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#define PH_STEP(C, R, B) { const uint32_t t = dpp_u32<C, R, B>(0u, v); v = t > v ? t : v; }
  PH_DPP_STEPS(PH_STEP)
#undef PH_STEP
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#define PH_STEP(C, R, B)                                                                                  \
  {                                                                                                        \
    const uint64_t t = ((uint64_t)dpp_u32<C, R, B>(0xffffffffu, (uint32_t)(v >> 32)) << 32) |             \
                       dpp_u32<C, R, B>(0xffffffffu, (uint32_t)v);                                         \
    v = t < v ? t : v;                                                                                     \
  }
  PH_DPP_STEPS(PH_STEP)
#undef PH_STEP
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#define PH_STEP(C, R, B)                                                                                  \
  {                                                                                                        \
    const uint64_t t = ((uint64_t)dpp_u32<C, R, B>(0u, (uint32_t)(v >> 32)) << 32) | dpp_u32<C, R, B>(0u, (uint32_t)v); \
    v = t > v ? t : v;                                                                                     \
  }
  PH_DPP_STEPS(PH_STEP)
#undef PH_STEP
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}
#undef PH_DPP_STEPS

// m <= 64 * ITEMS: radix selection, 8 bits per pass, with ONE WAVEFRONT per column and the keys in its registers (up to
// 96 per lane).  The column is read once; keys are binned on (key - lo) >> shift over the current range [lo, lo + range]
// (first the range of the column's keys, then the bin that holds the wanted rank) into 256 bins, and the search stops as
// soon as the bin holds a single key or is one key wide: doubles of similar magnitude need two to three passes.  There is
// no workgroup barrier anywhere -- a pass is ITEMS LDS atomics per lane into the wavefront's own 256-bin histogram, a scan
// of the bins by the same wavefront, and wave-uniform results come back through readlane instead of LDS.  Two wavefronts
// per SIMD (eight columns in flight per CU, 40 KB each at C2) keep the memory system busy while the others select.  For an
// even count the upper middle value is another copy of the selected key (ties) or the smallest key above it (one more
// sweep of the registers).
// The kernel is bound by its vector instructions (~35 per key), so the common steps work on the HIGH dword of the keys:
// the first range is [min high dword << 32, max high dword << 32 | ~0] -- wider than [min, max] but covering it -- and
// while a pass shifts by >= 32 bits (the first one or two do) bin and range test are 32-bit operations; the exact 64-bit
// form takes over below that.
template <int ITEMS, int WG_PER_CU>
__global__ void __launch_bounds__(256, WG_PER_CU)
col_medians_wave_kernel(const double* __restrict__ S, int64_t lds, int32_t m, int32_t n,
                        int ignore_zero_mode, const uint32_t* __restrict__ flags, double* __restrict__ med,
                        unsigned long long* __restrict__ dbg) {
#ifdef PLAIDHIP_DIAG
#define PH_MSTAMP(k) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st[k] += t_ - tl; tl = t_; }
  unsigned long long st[5] = {0, 0, 0, 0, 0}, tl = __builtin_amdgcn_s_memtime(), npass = 0;
#else
#define PH_MSTAMP(k)
#endif
  // per wavefront 256 bins + 64 private trash bins (one per lane) that keys outside the current range count into: the
  // atomic is unconditional, so no per-key lane mask has to live in scalar registers across the unrolled loop
  __shared__ __align__(16) uint32_t s_hist[4][320];
  const int ignore_zero = resolve_ignore_zero(ignore_zero_mode, flags);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* hist = s_hist[wave];
  *reinterpret_cast<uint4*>(&hist[lane * 4]) = make_uint4(0u, 0u, 0u, 0u);
  hist[256 + lane] = 0u;
  wave_lds_sync();
  const uint32_t trash = 256u + (uint32_t)lane;
  const int nwaves = gridDim.x * 4;
  for (int c = blockIdx.x * 4 + wave; c < n; c += nwaves) {
    const double* sc = S + (int64_t)c * lds;
    uint64_t key[ITEMS];
    double raw[ITEMS];
    int lane_o = lane;                       // opaque per column: the offsets are recomputed, not kept in ITEMS registers
    asm volatile("" : "+v"(lane_o));
    // The first FULL = ITEMS - 16 rows of 64 lie inside every column this instantiation is launched for (m > 64 FULL):
    // plain loads, no mask.  Only the last 16 rows can reach past the column's end: clamped address, masked below.
    constexpr int FULL = ITEMS - 16;
    const double* __restrict__ scl = sc + lane_o;
    // A 16-byte aligned column reads those FULL rows two values per lane: 8-byte loads run at 0.54-0.70 of the rate of
    // 16-byte ones on this part, and this read is half of the kernel's time.  Which lane and register hold which value
    // does not matter to the selection.  A column that starts on an odd multiple of 8 bytes keeps the 8-byte loads.
#if PLAIDHIP_MED_PAIR_LOADS
    const bool pairs = FULL > 0 && __builtin_amdgcn_readfirstlane((int)(reinterpret_cast<uintptr_t>(sc) & 15u)) == 0;
#else
    constexpr bool pairs = false;
#endif
    if (pairs) {
      const f64x2_t* __restrict__ sp = reinterpret_cast<const f64x2_t*>(sc) + lane_o;
#pragma unroll
      for (int jj = 0; jj < FULL / 2; ++jj) {
        const f64x2_t v2 = __builtin_nontemporal_load(sp + jj * 64);
        raw[2 * jj] = v2.x;
        raw[2 * jj + 1] = v2.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < FULL; ++j) raw[j] = __builtin_nontemporal_load(scl + j * 64);
    }
#pragma unroll
    for (int j = FULL; j < ITEMS; ++j) {
      const int i = lane_o + j * 64;
      raw[j] = __builtin_nontemporal_load(sc + (i < m ? i : m - 1));
    }
    // (the bound is re-read through an opaque copy: the lane masks of the address clamps above must not be kept in
    //  scalar registers until the values arrive)
    int m_use = m;
    asm volatile("" : "+s"(m_use));
    // a valid key never has an all-ones high dword (that would be a NaN): masked <=> high dword == ~0
    uint32_t hmn = ~0u, hmx = 0u, cnt = 0;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      // masked_key() in 32-bit steps, all-ones for NaN, ignored zeros and the rows behind the column's end
      const double v = raw[j];
      const double c0 = v + 0.0;                                   // -0 -> +0
      const uint32_t h0 = (uint32_t)__double2hiint(c0), l0 = (uint32_t)__double2loint(c0);
      const uint32_t sgn = (uint32_t)((int32_t)h0 >> 31);
      bool masked = (v != v) | ((ignore_zero != 0) & (v == 0.0));
      if (j >= FULL) masked = masked | (lane_o + j * 64 >= m_use);
      const uint32_t h = masked ? ~0u : (h0 ^ (sgn | 0x80000000u));
      uint32_t l = masked ? ~0u : (l0 ^ sgn);
      asm volatile("" : "+v"(l));   // computed HERE: hipcc otherwise sinks it to its first use and keeps sign, mask and raw dword per key until then
      key[j] = ((uint64_t)h << 32) | l;
      cnt += (uint32_t)__popcll(__ballot(h != ~0u));
      hmn = h < hmn ? h : hmn;
      const uint32_t hx = masked ? 0u : h;
      hmx = hx > hmx ? hx : hmx;
      if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // (keeps the unrolled loops from running ahead: registers)
    }
    hmn = wave_min_u32(hmn);
    hmx = wave_max_u32(hmx);
    PH_MSTAMP(0)   // loads + keys + min/max
    double r;
    if (cnt == 0) {
      r = ignore_zero ? 0.0 : __longlong_as_double(0x7ff8000000000000ll);
    } else {
      const uint32_t k_lo = (cnt - 1) >> 1, k_hi = cnt >> 1;
      uint64_t lo = (uint64_t)hmn << 32, range = ((uint64_t)(hmx - hmn) << 32) | 0xffffffffull;
      if (hmx == hmn) {
        // every valid key shares its high dword (constant or nearly constant column): exact [min, max] of the low dwords
        uint32_t lmn = ~0u, lmx = 0u;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
          const bool valid = (uint32_t)(key[j] >> 32) != ~0u;
          const uint32_t l = (uint32_t)key[j];
          lmn = (valid && l < lmn) ? l : lmn;
          lmx = (valid && l > lmx) ? l : lmx;
        }
        lmn = wave_min_u32(lmn);
        lmx = wave_max_u32(lmx);
        lo |= (uint64_t)lmn;
        range = (uint64_t)(lmx - lmn);
      }
      uint32_t k = k_lo;         // rank wanted inside [lo, lo + range]
      uint32_t count = cnt;      // keys inside [lo, lo + range]
      while (range != 0ull && count > 1u) {
        const int bits = 64 - __clzll((long long)range);
        const int shift = bits > 8 ? bits - 8 : 0;
        if (shift >= 32) {
          // lo has a zero low dword and range an all-ones one (true of the first range and kept by every pass that
          // shifts by >= 32): bin and range test from the high dwords alone
          const uint32_t lo_h = (uint32_t)(lo >> 32), range_h = (uint32_t)(range >> 32);
          const int sh = shift - 32;
#pragma unroll
          for (int j = 0; j < ITEMS; ++j) {
            const uint32_t dh = (uint32_t)(key[j] >> 32) - lo_h;      // below lo wraps above every range; masked keys lie above
            const uint32_t bin = (dh <= range_h) ? (dh >> sh) : trash;
            atomicAdd(&hist[bin], 1u);
            if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
          }
        } else {
#pragma unroll
          for (int j = 0; j < ITEMS; ++j) {
            const uint64_t d = key[j] - lo;
            const uint32_t bin = (d <= range) ? (uint32_t)(d >> shift) : trash;
            atomicAdd(&hist[bin], 1u);
            if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
          }
        }
        wave_lds_sync();
        // lane l owns bins 4l .. 4l+3
        const uint4 h4 = *reinterpret_cast<const uint4*>(&hist[lane * 4]);
        *reinterpret_cast<uint4*>(&hist[lane * 4]) = make_uint4(0u, 0u, 0u, 0u);
        const uint32_t mine = h4.x + h4.y + h4.z + h4.w;
        const uint32_t incl = wave_scan_add_u32(mine);
        uint32_t excl = incl - mine;
        const bool here = mine != 0 && excl <= k && k < incl;
        uint32_t d = 0, hh = h4.x;
        if (here) {
          if (k >= excl + h4.x) { excl += h4.x; d = 1; hh = h4.y;
            if (k >= excl + h4.y) { excl += h4.y; d = 2; hh = h4.z;
              if (k >= excl + h4.z) { excl += h4.z; d = 3; hh = h4.w; } } }
        }
        const int src = __builtin_ctzll(__ballot(here));     // exactly one lane holds the wanted rank
        const uint32_t dsel = (uint32_t)__builtin_amdgcn_readlane((int)((uint32_t)lane * 4u + d), src);
        const uint32_t below = (uint32_t)__builtin_amdgcn_readlane((int)excl, src);
        count = (uint32_t)__builtin_amdgcn_readlane((int)hh, src);
        wave_lds_sync();
        k -= below;
        lo += (uint64_t)dsel << shift;
        range = shift ? ((1ull << shift) - 1ull) : 0ull;
#ifdef PLAIDHIP_DIAG
        ++npass;
#endif
      }
      PH_MSTAMP(1)   // histogram passes
      uint64_t V = lo;                       // range == 0: `count` copies of lo
      if (range != 0ull) {                   // a single key inside a wider bin: fetch it
        uint64_t f = ~0ull;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
          const uint64_t d = key[j] - lo;
          f = (d <= range) ? key[j] : f;
          if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        V = wave_min_u64(f);
      }
      const uint32_t c_le = (k_lo - k) + count;   // keys <= V
      uint64_t V2 = V;
      if (k_hi != k_lo && k_hi >= c_le) {
        // even count and the upper middle is the next distinct key: smallest key above V
        uint64_t mn = ~0ull;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
          const uint64_t t = key[j] - V - 1ull;        // key <= V wraps to the top
          mn = t < mn ? t : mn;
          if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        V2 = wave_min_u64(mn) + V + 1ull;
      }
      r = (V2 == V) ? key_to_f64(V) : midpoint_f64(key_to_f64(V), key_to_f64(V2));
    }
    if (lane == 0) med[c] = r;
    PH_MSTAMP(2)   // single-key fetch + upper middle
  }
#ifdef PLAIDHIP_DIAG
  if (dbg != nullptr && lane == 0) {
    unsigned long long* d = dbg + (size_t)(blockIdx.x * 4 + wave) * 4;
    d[0] = st[0]; d[1] = st[1]; d[2] = st[2]; d[3] = npass;
  }
#endif
#undef PH_MSTAMP
}

// key of one value as two dwords (same order as masked_key), masked entries -> {~0, ~0}
struct Key32 { uint32_t hi, lo; };
__device__ __forceinline__ Key32 masked_key32(double v, int ignore_zero) {
  const double c = v + 0.0;                                    // -0 -> +0
  const uint32_t h = (uint32_t)__double2hiint(c), l = (uint32_t)__double2loint(c);
  const uint32_t sgn = (uint32_t)((int32_t)h >> 31);           // 0 / ~0
  Key32 k{h ^ (sgn | 0x80000000u), l ^ sgn};
  const bool masked = (v != v) | ((ignore_zero != 0) & (v == 0.0));
  if (masked) { k.hi = 0xffffffffu; k.lo = 0xffffffffu; }
  return k;
}

// One wavefront visits every key of a column: f(key) is called by ALL lanes together (masked or
// out-of-range entries carry the all-ones key), 16-byte loads, 8 KiB per wavefront in flight.
template <typename F>
__device__ __forceinline__ void sweep_column(const double* __restrict__ sc, int32_t m, int ignore_zero, int lane, F&& f) {
  constexpr int UN = 8;
  const int head = (int)((reinterpret_cast<uintptr_t>(sc) >> 3) & 1u);   // first element not 16-byte aligned
  const int npairs = (m - head) >> 1;
  const int tail = (m - head) & 1;
  {
    Key32 k{0xffffffffu, 0xffffffffu};
    if (lane == 0 && head) k = masked_key32(sc[0], ignore_zero);
    if (lane == 1 && tail) k = masked_key32(sc[m - 1], ignore_zero);
    f(k);
  }
  const f64x2_t* __restrict__ p = reinterpret_cast<const f64x2_t*>(sc + head);
  for (int base = 0; base < npairs; base += 64 * UN) {
    f64x2_t v[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int i = base + u * 64 + lane;
      v[u] = p[i < npairs ? i : npairs - 1];
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const bool ok = base + u * 64 + lane < npairs;
      Key32 a = masked_key32(v[u].x, ignore_zero), b = masked_key32(v[u].y, ignore_zero);
      if (!ok) { a.hi = a.lo = b.hi = b.lo = 0xffffffffu; }
      f(a);
      f(b);
    }
  }
}

// The same walk handing out the raw doubles: f(value, exists) is called by ALL lanes together.
template <typename F>
__device__ __forceinline__ void sweep_column_f64(const double* __restrict__ sc, int32_t m, int lane, F&& f) {
  constexpr int UN = 8;
  const int head = (int)((reinterpret_cast<uintptr_t>(sc) >> 3) & 1u);   // first element not 16-byte aligned
  const int npairs = (m - head) >> 1;
  const int tail = (m - head) & 1;
  {
    double v = 0.0;
    bool ok = false;
    if (lane == 0 && head) { v = sc[0]; ok = true; }
    if (lane == 1 && tail) { v = sc[m - 1]; ok = true; }
    f(v, ok);
  }
  const f64x2_t* __restrict__ p = reinterpret_cast<const f64x2_t*>(sc + head);
  for (int base = 0; base < npairs; base += 64 * UN) {
    f64x2_t v[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int i = base + u * 64 + lane;
      v[u] = p[i < npairs ? i : npairs - 1];
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const bool ok = base + u * 64 + lane < npairs;
      f(v[u].x, ok);
      f(v[u].y, ok);
    }
  }
}

// The same walk, software-pipelined: the 8 KiB of batch k + 1 are requested before batch k is processed (two register
// buffers), so a wavefront always has a batch in flight while it classifies the previous one.  The plain walk issues a
// batch, waits for all of it, processes it, and only then asks for the next: with the 16 wavefronts per CU this kernel's
// LDS lists allow, the column sweep ran at 3.5 TB/s with the vector units 60 % idle.  f must issue the same memory
// operations for every batch (no wave-uniform branch around a store): hipcc's wait counters then stay exact and the
// wait before batch k is "all but the 8 loads of batch k + 1", not "everything".  after_batch() runs behind every batch
// (wave-uniform work: flushing a staging list).
template <typename F, typename G>
__device__ __forceinline__ void sweep_column_f64_pipelined(const double* __restrict__ sc, int32_t m, int lane, F&& f, G&& after_batch) {
  constexpr int UN = 8;
  const int head = (int)((reinterpret_cast<uintptr_t>(sc) >> 3) & 1u);   // first element not 16-byte aligned
  const int npairs = (m - head) >> 1;
  const int tail = (m - head) & 1;
  {
    double v = 0.0;
    bool ok = false;
    if (lane == 0 && head) { v = sc[0]; ok = true; }
    if (lane == 1 && tail) { v = sc[m - 1]; ok = true; }
    f(v, ok);
    after_batch();
  }
  const f64x2_t* __restrict__ p = reinterpret_cast<const f64x2_t*>(sc + head);
  f64x2_t va[UN], vb[UN];
#define PH_SWEEP_LOAD(buf, b0)                                          \
  _Pragma("unroll") for (int u = 0; u < UN; ++u) {                       \
    const int i = (b0) + u * 64 + lane;                                  \
    buf[u] = __builtin_nontemporal_load(p + (i < npairs ? i : (npairs > 0 ? npairs - 1 : 0))); \
  }
#define PH_SWEEP_USE(buf, b0)                                            \
  _Pragma("unroll") for (int u = 0; u < UN; ++u) {                       \
    const bool ok = (b0) + u * 64 + lane < npairs;                       \
    f(buf[u].x, ok);                                                     \
    f(buf[u].y, ok);                                                     \
  }
  if (npairs > 0) {
    PH_SWEEP_LOAD(va, 0)
    for (int base = 0; base < npairs; base += 2 * 64 * UN) {
      PH_SWEEP_LOAD(vb, base + 64 * UN)
      PH_SWEEP_USE(va, base)
      after_batch();
      PH_SWEEP_LOAD(va, base + 2 * 64 * UN)
      PH_SWEEP_USE(vb, base + 64 * UN)
      after_batch();
    }
  }
#undef PH_SWEEP_LOAD
#undef PH_SWEEP_USE
}

// k-th smallest (0-based) of the wavefront's register-resident keys (ITEMS per lane; all-ones = no key) by radix selection
// over [kmin, kmax] with the wavefront's own histogram (256 bins + a trash bin per lane, all zero on entry and on return):
// the selection loop of col_medians_wave_kernel in its plain 64-bit form.  `count` = number of keys.
template <int ITEMS>
__device__ __forceinline__ uint64_t wave_radix_select(const uint64_t (&key)[ITEMS], uint32_t k, uint32_t count, uint64_t kmin,
                                                      uint64_t kmax, uint32_t* hist, int lane) {
  const uint32_t trash = 256u + (uint32_t)lane;
  uint64_t lo = kmin, range = kmax - kmin;
  while (range != 0ull && count > 1u) {
    const int bits = 64 - __clzll((long long)range);
    const int shift = bits > 8 ? bits - 8 : 0;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      const uint64_t d = key[j] - lo;          // below lo wraps above every range in use; all-ones lies above kmax
      atomicAdd(&hist[(d <= range) ? (uint32_t)(d >> shift) : trash], 1u);
    }
    wave_lds_sync();
    const uint4 h4 = *reinterpret_cast<const uint4*>(&hist[lane * 4]);
    *reinterpret_cast<uint4*>(&hist[lane * 4]) = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t mine = h4.x + h4.y + h4.z + h4.w;
    const uint32_t incl = wave_scan_add_u32(mine);
    uint32_t excl = incl - mine;
    const bool here = mine != 0 && excl <= k && k < incl;
    uint32_t d = 0, hh = h4.x;
    if (here) {
      if (k >= excl + h4.x) { excl += h4.x; d = 1; hh = h4.y;
        if (k >= excl + h4.y) { excl += h4.y; d = 2; hh = h4.z;
          if (k >= excl + h4.z) { excl += h4.z; d = 3; hh = h4.w; } } }
    }
    const int src = __builtin_ctzll(__ballot(here));
    const uint32_t dsel = (uint32_t)__builtin_amdgcn_readlane((int)((uint32_t)lane * 4u + d), src);
    const uint32_t below = (uint32_t)__builtin_amdgcn_readlane((int)excl, src);
    count = (uint32_t)__builtin_amdgcn_readlane((int)hh, src);
    wave_lds_sync();
    k -= below;
    lo += (uint64_t)dsel << shift;
    range = shift ? ((1ull << shift) - 1ull) : 0ull;
  }
  if (range == 0ull) return lo;              // `count` copies of lo
  uint64_t f = ~0ull;                        // a single key inside a wider bin: fetch it
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const uint64_t d = key[j] - lo;
    f = (d <= range) ? key[j] : f;
  }
  return wave_min_u64(f);
}

// The search interval is [lo, lo + 2^B - 1]; a key K lies inside iff K - lo does not borrow and
// (K - lo) >> B == 0.  Its bin is (K - lo) >> shift, shift = max(B - 8, 0).  Everything per key is
// 32-bit arithmetic (64-bit integer compares and shifts run at a quarter of that rate).
struct RangeTest {
  uint32_t lohi, lolo;
  int shift;        // bin = d >> shift
  uint32_t nbins;   // 1 << (B - shift) <= 256
  // returns the bin, or 0xffffffff when the key is outside the interval
  __device__ __forceinline__ uint32_t bin(const Key32& k) const {
    const uint32_t dlo = k.lo - lolo;
    const uint32_t borrow = k.lo < lolo ? 1u : 0u;
    const uint32_t dhi = k.hi - lohi - borrow;
    const bool under = (k.hi < lohi) | ((k.hi == lohi) & (borrow != 0u));
    uint32_t b;
    bool hi_ok = true;
    if (shift >= 32) {
      b = dhi >> (shift - 32);
    } else {
      b = shift ? __builtin_amdgcn_alignbit(dhi, dlo, (uint32_t)shift) : dlo;
      hi_ok = (dhi >> shift) == 0u;   // shift == 0: dhi must be 0
    }
    const bool valid = k.hi != 0xffffffffu;   // masked entries (no valid key has an all-ones high word)
    return (valid && !under && hi_ok && b < nbins) ? b : 0xffffffffu;
  }
};

// Any m: ONE WAVEFRONT per column, no workgroup barriers.  The column is swept three or four
// times (the first sweep from HBM, the others from L2): min/max of the keys; a 256-bin histogram
// over the current key range (repeated on the bin that holds the wanted rank while that bin has
// more than CAP keys); a collect sweep that compacts the keys of the bin into LDS, where the
// wavefront sorts them (bitonic) and reads the middle key(s) off.  Every wavefront works on its
// own column with its own 1 KiB histogram and CAP-key list, so a CU keeps 16 columns in flight
// and nothing waits for another wavefront.  Columns of more than 4 CAP values begin with a sampled
// start instead (below): one sweep that replaces the min/max sweep and the first histogram sweeps,
// and leaves the keys near the middle rank in a candidate list that the collect step reads.
template <int CAP, int kSampleChunks>   // kSampleChunks x 64 sample values, spread over the column
__global__ void __launch_bounds__(256, 4)   // four workgroups per CU is what the LDS lists allow: 128 registers
col_medians_stream_kernel(const double* __restrict__ S, int64_t lds, int32_t m, int32_t n,
                          int ignore_zero_mode, const uint32_t* __restrict__ flags,
                          double* __restrict__ med, unsigned long long* __restrict__ cand_all, int32_t ccap,
                          unsigned long long* __restrict__ dbg, const int32_t* __restrict__ status = nullptr) {
#ifdef PLAIDHIP_DIAG
#define PH_SSTAMP(k) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st[k] += t_ - tl; tl = t_; }
  unsigned long long st[6] = {0, 0, 0, 0, 0, 0}, tl = __builtin_amdgcn_s_memtime();
#else
#define PH_SSTAMP(k)
#endif
  // (+64: a private trash bin / trash slot per lane, so that the classification sweep below is free of branches)
  __shared__ __align__(16) uint32_t s_hist[4][256 + 64];
  __shared__ unsigned long long s_list[4][CAP + 64];
  // (measured on 8,192 columns x 50k: 16 chunks no faster than 8; 3 sigma 20 % SLOWER -- a miss costs three sweeps)
  constexpr float kSampleSigmas = 4.0f;
  const int ignore_zero = resolve_ignore_zero(ignore_zero_mode, flags);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* hist = s_hist[wave];
  unsigned long long* list = s_list[wave];
  *reinterpret_cast<uint4*>(&hist[lane * 4]) = make_uint4(0u, 0u, 0u, 0u);
  wave_lds_sync();

  const int nwaves = gridDim.x * 4;
  // this wavefront's candidate list in global memory (see the sampled start below)
  unsigned long long* cand = cand_all != nullptr ? cand_all + (size_t)(blockIdx.x * 4 + wave) * (size_t)ccap : nullptr;
  for (int c = blockIdx.x * 4 + wave; c < n; c += nwaves) {
    if (status != nullptr && status[c] != 0) continue;   // (wave-uniform) its median came out of the crossprod launch
    const double* sc = S + (int64_t)c * lds;
    uint32_t cnt = 0, k_lo = 0, k_hi = 0, k = 0, count = 0;
    uint32_t ncand = 0;          // keys of the sample interval written to `cand` by the sampled start (0: none / overflow)
    uint64_t hi_cap = ~0ull;     // sampled start: its counts cover the keys <= qb only (the histogram interval is padded
                                 // to a power of two and may reach beyond qb) -- every later sweep applies the same cap
    uint64_t lo = 0;
    int B = 0;
    bool seeded = false;
    // ---- sampled start (large columns): a 512-entry sample (8 chunks spread over the column) gives a key
    //      interval around the middle rank, 4 sigma of a sample quantile either side; ONE sweep then counts the
    //      valid keys, the keys below the interval and a 256-bin histogram inside it, which replaces the min/max
    //      sweep and the first two histogram sweeps of the generic path.  If the interval misses the middle
    //      rank (probability ~1e-4 per column for exchangeable data) the generic path starts from scratch.
    if (m > 4 * CAP) {
      // the sample stays in registers (8 keys per lane) and the two bracket keys are SELECTED (two short radix
      // selections on the wavefront's histogram) instead of read off a sorted list: sorting 512 keys in LDS was 45
      // compare-exchange stages with four round trips each, 13 % of the kernel's time (in-kernel stamps)
      uint64_t skey[kSampleChunks];
      double sraw[kSampleChunks];
#pragma unroll
      for (int u = 0; u < kSampleChunks; ++u) {
        int64_t i = (int64_t)u * m / kSampleChunks + lane;
        sraw[u] = sc[i < m ? i : m - 1];
      }
      uint32_t ns = 0;
      uint64_t smn = ~0ull, smx = 0ull;
#pragma unroll
      for (int u = 0; u < kSampleChunks; ++u) {
        const uint64_t kk = masked_key(sraw[u], ignore_zero);
        skey[u] = kk;
        const bool valid = kk != ~0ull;
        ns += (uint32_t)__popcll(__ballot(valid));
        smn = kk < smn ? kk : smn;
        smx = (valid && kk > smx) ? kk : smx;
      }
      smn = wave_min_u64(smn);
      smx = wave_max_u64(smx);
      const uint32_t mid = ns > 0 ? (ns - 1u) >> 1 : 0u;
      const uint32_t w = (uint32_t)(kSampleSigmas * 0.5f * sqrtf((float)ns)) + 2u;   // kSampleSigmas sigma of a sample quantile's rank
      if (ns >= 256u && mid > w && mid + 1u + w < ns - 1u) {
        const uint64_t qa = wave_radix_select<kSampleChunks>(skey, mid - w, ns, smn, smx, hist, lane);
        const uint64_t qb = wave_radix_select<kSampleChunks>(skey, mid + 1u + w, ns, smn, smx, hist, lane);
        const int Bw = qb == qa ? 1 : 64 - __clzll((long long)(qb - qa));   // [qa, qa + 2^Bw - 1] covers [qa, qb]
        RangeTest rt;
        rt.lohi = (uint32_t)(qa >> 32);
        rt.lolo = (uint32_t)qa;
        rt.shift = Bw > 8 ? Bw - 8 : 0;
        rt.nbins = 1u << (Bw - rt.shift);
        // ONE sweep: classification on the doubles themselves (three compares per key; counters in scalar registers
        // through ballots), and only the keys inside [qa, qb] -- a sixth of the column -- are turned into keys, binned
        // and appended to this wavefront's candidate list in global memory; the selection below then reads the list
        // instead of sweeping the column a second time (1.36 instead of 2 passes over a column that fits no cache).
        const double qa_d = key_to_f64(qa), qb_d = key_to_f64(qb);
        uint32_t below = 0;
        PH_SSTAMP(0)   // sample: strided loads + sort
        // Branch-free per value: every lane counts into the histogram (lanes outside the interval into their private trash
        // bin) and writes its key into the wavefront's LDS list (outside the interval, or past the list's end: into its
        // trash slot), so the 16 values of a batch are one basic block the scheduler can interleave.  Behind each batch
        // the staged keys -- about a sixth of the batch -- go to the candidate list in global memory with full-wave
        // stores.  A batch that stages more than CAP keys (an interval far too wide: heavy ties) gives the list up; the
        // collect sweep then reads the column, as it does without a list.
        uint32_t nstage = 0;
        bool list_ok = cand != nullptr;
        const uint32_t trash_bin = 256u + (uint32_t)lane, trash_slot = (uint32_t)CAP + (uint32_t)lane;
        auto classify = [&](auto iz_c) {
          return [&](double v, bool ok) {
          // (ordered compares are false for a NaN: `lt` and `in` need no validity test of their own)
          // The wave-level masks are built from ballots of SINGLE compares combined with scalar ANDs: the ballot of a
          // combined predicate is materialised by hipcc as v_cndmask + v_cmp per ballot (6 of the 31 vector instructions
          // per value); the lane's own `in` below is the same combination as a predicate (scalar ANDs of the same masks).
          const bool nz = decltype(iz_c)::value ? (v != 0.0) : true;
          const bool in = ok && nz && !(v < qa_d) && (v <= qb_d);
          const unsigned long long ltm_ = __ballot(v < qa_d);
          unsigned long long live = __ballot(ok) & __ballot(v == v);
          if (decltype(iz_c)::value) live &= __ballot(v != 0.0);
          const unsigned long long bal = live & __ballot(v <= qb_d) & ~ltm_;
          cnt += (uint32_t)__popcll(live);
          below += (uint32_t)__popcll(live & ltm_);
          const double c0 = v + 0.0;                                   // -0 -> +0
          const uint32_t h = (uint32_t)__double2hiint(c0), l = (uint32_t)__double2loint(c0);
          const uint32_t sgn = (uint32_t)((int32_t)h >> 31);
          const uint64_t key = ((uint64_t)(h ^ (sgn | 0x80000000u)) << 32) | (uint64_t)(l ^ sgn);
          const uint32_t b = (uint32_t)((key - qa) >> rt.shift);
          atomicAdd(&hist[in ? b : trash_bin], 1u);
          const uint32_t pos = nstage + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
          list[(in && pos < (uint32_t)CAP) ? pos : trash_slot] = key;
          nstage += (uint32_t)__popcll(bal);
        };
        };
        auto flush = [&]() {
          nstage = (uint32_t)__builtin_amdgcn_readfirstlane((int)nstage);
          if (nstage > (uint32_t)CAP) list_ok = false;
          if (list_ok && nstage != 0u) {
            wave_lds_sync();
            for (uint32_t i = (uint32_t)lane; i < nstage; i += 64u)
              if (ncand + i < (uint32_t)ccap) cand[ncand + i] = list[i];
            wave_lds_sync();
          }
          ncand += nstage;
          nstage = 0;
        };
        // (the ignore.zero test is compiled in or out: it is the same for every column of the call)
        if (ignore_zero != 0) sweep_column_f64_pipelined(sc, m, lane, classify(std::true_type{}), flush);
        else sweep_column_f64_pipelined(sc, m, lane, classify(std::false_type{}), flush);
        if (!list_ok) ncand = 0xffffffffu;
        PH_SSTAMP(1)   // classification sweep
        cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt);
        below = (uint32_t)__builtin_amdgcn_readfirstlane((int)below);
        ncand = (uint32_t)__builtin_amdgcn_readfirstlane((int)ncand);
        if (cand == nullptr || ncand > (uint32_t)ccap) ncand = 0;   // no list (or given up, or overflown): the collect sweep reads the column
        wave_lds_sync();
        const uint4 h4 = *reinterpret_cast<const uint4*>(&hist[lane * 4]);
        *reinterpret_cast<uint4*>(&hist[lane * 4]) = make_uint4(0u, 0u, 0u, 0u);
        wave_lds_sync();
        const uint32_t mine = h4.x + h4.y + h4.z + h4.w;
        const uint32_t incl = wave_scan_add_u32(mine);
        const uint32_t inside = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (cnt > 0u) {
          k_lo = (cnt - 1u) >> 1;
          k_hi = cnt >> 1;
          if (below <= k_lo && k_lo - below < inside) {
            k = k_lo - below;
            uint32_t excl = incl - mine;
            const bool owner = mine != 0 && excl <= k && k < incl;
            uint32_t d = 0, hh = h4.x;
            if (k >= excl + h4.x) { excl += h4.x; d = 1; hh = h4.y;
              if (k >= excl + h4.y) { excl += h4.y; d = 2; hh = h4.z;
                if (k >= excl + h4.z) { excl += h4.z; d = 3; hh = h4.w; } } }
            const int src = (int)__builtin_ctzll(__ballot(owner));
            const uint32_t dsel = (uint32_t)__builtin_amdgcn_readlane((int)((uint32_t)lane * 4u + d), src);
            k -= (uint32_t)__builtin_amdgcn_readlane((int)excl, src);
            count = (uint32_t)__builtin_amdgcn_readlane((int)hh, src);
            lo = qa + ((uint64_t)dsel << rt.shift);
            B = rt.shift;
            seeded = true;
            hi_cap = qb;
          }
        }
        if (!seeded) ncand = 0;
      } else {
        wave_lds_sync();
      }
    }
    PH_SSTAMP(2)   // scan of the seeded histogram
    if (!seeded) {
    // ---- generic start, sweep 0: range of the keys' high words and the number of unmasked entries ---------
    uint32_t hmin = 0xffffffffu, hmax = 0u;
    cnt = 0;
    sweep_column(sc, m, ignore_zero, lane, [&](const Key32& k_) {
      const bool valid = k_.hi != 0xffffffffu;      // no valid key has an all-ones high word
      cnt += valid ? 1u : 0u;
      hmin = k_.hi < hmin ? k_.hi : hmin;            // (a masked key never lowers the minimum)
      hmax = (valid && k_.hi > hmax) ? k_.hi : hmax;
    });
    for (int off = 32; off >= 1; off >>= 1) {
      const uint32_t a_ = __shfl_xor(hmin, off, 64), b_ = __shfl_xor(hmax, off, 64);
      hmin = a_ < hmin ? a_ : hmin;
      hmax = b_ > hmax ? b_ : hmax;
      cnt += __shfl_xor(cnt, off, 64);
    }
    cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt);
    hmin = (uint32_t)__builtin_amdgcn_readfirstlane((int)hmin);
    hmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)hmax);
    if (cnt != 0u) {
      k_lo = (cnt - 1) >> 1;
      k_hi = cnt >> 1;
      lo = (uint64_t)hmin << 32;
      B = 32 + (hmax == hmin ? 0 : 32 - __clz((int)(hmax - hmin)));   // interval [lo, lo + 2^B - 1] holds every key
      k = k_lo;       // rank wanted inside the interval
      count = cnt;    // keys inside the interval
    }
    }
    double r;
    if (cnt == 0) {
      r = ignore_zero ? 0.0 : __longlong_as_double(0x7ff8000000000000ll);
    } else {
      // ---- histogram sweeps until the interval fits the list ------------------------------
      while (B != 0 && count > (uint32_t)CAP) {
        RangeTest rt;
        rt.lohi = (uint32_t)(lo >> 32);
        rt.lolo = (uint32_t)lo;
        rt.shift = B > 8 ? B - 8 : 0;
        rt.nbins = 1u << (B - rt.shift);
        sweep_column(sc, m, ignore_zero, lane, [&](const Key32& key) {
          const uint32_t b = rt.bin(key);
          if (b != 0xffffffffu && ((((uint64_t)key.hi << 32) | key.lo) <= hi_cap)) atomicAdd(&hist[b], 1u);
        });
        wave_lds_sync();
        const uint4 h4 = *reinterpret_cast<const uint4*>(&hist[lane * 4]);
        *reinterpret_cast<uint4*>(&hist[lane * 4]) = make_uint4(0u, 0u, 0u, 0u);
        wave_lds_sync();
        const uint32_t mine = h4.x + h4.y + h4.z + h4.w;
        const uint32_t incl = wave_scan_add_u32(mine);
        uint32_t excl = incl - mine;
        const bool owner = mine != 0 && excl <= k && k < incl;
        uint32_t d = 0, hh = h4.x;
        if (k >= excl + h4.x) { excl += h4.x; d = 1; hh = h4.y;
          if (k >= excl + h4.y) { excl += h4.y; d = 2; hh = h4.z;
            if (k >= excl + h4.z) { excl += h4.z; d = 3; hh = h4.w; } } }
        const int src = (int)__builtin_ctzll(__ballot(owner));   // exactly one lane owns the wanted rank
        const uint32_t dsel = (uint32_t)__builtin_amdgcn_readlane((int)((uint32_t)lane * 4u + d), src);
        const uint32_t below = (uint32_t)__builtin_amdgcn_readlane((int)excl, src);
        count = (uint32_t)__builtin_amdgcn_readlane((int)hh, src);
        k -= below;
        lo += (uint64_t)dsel << rt.shift;
        B = rt.shift;
      }
      PH_SSTAMP(3)   // generic start / further histogram sweeps (none after a seeded start that fits the list)
      uint64_t V = lo, V2 = lo;
      bool need_above = false;
      if (B != 0) {
        // ---- collect sweep: keys of the interval -> LDS ------------------------------------
        RangeTest rt;
        rt.lohi = (uint32_t)(lo >> 32);
        rt.lolo = (uint32_t)lo;
        rt.shift = B > 8 ? B - 8 : 0;
        rt.nbins = 1u << (B - rt.shift);
        uint32_t base = 0;
        auto collect = [&](const Key32& key) {
          const bool in = rt.bin(key) != 0xffffffffu && ((((uint64_t)key.hi << 32) | key.lo) <= hi_cap);
          const unsigned long long bal = __ballot(in);
          if (in) {
            const uint32_t pos = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            if (pos < (uint32_t)CAP) list[pos] = ((unsigned long long)key.hi << 32) | key.lo;
          }
          base += (uint32_t)__popcll(bal);
        };
        if (ncand != 0u) {
          // the interval lies inside the sample interval: its keys are among the candidates (written by this very
          // wavefront a moment ago: same-wave stores and loads are ordered)
          // (16-byte loads, 8 KiB per batch, the next batch requested before the current one is used: read 256 keys at a
          //  time with a round trip each, this loop was most of the 18 % of the kernel spent behind the sweep)
          typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));
          const u64x2_t* __restrict__ cp = reinterpret_cast<const u64x2_t*>(cand);
          const uint32_t npair = (ncand + 1u) >> 1;   // (an odd count reads one slot past the last key: inside the list, masked below)
          constexpr int CB = 8;
          u64x2_t ka[CB], kb[CB];
#define PH_CAND_LOAD(buf, b0)                                            \
  _Pragma("unroll") for (int u = 0; u < CB; ++u) {                        \
    const uint32_t i = (b0) + (uint32_t)u * 64u + (uint32_t)lane;         \
    buf[u] = cp[i < npair ? i : npair - 1u];                              \
  }
#define PH_CAND_USE(buf, b0)                                              \
  _Pragma("unroll") for (int u = 0; u < CB; ++u) {                        \
    const uint32_t i = 2u * ((b0) + (uint32_t)u * 64u + (uint32_t)lane);  \
    Key32 k0{(uint32_t)(buf[u].x >> 32), (uint32_t)buf[u].x}, k1{(uint32_t)(buf[u].y >> 32), (uint32_t)buf[u].y}; \
    if (i >= ncand) { k0.hi = 0xffffffffu; k0.lo = 0xffffffffu; }         \
    if (i + 1u >= ncand) { k1.hi = 0xffffffffu; k1.lo = 0xffffffffu; }    \
    collect(k0);                                                          \
    collect(k1);                                                          \
  }
          PH_CAND_LOAD(ka, 0u)
          for (uint32_t i0 = 0; i0 < npair; i0 += 2u * 64u * CB) {
            PH_CAND_LOAD(kb, i0 + 64u * CB)
            PH_CAND_USE(ka, i0)
            PH_CAND_LOAD(ka, i0 + 2u * 64u * CB)
            PH_CAND_USE(kb, i0 + 64u * CB)
          }
#undef PH_CAND_LOAD
#undef PH_CAND_USE
        } else {
          sweep_column(sc, m, ignore_zero, lane, collect);
        }
        // ---- sort the list (count <= CAP keys, padded with all-ones to a power of two) ------
        uint32_t N = 2;
        while (N < count) N <<= 1;
        for (uint32_t i = count + lane; i < N; i += 64) list[i] = ~0ull;
        wave_lds_sync();
        for (uint32_t kk = 2; kk <= N; kk <<= 1)
          for (uint32_t j = kk >> 1; j >= 1; j >>= 1) {
            for (uint32_t t = lane; t < (N >> 1); t += 64) {
              const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // lower index of the pair
              const uint32_t p = i | j;
              const bool up = (i & kk) == 0;
              const unsigned long long x = list[i], y = list[p];
              if ((x > y) == up) { list[i] = y; list[p] = x; }
            }
            wave_lds_sync();
          }
        V = list[k];
        V2 = V;
        if (k_hi != k_lo) {
          if (k + 1 < count) V2 = list[k + 1];
          else need_above = true;
        }
        wave_lds_sync();   // the list is refilled by the next column
      } else {
        // `count` copies of the key lo; the upper middle is another copy or the next larger key
        const uint32_t c_le = (k_lo - k) + count;
        need_above = k_hi != k_lo && k_hi >= c_le;
      }
      PH_SSTAMP(4)   // collect (candidates or column) + sort
      if (need_above) {   // rare: the upper middle key is the smallest key above V (one more sweep)
        uint64_t above = ~0ull;
        sweep_column(sc, m, ignore_zero, lane, [&](const Key32& key) {
          const uint64_t kk = ((uint64_t)key.hi << 32) | key.lo;
          above = (kk > V && key.hi != 0xffffffffu && kk < above) ? kk : above;
        });
        for (int off = 32; off >= 1; off >>= 1) {
          const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)above, off, 64);
          above = o < above ? o : above;
        }
        V2 = above;
      }
      r = (V2 == V) ? key_to_f64(V) : midpoint_f64(key_to_f64(V), key_to_f64(V2));
    }
    if (lane == 0) med[c] = r;
    PH_SSTAMP(5)   // upper-middle sweep (rare)
  }
#ifdef PLAIDHIP_DIAG
  if (dbg != nullptr && lane == 0) {
    unsigned long long* d = dbg + (size_t)(blockIdx.x * 4 + wave) * 8;
    for (int q = 0; q < 6; ++q) d[q] = st[q];
  }
#endif
#undef PH_SSTAMP
}

#ifdef PLAIDHIP_DIAG
static unsigned long long* g_med_dbg = nullptr;   // tools/ build: per-phase stamps of the wave-per-column kernel
void debug_set_median_stamps(void* dbg) { g_med_dbg = static_cast<unsigned long long*>(dbg); }
static unsigned long long* median_stamps() { return g_med_dbg; }
#else
static unsigned long long* median_stamps() { return nullptr; }
#endif

template <int ITEMS, int WG_PER_CU>
static void launch_wave(plaidhip_ctx* ctx, const double* S, int64_t lds, int32_t m, int32_t n,
                        int ignore_zero, const uint32_t* flags, double* med) {
  static_assert(ITEMS >= 16 && ITEMS % 16 == 0, "classes of 1,024 values");
  const int cap = ctx->num_cu * WG_PER_CU * 4;            // WG_PER_CU workgroups of four wavefronts per CU, several rounds
  const int need = (n + 3) / 4;
  const int grid = need < cap ? need : cap;
  hipLaunchKernelGGL((col_medians_wave_kernel<ITEMS, WG_PER_CU>), dim3(grid), dim3(256), 0, ctx->stream, S, lds, m, n, ignore_zero,
                     flags, med, median_stamps());
}

// ---- medians selected while the sparse crossprod writes the scores (spmm_scatter_csc_f64<.., MED>, kernels_spmm.hip) ----
// 1. the mean score of every column before the crossprod: alpha * sum_i x[i, c] u[i] + beta * kappa (geneset.cpp: u, kappa)
__global__ void __launch_bounds__(256)
colmean_predict_kernel(const int32_t* __restrict__ Xp, const int32_t* __restrict__ Xi, const double* __restrict__ Xx, int32_t n,
                       const double* __restrict__ u, double alpha, const double* __restrict__ alpha_div, double beta_kappa,
                       double* __restrict__ pred) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double al = alpha_div != nullptr ? alpha / *alpha_div : alpha;
  for (int c = blockIdx.x * 4 + wave; c < n; c += gridDim.x * 4) {
    // (four independent chains: the loop is a load, a dependent gather and an add -- one round trip per 64 values when
    // rolled, 0.54 ms for the 1e8 stored values of config 3)
    const int q1 = Xp[c + 1];
    int q = Xp[c] + lane;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (; q + 192 < q1; q += 256) {
      const int i0 = Xi[q], i1 = Xi[q + 64], i2 = Xi[q + 128], i3 = Xi[q + 192];
      const double x0 = Xx[q], x1 = Xx[q + 64], x2 = Xx[q + 128], x3 = Xx[q + 192];
      s0 += x0 * u[i0];
      s1 += x1 * u[i1];
      s2 += x2 * u[i2];
      s3 += x3 * u[i3];
    }
    for (; q < q1; q += 64) s0 += Xx[q] * u[Xi[q]];
    double s = (s0 + s1) + (s2 + s3);
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) pred[c] = al * s + beta_kappa;
  }
}

// 2. calibration on the first K <= 256 columns (crossprod + standalone medians of those ran before), ROBUST against odd
//    columns among them (empty cells, outliers, NaN): offset = the MEDIAN of (column median - predicted mean), half width =
//    2.3 x the 90th percentile of the absolute deviations from it (normal deviates: 1.645 sigma -> a bracket of ~3.8 sigma
//    either side, 1-5 % of a column's scores); the ignore-zero rule of the sample is what the bracket is calibrated for.
//    Columns outside the bracket are simply left to the standalone kernel.
__global__ void __launch_bounds__(256)
median_calibrate_kernel(const double* __restrict__ medK, const double* __restrict__ pred, int32_t K,
                        const uint32_t* __restrict__ flagsK, double* __restrict__ cal) {
  __shared__ double s_v[256];
  __shared__ double s_pick;
  __shared__ int s_cnt;
  const int t = threadIdx.x;
  double d = INFINITY;
  if (t < K) {
    const double x = medK[t] - pred[t];
    if (x == x && fabs(x) < INFINITY) d = x;
  }
  if (t == 0) s_cnt = 0;
  __syncthreads();
  if (d < INFINITY) atomicAdd(&s_cnt, 1);
  auto select = [&](double mine, int k) {   // the k-th smallest (0-based) of the 256 values, ties by thread index
    s_v[t] = mine;
    __syncthreads();
    int r = 0;
    for (int j = 0; j < 256; ++j) r += (s_v[j] < mine || (s_v[j] == mine && j < t)) ? 1 : 0;
    if (r == k) s_pick = mine;
    __syncthreads();
    const double out = s_pick;
    __syncthreads();
    return out;
  };
  __syncthreads();
  const int n_ok = s_cnt;
  if (n_ok < 16) {   // too few usable columns: an empty bracket (every column goes to the standalone kernel)
    if (t == 0) { cal[0] = 0.0; cal[1] = -1.0; cal[2] = 0.0; }
    return;
  }
  const double off = select(d, (n_ok - 1) / 2);
  const double dev = d < INFINITY ? fabs(d - off) : INFINITY;
  const double q90 = select(dev, (int)(0.9 * (n_ok - 1)));
  if (t == 0) {
    cal[0] = off;
    cal[1] = 2.3 * q90 + 4.0 * fabs(off) * 0x1p-52;
    cal[2] = (flagsK[1] != 0u && flagsK[0] == 0u) ? 1.0 : 0.0;
  }
}

// 3. one wavefront per column: the counts of its (chunk, wavefront) slices say whether both middle order statistics lie
//    among the candidates; if so they are selected from them (<= 64 per lane, in registers: wave_radix_select) -- the same
//    two values the standalone kernels select, averaged the same way.  status[c] = 1: med[c] is final; 0: unresolved
//    (bracket missed, a slice overflowed, empty column, or the matrix as a whole follows the other ignore.zero rule than
//    the calibration sample did).
constexpr int kFmedItems = 64;   // candidates per lane: 4,096 per column
template <int ITEMS>
__device__ __forceinline__ void fmed_select_from(const unsigned long long* __restrict__ cand, int c, int32_t nslice, int32_t capc,
                                                 const uint32_t* s_off, uint32_t total, int64_t k1, int64_t k2, uint32_t below,
                                                 uint32_t* s_hist, int lane, double* __restrict__ med, int32_t* __restrict__ status) {
  // gather the candidates: flat index f -> slice by binary search in the offsets
  uint64_t key[ITEMS];
  uint64_t kmin = ~0ull, kmax = 0ull;
#pragma unroll
  for (int t = 0; t < ITEMS; ++t) {
    const uint32_t f = (uint32_t)t * 64u + (uint32_t)lane;
    uint64_t kk = ~0ull;
    if (f < total) {
      int lo = 0, hi = nslice;              // largest s with s_off[s] <= f
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_off[mid] <= f) lo = mid; else hi = mid; }
      const double v = __longlong_as_double((long long)cand[((int64_t)c * nslice + lo) * capc + (f - s_off[lo])]);
      kk = masked_key(v, 0);
      kmin = kk < kmin ? kk : kmin;
      kmax = kk > kmax ? kk : kmax;
    }
    key[t] = kk;
  }
  kmin = wave_min_u64(kmin);
  kmax = wave_max_u64(kmax);
  const uint64_t a1 = wave_radix_select<ITEMS>(key, (uint32_t)(k1 - below), total, kmin, kmax, s_hist, lane);
  const uint64_t a2 = (k2 == k1) ? a1 : wave_radix_select<ITEMS>(key, (uint32_t)(k2 - below), total, kmin, kmax, s_hist, lane);
  if (lane == 0) {
    med[c] = (a1 == a2) ? key_to_f64(a1) : midpoint_f64(key_to_f64(a1), key_to_f64(a2));
    status[c] = 1;
  }
}

__global__ void __launch_bounds__(64)
median_select_kernel(const unsigned long long* __restrict__ cand, const uint4* __restrict__ cnt, int32_t n, int32_t nslice,
                     int32_t capc, int32_t m, const double* __restrict__ cal, int ignore_zero_mode,
                     const uint32_t* __restrict__ flags, double* __restrict__ med, int32_t* __restrict__ status) {
  __shared__ __align__(16) uint32_t s_hist[256 + 64];
  __shared__ uint32_t s_off[257];
  const int lane = threadIdx.x;
  const int iz_true = resolve_ignore_zero(ignore_zero_mode, flags);
  const bool mode_ok = (cal[2] != 0.0) == (iz_true != 0) && cal[1] >= 0.0;
  *reinterpret_cast<uint4*>(&s_hist[lane * 4]) = make_uint4(0u, 0u, 0u, 0u);
  s_hist[256 + lane] = 0u;
  wave_lds_sync();
  for (int c = blockIdx.x; c < n; c += gridDim.x) {
    // counts of the column's slices (nslice <= 256: chunks x wavefronts)
    uint32_t below = 0, zero = 0, nan = 0, total = 0;
    bool over = false;
    for (int s0 = 0; s0 < nslice; s0 += 64) {
      const int sidx = s0 + lane;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (sidx < nslice) v = cnt[(int64_t)c * nslice + sidx];
      over |= v.w > (uint32_t)capc;
      const uint32_t incl = wave_scan_add_u32(v.w);
      if (sidx < nslice) s_off[sidx] = total + incl - v.w;
      total += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      uint32_t b = v.x, z = v.y, q = v.z;
      for (int off = 32; off >= 1; off >>= 1) { b += __shfl_xor(b, off, 64); z += __shfl_xor(z, off, 64); q += __shfl_xor(q, off, 64); }
      below += b; zero += z; nan += q;
    }
    if (lane == 0) s_off[nslice] = total;
    wave_lds_sync();
    const bool any_over = __ballot(over) != 0ull;
    // (the crossprod launch only notes WHETHER a wavefront wrote NaN scores -- they are skipped, na.rm -- not how many: such
    // a column is left to the standalone kernel)
    const int64_t nv = (int64_t)m - (iz_true ? zero : 0);
    const int64_t k1 = (nv - 1) >> 1, k2 = nv >> 1;
    const bool ok = mode_ok && !any_over && nan == 0 && nv > 0 && total <= (uint32_t)(kFmedItems * 64) && (int64_t)below <= k1 &&
                    k2 < (int64_t)below + total;
    if (!ok) {
      if (lane == 0) status[c] = 0;
      wave_lds_sync();
      continue;
    }
    // (ITEMS candidates per lane, by how many there are: the gather and the selection passes cost in proportion, and a
    // bracket of 1-5 % of 50,000 scores holds 500 ... 2,500 candidates, not the 4,096 the lists could hold)
    if (total <= 8u * 64u) fmed_select_from<8>(cand, c, nslice, capc, s_off, total, k1, k2, below, s_hist, lane, med, status);
    else if (total <= 16u * 64u) fmed_select_from<16>(cand, c, nslice, capc, s_off, total, k1, k2, below, s_hist, lane, med, status);
    else if (total <= 32u * 64u) fmed_select_from<32>(cand, c, nslice, capc, s_off, total, k1, k2, below, s_hist, lane, med, status);
    else fmed_select_from<kFmedItems>(cand, c, nslice, capc, s_off, total, k1, k2, below, s_hist, lane, med, status);
    wave_lds_sync();
  }
}

int launch_colmean_predict(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t n, const double* u,
                           double alpha, const double* alpha_div, double beta_kappa, double* pred) {
  if (n == 0) return PLAIDHIP_OK;
  const int cap = ctx->num_cu * 8;
  const int need = (n + 3) / 4;
  hipLaunchKernelGGL(colmean_predict_kernel, dim3(need < cap ? need : cap), dim3(256), 0, ctx->stream, Xp, Xi, Xx, n, u, alpha,
                     alpha_div, beta_kappa, pred);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_median_calibrate(plaidhip_ctx* ctx, const double* medK, const double* pred, int32_t K, const uint32_t* flagsK,
                            double* cal) {
  hipLaunchKernelGGL(median_calibrate_kernel, dim3(1), dim3(256), 0, ctx->stream, medK, pred, K, flagsK, cal);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_median_select(plaidhip_ctx* ctx, const unsigned long long* cand, const uint32_t* cnt, int32_t n, int32_t nslice,
                         int32_t capc, int32_t m, const double* cal, int ignore_zero, const uint32_t* flags, double* med,
                         int32_t* status) {
  if (n == 0) return PLAIDHIP_OK;
  const int cap = ctx->num_cu * 16;
  hipLaunchKernelGGL(median_select_kernel, dim3(n < cap ? n : cap), dim3(64), 0, ctx->stream, cand,
                     reinterpret_cast<const uint4*>(cnt), n, nslice, capc, m, cal, ignore_zero, flags, med, status);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_col_medians(plaidhip_ctx* ctx, const double* S, int64_t lds, int32_t m, int32_t n,
                       int ignore_zero, const uint32_t* flags, double* med, const int32_t* status) {
  if (n == 0) return PLAIDHIP_OK;
  // register-resident radix selection up to 6,144 values per column, streaming beyond (switch-over measured, DESIGN.md
  // 4.3).  PLAIDHIP_MEDIAN_KERNEL=stream sends every m to the streaming kernel in the tools/ build (make diag), which is
  // how the switch-over is measured again; any other value is ignored.
#ifdef PLAIDHIP_DIAG
  static const char* force = getenv("PLAIDHIP_MEDIAN_KERNEL");
  const bool force_stream = force != nullptr && strcmp(force, "stream") == 0;
#else
  constexpr bool force_stream = false;
#endif
  if (m <= 6144 && !force_stream) {
    // (the kernel reads its first ITEMS - 16 rows of 64 values without a bound: the class follows from m, here and only here)
    const int cls = m <= 1024 ? 16 : ((m + 1023) / 1024) * 16;
    switch (cls) {
      case 16: launch_wave<16, 4>(ctx, S, lds, m, n, ignore_zero, flags, med); break;
      case 32: launch_wave<32, 4>(ctx, S, lds, m, n, ignore_zero, flags, med); break;
      case 48: launch_wave<48, 3>(ctx, S, lds, m, n, ignore_zero, flags, med); break;
      case 64: launch_wave<64, 3>(ctx, S, lds, m, n, ignore_zero, flags, med); break;
      case 80: launch_wave<80, 2>(ctx, S, lds, m, n, ignore_zero, flags, med); break;
      default: launch_wave<96, 2>(ctx, S, lds, m, n, ignore_zero, flags, med); break;
    }
  } else {
#ifdef PLAIDHIP_DIAG
    static const char* wg_env = getenv("PLAIDHIP_STREAM_WGS");
    const int cap = ctx->num_cu * (wg_env ? atoi(wg_env) : 8);
#else
    const int cap = ctx->num_cu * 8;                      // 8 workgroups x 4 wavefronts per CU
#endif
    const int need = (n + 3) / 4;
    // candidate lists of the sampled start: a quarter of a column per wavefront in flight (the sample interval holds
    // about a sixth; a list that overflows is not used and the column is swept a second time instead)
    const int grid = need < cap ? need : cap;
    const int32_t ccap = m > 4 * 1024 ? ((m / 4 + 63) & ~63) : 0;
    unsigned long long* cand = nullptr;
    if (ccap > 0) {
      const int rc = ensure_workspace(ctx, (size_t)grid * 4 * (size_t)ccap * 8);
      if (rc != PLAIDHIP_OK) return rc;
      cand = reinterpret_cast<unsigned long long*>(ctx->ws);
    }
    // sample size: 512 values up to 32,768 sets, 1,024 beyond (a narrower bracket: 12.5 % instead of 17.6 % of the column
    // become candidates; measured on 8,192 columns, one box: 50k sets 0.975 -> 0.89 ms, 20k equal, 8k 0.160 -> 0.177: the two
    // bracket selections cost 30 us per column at 512 values and 50 us at 1,024; 2,048 values lose everywhere)
#ifdef PLAIDHIP_DIAG
    static const char* sc_env = getenv("PLAIDHIP_SAMPLE_CHUNKS");
    const int sc = sc_env ? atoi(sc_env) : (m > 32768 ? 16 : 8);
#else
    const int sc = m > 32768 ? 16 : 8;
#endif
    if (sc == 16)
      hipLaunchKernelGGL((col_medians_stream_kernel<1024, 16>), dim3(grid), dim3(256), 0, ctx->stream, S,
                         lds, m, n, ignore_zero, flags, med, cand, ccap, median_stamps(), status);
    else
      hipLaunchKernelGGL((col_medians_stream_kernel<1024, 8>), dim3(grid), dim3(256), 0, ctx->stream, S,
                         lds, m, n, ignore_zero, flags, med, cand, ccap, median_stamps(), status);
  }
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
