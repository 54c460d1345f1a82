// tools/ build only (make diag, -DPLAIDHIP_DIAG): the ablation arms, phase stamps and diagnostic launches of kernels_spmm.hip.
// The product library never sees this file: kernels_spmm.hip includes it, one numbered section at a time, inside
// `#ifdef PLAIDHIP_DIAG` and defines the plain form of the same macros in the `#else` branch beside the include -- the hot
// loops of the product read without any of this.  Every arm that changes what a kernel computes gives WRONG scores by design
// (it prices one pipe at a time); tools/bench_spmm.py --ablate N / --stamps drives them through plaidhip_debug_set_ablation.
#ifndef PH_DIAG_SECTION
#error "include through kernels_spmm.hip with PH_DIAG_SECTION set"
#endif
#if PH_DIAG_SECTION == 1
static int g_ablate = 0;
static unsigned long long* g_dbg = nullptr;
#endif
#if PH_DIAG_SECTION == 2
#define PH_COL_PF (ABLATE != 3)
#define PH_COL_STAMP (ABLATE == 4)
#define PH_COL_LDS_AT(o_) lds_at<ABLATE>(o_)
#define PH_COL_SYNTH_IDS (ABLATE == 2)
#endif
#if PH_DIAG_SECTION == 3
        const gptr_u8 ibase0 = ibase;
#endif
#if PH_DIAG_SECTION == 4   /* tools/ build only: ABL 2 = synthetic ids (no index stream), 6 = the same 2 KiB again (L1-resident) */
#define PLAIDHIP_LOADQ(rel)                                                                          \
  (ABL == 2 ? u32x4{lane_o | ((lane_o + 64u) << 16), (lane_o + 128u) | ((lane_o + 192u) << 16),       \
                    (lane_o + 256u) | ((lane_o + 320u) << 16), (lane_o + 384u) | ((lane_o + 448u + (rel)) << 16)} \
            : (ABL == 6 ? *(gptr_u32x4)(ibase0 + (int64_t)((rel) & 1) * 1024 + ioff)                   \
                        : *(gptr_u32x4)(ibase + (int64_t)(rel) * 1024 + ioff)))
#define PH_PAIR_PSTORE (ABL != 5 && ABL != 9)   /* 5: no partial-sum round trip between slices; 9: loads only (wrong scores) */
#define PH_PAIR_PLOAD (ABL != 5 && ABL != 8)    /* 8: stores only */
#define PH_PAIR_PSLOT(k_) (ABL == 10 ? ((k_) & 3) : (k_))   /* 10: a four-tile scratch per workgroup: always L2-resident */
#define PH_PAIR_PST_NT (ABL == 11 || ABL == 12)   /* 11: non-temporal partial stores and loads, 12: stores only, 13: loads only */
#define PH_PAIR_PLD_NT (ABL == 11 || ABL == 13 || ABL == 14)
#define PH_PAIR_PST_SC1 (ABL == 14 || ABL == 15)   /* 14: agent-scope (sc1) 8-byte stores + nt loads, 15: sc1 stores + sc1 loads */
#define PH_PAIR_PLD_SC1 (ABL == 15)
#define PH_PAIR_SST_SC1 (ABL == 16)   /* 16: score stores with agent scope (sc1: the lines do not stay in L2) */
#define PH_PAIR_META (ABL != 7)       /* 7: no per-tile metadata loads (wrong scores) */
#endif
#if PH_DIAG_SECTION == 5
#define PH_SC_ABL(k) (a.abl == (k) || (a.abl == 4 && ((k) == 1 || (k) == 2)))
#endif
#if PH_DIAG_SECTION == 6
#define PH_SC_STAMP(k)                                                                \
  do {                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                 \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();                        \
    __builtin_amdgcn_s_waitcnt(0xC07F);                                                \
    t_ph[k] += t_ - t_last;                                                            \
    t_last = t_;                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                 \
  } while (0)
#define PH_SC_STAMP_IDS(x) do { asm volatile("" : "+v"(x)); PH_SC_STAMP(5); } while (0)
#endif
#if PH_DIAG_SECTION == 7
  unsigned long long t_ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_last = __builtin_amdgcn_s_memtime();
#endif
#if PH_DIAG_SECTION == 8
  if (a.dbg != nullptr && (tid & 63) == 0)
    for (int k = 0; k < 8; ++k) a.dbg[((size_t)blockIdx.x * NW + wave) * 8 + k] = t_ph[k];
#endif
#if PH_DIAG_SECTION == 9
  a.dbg = g_dbg;
  a.abl = g_ablate > 100 ? g_ablate - 100 : 0;
#endif
#if PH_DIAG_SECTION == 10
  if (g_ablate == 4) {   // in-kernel stamps
    a.dbg = g_dbg;
    PH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&spmm_colpair_mixed<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    hipLaunchKernelGGL(spmm_colpair_mixed<true>, dim3(grid), dim3(1024), smem, ctx->stream, a);
  } else
#endif
#if PH_DIAG_SECTION == 11
  if (g_ablate == 4) {   // in-kernel stamps
    qa.s.dbg = g_dbg;
    PH_FULL_LDS(ctx, (&spmm_colquad_u16<true>));
    hipLaunchKernelGGL((spmm_colquad_u16<true>), dim3(grid), dim3(1024), smem, ctx->stream, qa);
  } else
#endif
#if PH_DIAG_SECTION == 12
#define PH_PAIR_ABL_ARM(N)                                                                               \
  else if (g_ablate == N) {   /* tools/ only, wrong scores: 2 no index loads, 5 no partial-sum round trip, 6 index loads */ \
    a.dbg = g_dbg;            /* always hit L1, 7 no tile metadata, 8 partial stores only, 9 partial loads only, 10 a   */ \
    PH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&spmm_colpair_f64<true, N>),               /* four-tile scratch */ \
                               hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));                   \
    hipLaunchKernelGGL((spmm_colpair_f64<true, N>), dim3(grid), dim3(1024), smem, ctx->stream, a);        \
  }
  PH_PAIR_ABL_ARM(2) PH_PAIR_ABL_ARM(5) PH_PAIR_ABL_ARM(6) PH_PAIR_ABL_ARM(7) PH_PAIR_ABL_ARM(8) PH_PAIR_ABL_ARM(9) PH_PAIR_ABL_ARM(10) PH_PAIR_ABL_ARM(11) PH_PAIR_ABL_ARM(12) PH_PAIR_ABL_ARM(13) PH_PAIR_ABL_ARM(14) PH_PAIR_ABL_ARM(15) PH_PAIR_ABL_ARM(16)
#undef PH_PAIR_ABL_ARM
  else if (g_ablate == 4) {   // in-kernel stamps (tools/ only)
    a.dbg = g_dbg;
    PH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&spmm_colpair_f64<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    hipLaunchKernelGGL(spmm_colpair_f64<true>, dim3(grid), dim3(1024), smem, ctx->stream, a);
  }
#endif
#if PH_DIAG_SECTION == 13
void debug_set_ablation(int mode, void* dbg) { g_ablate = mode; g_dbg = static_cast<unsigned long long*>(dbg); }
#endif
#if PH_DIAG_SECTION == 14
  if constexpr (!CSC_X && BLOCK >= 512) {
    if (g_ablate != 0) {   // diagnostic kernels
      a.dbg = g_dbg;
#define PLAIDHIP_ABL(N)                                                                              \
  if (g_ablate == N) {                                                                                \
    PH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&spmm_colgather_f64<false, BLOCK, N>),   \
                               hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));               \
    hipLaunchKernelGGL((spmm_colgather_f64<false, BLOCK, N>), dim3(grid), dim3(BLOCK), smem, ctx->stream, a); \
  }
      PLAIDHIP_ABL(1) PLAIDHIP_ABL(2) PLAIDHIP_ABL(3) PLAIDHIP_ABL(4)
#undef PLAIDHIP_ABL
      PH_HIP(hipGetLastError());
      return PLAIDHIP_OK;
    }
  }
#endif
#if PH_DIAG_SECTION == 15
    else if (g_ablate == 4) {   // in-kernel stamps of the 768-thread register-partial form (tools/ only)
      a.dbg = g_dbg;
      PH_FULL_LDS(ctx, (&spmm_colpair_f64<true, 0, false, false, false, kPairRegWaves * 64, true, true>));
      hipLaunchKernelGGL((spmm_colpair_f64<true, 0, false, false, false, kPairRegWaves * 64, true, true>), dim3(grid),
                         dim3(kPairRegWaves * 64), smem, ctx->stream, a);
    }
#endif
