// Internal declarations shared by the C-ABI translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../../include/plaidhip.h"

namespace plaidhip {

// LDS budget of one CU on gfx950: 160 KiB, one workgroup may own all of it.
constexpr int kLdsBytes = 160 * 1024;
// The LDS-resident column kernels keep one 8-byte entry per gene plus kPadSlots zero
// entries that padded index slots point at.
constexpr int kPadSlots = 32;
constexpr int kMaxLdsGenes = kLdsBytes / 8 - kPadSlots;  // 20448
// bitonic sort in LDS: 8-byte keys
constexpr int kMaxLdsKeys = kLdsBytes / 8;               // 20480
// pair kernel: 16-byte entries (two sample columns), 16 zero entries behind them
constexpr int kPadSlotsPair = 16;
constexpr int kMaxLdsGenesPair = kLdsBytes / 16 - kPadSlotsPair;   // 10224
// pair plans of more than one gene slice whose tiles can be dealt to 12 wavefronts, at most 8 each (<= 6,144 sets): the
// pair kernel runs them at 768 threads (3 wavefronts per SIMD: 168 vector registers each) and keeps a lane's partial sums of
// the slices before in registers, one pair per tile
constexpr int kPairRegWaves = 12;
constexpr int kPairRegPartials = 8;
constexpr int kMaxPairSlices = 8;
// scatter kernel (sparse X): fp64 accumulators of one chunk of gene sets in LDS
constexpr int kScatterTrash = 64;                      // accumulators behind a chunk that padded id slots add into
// threads per workgroup of the scatter kernel (512: two workgroups per CU, measured slower; the -D override is for the
// A/B builds of tools/: make variant NAME=b512 DEFS=-DPLAIDHIP_SCATTER_BLOCK=512)
#ifndef PLAIDHIP_SCATTER_BLOCK
#define PLAIDHIP_SCATTER_BLOCK 1024
#endif
constexpr int kScatterBlock = PLAIDHIP_SCATTER_BLOCK;
// further id segments (genes in more than 128 sets of a chunk) whose loads ride the scatter walk's static pipeline per
// wavefront and item; a wavefront with more of them fetches the rest group by group (A/B builds: -DPLAIDHIP_SCATTER_HE=8)
// groups of 16 first-segment loads a wavefront requests before it applies the first one: 2 (3, round 5's depth, puts 960
// requests into the CU's in-order memory pipe at the start of an item and the youngest wavefronts' first ids behind all of
// them: +2.5 % at 16,384 x 50,000, profiles/r06h_scatter_depth_ab.txt; A/B builds: -DPLAIDHIP_SCATTER_DEPTH=3)
#ifndef PLAIDHIP_SCATTER_DEPTH
#define PLAIDHIP_SCATTER_DEPTH 2
#endif
#ifndef PLAIDHIP_SCATTER_HE
#define PLAIDHIP_SCATTER_HE 12
#endif
// sets per chunk: 17 passes of the workgroup's 1,024 threads over the accumulators (136 KiB of the 160; the chunk epilogue
// keeps one 16-byte factor pair per pass in registers, and 20 of them left none for anything else: 50,000 sets are three
// chunks either way)
constexpr int kScatterChunk = 17 * kScatterBlock;

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what, const char* file, int line);
// Every `int plaidhip_*` entry point is a function-try-block that ends here: a C++ exception (std::bad_alloc from a host-side
// plan, std::system_error from a thread the system refuses) becomes an error code and a message -- it never unwinds into
// the caller's C stack (R's, ctypes').  Exceptions inside the library's own worker threads are not covered by this.
inline int on_exception() noexcept {
  try {
    throw;
  } catch (const std::bad_alloc&) {
    set_error("out of host memory");
    return PLAIDHIP_ENOMEM;
  } catch (const std::exception& e) {
    set_error("unexpected C++ exception: %s", e.what());
    return PLAIDHIP_EHIP;
  } catch (...) {
    set_error("unexpected C++ exception");
    return PLAIDHIP_EHIP;
  }
}

#define PH_HIP(call)                                                              \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) return ::plaidhip::hip_fail(e_, #call, __FILE__, __LINE__); \
  } while (0)

#define PH_REQUIRE(cond, ...)                 \
  do {                                        \
    if (!(cond)) {                            \
      ::plaidhip::set_error(__VA_ARGS__);     \
      return PLAIDHIP_EINVAL;                 \
    }                                         \
  } while (0)

}  // namespace plaidhip

struct plaidhip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // growable scratch
  void* ws = nullptr;
  size_t ws_bytes = 0;
  int num_cu = 256;
  // prepared gene-set collections of the host-level entry points (api.cpp: acquire_geneset), most recent last
  struct cached_geneset { uint64_t hash, hash2; int32_t g, m; struct plaidhip_geneset* gs; };
  std::vector<cached_geneset> gs_cache;
  int precision = 0;   // PLAIDHIP_PRECISION_*: 0 fp64 throughout (default), 1 fp32 operand staging in the dense SpMM
  // plaidhip_set_option (include/plaidhip.h: enum plaidhip_option)
  int opt_dense_kernel = 0;    // 0 auto | 1 one-column | 2 pair wherever it applies | 3 dense bf16x3 GEMM on MFMA | 4 auto, pair kernel in its scratch form
  int opt_sparse_kernel = 0;   // 0 auto | 1 scatter | 2 gather
  int opt_nt_store = -1;       // -1 auto | 0 | 1
  int opt_ranks_f32 = 2;       // rank inputs: 0 fp64 kernels | 1 fp32 staging | 2 u16 staging, integer sums (all exact)
  int opt_rank_kernel = 0;     // 0 auto | 1 sorting network | 2 bucket ranker
  int opt_scatter_fixed = 1;   // scatter kernel: u64 fixed-point accumulators for inputs declared bounded (rank weights)
  int opt_scatter_order = 1;   // scatter kernel: 0 (column, chunk) | 1 (chunk, column) item order
  int opt_fused_medians = 0;   // medians selected inside the sparse crossprod: 0 by size (>= 1e9 scores) | 1 whenever possible | 2 never
  double* d_sel = nullptr;        // {0 or -1, max, smallest > 0, largest column sum or +inf} of the stored values of a sparse X (scatter kernel's choice of accumulators)
                                  // (a 128-byte block: d_spec at byte 64; bytes 96..127 hold the EMPTY median bracket {0, -1, 0, 0} a
                                  //  calibration launch of the dense fused crossprod classifies against, written once at plaidhip_init)
  uint32_t* d_spec = nullptr;     // speculative launches (u16 quad kernel): [0] generation that saw a non-rank, [1..3] its private flag words
  uint32_t spec_gen = 0;          // generation of the last speculative launch (host side)
  // medians selected inside the last sparse crossprod launch (launch_spmm_csc_fused_f64): what plaidhip_dev_col_medians_resume
  // needs to finish them.  The scratch holds, per sample column: the predicted mean, the status word, per (chunk, wavefront)
  // four counts and a slice of candidate scores.
  void* fmed_buf = nullptr;
  size_t fmed_bytes = 0;
  uint64_t fmed_gen = 0;          // generation counter of the fused launches: the token a caller hands back to resume
  struct fused_medians {
    bool valid = false;
    uint64_t token = 0;           // generation of the launch that left this state (0: none)
    const double* S = nullptr;
    int64_t lds = 0;
    int32_t m = 0, n = 0, nslice = 0, capc = 0;
    double* pred = nullptr;
    double* cal = nullptr;
    uint32_t* cnt = nullptr;
    unsigned long long* cand = nullptr;
    int32_t* status = nullptr;
  } fmed;
  void* tie_scratch = nullptr;    // ties.method first / last / dense: two scratch columns per column (kernels_rank.hip)
  size_t tie_scratch_bytes = 0;
  void* rank_scratch = nullptr;   // value-partitioned ranking of columns beyond the LDS (kernels_rank.hip), grown on demand
  size_t rank_scratch_bytes = 0;
  // test hook (plaidhip_debug_rank_fallbacks): the device words that count the columns the last launch handed to the sorting
  // network: [0] launch_ranks (the bucket ranker; lives in ws), [1] launch_colranks_partitioned (lives in rank_scratch);
  // nullptr: that launcher has not run with a hand-over list, or its buffer has been released since
  const int32_t* rank_fb_count[2] = {nullptr, nullptr};
  void* kcdf_table = nullptr;     // replaid.gsva.exact, rowtf "gauss": the table of Phi and a counter word (kernels_kcdf.hip), built on first use
  int debug_fail_crossprod = 0;   // test hook (plaidhip_debug_sharded_on_one_device): this context's shard fails in the crossprod phase
  // pinned staging of the pipelined host uploads (multi.cpp): kFeeders feeder threads x 2 buffers, their streams
  static constexpr int kFeeders = 4;
  void* pin[kFeeders][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
  size_t pin_bytes = 0;
  hipStream_t copy_stream[kFeeders] = {nullptr, nullptr, nullptr, nullptr};
  // device buffers of the host-level pipelines, kept between calls (an R session scores matrix after matrix of the
  // same shape; hipMalloc + hipFree of gigabytes per call cost milliseconds and a device synchronisation)
  static constexpr int kHostBufs = 6;
  void* hbuf[kHostBufs] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t hbuf_bytes[kHostBufs] = {0, 0, 0, 0, 0, 0};
};

// Prepared membership (built by geneset.cpp, see the header comment there).
//   tile_idx : u16 gene ids, layout [chunk][lane 0..63][8]  (a chunk = 8 gather steps; one
//              16-byte load per lane per chunk, 1 KiB per wave, coalesced).  Idle slots hold
//              g + r (r < kPadSlots) and read a zero entry behind the column in LDS.
//   wave_chunk_off[w] .. [w+1] : the contiguous chunk stream of wavefront w of the workgroup
//   wave_tile_off[w]  .. [w+1] : its tiles, as entries of wtile_end / wtile_id
//   wtile_end[k]      : absolute chunk index one past tile k's last chunk
//   meta_j/meta_w/meta_k[k*64 + lane] : per lane of wave-stream tile k: set id (or -1),
//                       1/(1e-8 + size) and size -- everything the epilogue needs, one
//                       coalesced load each, fetched a tile ahead
// one gene slice (g0 .. g0+gs) of the prepared membership; g <= kMaxLdsGenes needs one slice
struct plaidhip_slice {
  int32_t g0 = 0, gs = 0;
  int32_t waves = 0;           // wavefronts per workgroup the plan was built for
  int64_t chunks = 0;          // 8-step chunks over all tiles of this slice
  uint16_t* d_tile_idx = nullptr;
  int32_t* d_wave_chunk_off = nullptr;
  int32_t* d_wave_tile_off = nullptr;
  int32_t* d_wtile_end = nullptr;
  int32_t* d_meta_j = nullptr;
  double* d_meta_w = nullptr;
  double* d_meta_k = nullptr;
};

// pair plan: gene slices of <= kMaxLdsGenesPair genes; tiles, tile->wave assignment and the
// per-lane metadata are shared by all slices (see geneset.cpp)
struct plaidhip_pair_slice {
  int32_t g0 = 0, gs = 0;
  uint16_t* d_tile_idx = nullptr;
  int32_t* d_wave_chunk_off = nullptr;
  int32_t* d_wtile_end = nullptr;
};
// what the kernel reads per slice (device array, scalar loads)
struct plaidhip_pair_slice_dev {
  const uint16_t* tile_idx;
  const int32_t* wave_chunk_off;
  const int32_t* wtile_end;
  int32_t g0, gs;
};
struct plaidhip_pair_plan {
  int32_t waves = 0;                           // wavefronts that have tiles (the arrays are laid out for 16 either way)
  bool regp = false;                           // built for kPairRegWaves wavefronts x <= kPairRegPartials tiles (see above)
  int32_t ktiles = 0;                          // wave-stream tiles (all waves)
  int64_t chunks = 0;
  std::vector<plaidhip_pair_slice> slices;
  plaidhip_pair_slice_dev* d_slices = nullptr;
  // partial sums between gene slices: [workgroup][wave-stream tile + 1][lane] x {A, B}
  // (a regp plan has none until PLAIDHIP_OPT_SPMM_DENSE_KERNEL = 4 pins the scratch form: alloc_pair_partial)
  double* d_partial = nullptr;
  int32_t partial_wgs = 0;
  int32_t* d_wave_tile_off = nullptr;
  int32_t* d_meta_j = nullptr;
  double* d_meta_w = nullptr;
  double* d_meta_k = nullptr;
  // a regp plan is planned with flex steps (geneset.cpp, plan_tile_flex): [slice][wavefront 0..15][lane][the wavefront's
  // tile 0..7] one byte {source lane, is-host, has-host}; only the FLEX forms of the pair kernel walk such a plan
  uint8_t* d_flex = nullptr;
};

// Scatter plan (sparse X): G transposed, gene-major.  The sets are dealt to `nch` chunks of `ch` accumulator slots (the
// LDS accumulators of one chunk) in BLOCKS of kScatterBlock consecutive sets, block b to chunk b % nch at slots
// (b / nch) * kScatterBlock ..: a collection straight from gmt2mat() has its sets in decreasing size (R/gmt-utils.R:25), and
// chunks of consecutive sets gave the first chunk 72 % of all memberships -- two to three id segments per gene there, one
// fifth-full segment in the last chunk, 4.35 (value, chunk) pairs per stored value at config 3 instead of the 3.3 the
// interleaved deal needs (every chunk sees the whole range of set sizes).  A chunk pass of the 1,024 threads still writes
// 1,024 consecutive scores.  The sets of gene i inside chunk c are stored as whole segments
// of 128 u16 slot ids (a dword = two ids per lane; padding: a trash accumulator behind the chunk): segments seg[c*g + i] ..
// seg[c*g + i + 1] - 1 of d_ids.  (seg has nch*g + 1 entries, chunk-major, so the ranges of
// consecutive (chunk, gene) pairs are contiguous.)
#if defined(__HIPCC__)
#define PH_HD __host__ __device__
#else
#define PH_HD
#endif
PH_HD inline int32_t scatter_chunk_of(int32_t j, int32_t nch) { return (j / plaidhip::kScatterBlock) % nch; }
PH_HD inline int32_t scatter_slot_of(int32_t j, int32_t nch) {
  return ((j / plaidhip::kScatterBlock) / nch) * plaidhip::kScatterBlock + j % plaidhip::kScatterBlock;
}
PH_HD inline int32_t scatter_set_of(int32_t chunk, int32_t slot, int32_t nch) {
  return ((slot / plaidhip::kScatterBlock) * nch + chunk) * plaidhip::kScatterBlock + slot % plaidhip::kScatterBlock;
}
struct plaidhip_scatter_plan {
  int32_t ch = 0, nch = 0;
  int32_t kbits = 0;           // bits of the largest set size + 1: headroom of the fixed-point sums
  int64_t nseg = 0;
  int32_t* d_seg = nullptr;
  uint16_t* d_ids = nullptr;
  double* d_w = nullptr;   // per set 1/(1e-8 + size)
  double* d_k = nullptr;   // per set size
  double* d_kw = nullptr;  // {size x weight, weight} per set, m entries for STAT_MEAN then m for STAT_SUM: one 16-byte load per set in the scatter kernel's epilogue
  double* d_u = nullptr;   // per gene (1 / m) sum of the weights of its sets: g entries for STAT_MEAN, then g for STAT_SUM
  double kappa[2] = {0.0, 0.0};   // (1 / m) sum_j size_j weight_j per statistic
#ifdef PLAIDHIP_KEEP_HOST_PLANS
  std::vector<int32_t> h_seg;    // host-only tools build (tools/plan_probe): the uploaded plan, for its checker
  std::vector<uint16_t> h_ids;
#endif
};

struct plaidhip_geneset {
  plaidhip_ctx* ctx = nullptr;
  int32_t g = 0, m = 0;
  int64_t z = 0;
  int32_t tiles = 0;
  int64_t chunks = 0;          // total over slices
  std::vector<plaidhip_slice> slices;   // the column is consumed slice by slice when g > kMaxLdsGenes
  plaidhip_pair_plan pair;              // dense-X kernel: two columns per pass
  plaidhip_scatter_plan scatter;        // sparse-X kernel: nonzeros are scattered into per-set LDS accumulators
  bool rows_in_order = false;           // the sets came sorted by decreasing size: a tile's lanes are neighbouring rows of S
  // MFMA backend (opt-in, kernels_mfma.hip): the pattern is kept on the host and the dense bf16 sets x genes matrix
  // is built on first use
  std::vector<int32_t> h_Gp, h_Gi;
  void* d_dense_g = nullptr;
  int32_t dense_gk = 0;
};

namespace plaidhip {

int ensure_workspace(plaidhip_ctx* ctx, size_t bytes);
// RAII for the device buffers of one host-level call
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) hipFree(p); }
  int alloc(size_t bytes);
  template <typename T> T* as() { return static_cast<T*>(p); }
};
// slot `k` of the context's persistent host-pipeline buffers, grown to at least `bytes` (contents undefined)
int ctx_buffer(plaidhip_ctx* ctx, int k, size_t bytes, void** out);
// host-level helpers shared by api.cpp and multi.cpp
int acquire_geneset(plaidhip_ctx* ctx, int32_t g, int32_t m, const int32_t* Gp, const int32_t* Gi, plaidhip_geneset** out);
int check_host_csc(const int32_t* Xp, const int32_t* Xi, int32_t g, int32_t n);
int check_host_common(const void* G_p, int32_t g, int32_t n, int32_t m);
const char* last_error_cstr();
// A result's way home into the caller's pageable buffer (multi.cpp).  R hands over FRESH memory (allocMatrix -> malloc ->
// mmap): every page faults on its first write, inside the device-to-host copy -- 4.9 GB of scores took 309 ms instead of
// 92 (tools/ubench/d2h_fresh.cpp).  prepare() asks for transparent huge pages on the range (madvise; a hint, ignored where
// the system has them off) and starts threads that touch it chunk by chunk; copy() issues the chunk copies on the context's
// stream as their pages appear and returns when the last one is enqueued (the pageable copies themselves are synchronous
// in the runtime).  Small results are one plain copy.  The destination's previous contents are destroyed from prepare() on.
class HomeBuffer {
 public:
  HomeBuffer() = default;
  HomeBuffer(const HomeBuffer&) = delete;
  HomeBuffer& operator=(const HomeBuffer&) = delete;
  ~HomeBuffer() { finish(); }
  void prepare(void* dst, size_t bytes);
  int copy(plaidhip_ctx* ctx, const void* src_dev);   // (prepare() first; copies `bytes` of it)
  void finish();                                      // joins the touch threads (idempotent)
 private:
  struct State;
  State* st_ = nullptr;
};
// prepare + copy + finish
int copy_home(plaidhip_ctx* ctx, void* dst, const void* src_dev, size_t bytes);
// the other direction (multi.cpp): `cols` rows of row_bytes bytes from pageable host memory to device rows ldd_bytes apart
// (a flat array: row_bytes = ldd_bytes = 1, cols = bytes), through the context's pinned staging ring; stream-ordered for
// consumers on the context's stream, returns when the host side is done with `src`
int upload_host(plaidhip_ctx* ctx, void* dst, size_t ldd_bytes, const void* src, size_t row_bytes, int64_t cols);
// opt a kernel into the full 160 KiB of dynamic LDS, once per (kernel, device)
int allow_full_lds(plaidhip_ctx* ctx, const void* kernel, std::atomic<uint32_t>* done_mask);
#define PH_FULL_LDS(ctx, kernel)                                                          \
  do {                                                                                    \
    static std::atomic<uint32_t> mask_{0};   /* per call site; bit = device ordinal; host threads of several devices meet here */ \
    int rc_l_ = ::plaidhip::allow_full_lds((ctx), reinterpret_cast<const void*>(kernel), &mask_); \
    if (rc_l_ != PLAIDHIP_OK) return rc_l_;                                               \
  } while (0)
int spmm_block_for_genes(int32_t g);   // workgroup size of the column-resident SpMM kernel

// kernels_stats.hip / stats.cpp  (plaid.test)
int launch_row_group_ssd(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const int32_t* d_y,
                         const double* d_mean, double* d_ssd, double* ws);
int launch_row_group_moments(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n,
                             const int32_t* d_y, int64_t n0, int64_t n1, double* d_mean, double* d_ssd,
                             double* ws);
// sample-sharded replaid.gsva (multi.cpp): the block partials of launch_row_group_moments over one shard, their group-0
// reduction continued from a seed (shards chained in column order reproduce the one-shard sums bit for bit), and the z
// transform of a shard whose moments were taken over n_total samples
int launch_row_group_partials(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const int32_t* d_y,
                              const double* d_mean, double* ws);
int launch_reduce_blocks_seeded(plaidhip_ctx* ctx, const double* ws, int32_t rows, int32_t n, const double* d_seed,
                                double* d_out);
int launch_row_ztransform_shard(plaidhip_ctx* ctx, double* A, int64_t ld, int32_t rows, int32_t ncols, int32_t n_total,
                                const double* d_mean, const double* d_ssd);
// sample-sharded plaid.test (multi.cpp): launch_row_group_partials over a raw score shard with normalize_medians' shift
// (S - d_med[c]) + add applied on load (d_med null: no shift); the shifted scores are not written
int launch_row_group_shifted_partials(plaidhip_ctx* ctx, const double* S, int64_t ld, int32_t rows, int32_t n,
                                      const int32_t* d_y, const double* d_med, double add, const double* d_mean,
                                      double* ws);
int launch_transpose_f64(plaidhip_ctx* ctx, const double* A, int64_t lda, int32_t rows, int32_t cols, double* B,
                         int64_t ldb);
int launch_fold_change(plaidhip_ctx* ctx, const double* d_mean, int32_t rows, int64_t ld2, double* d_F);
int64_t row_group_ws_doubles(int32_t rows, int32_t n);
// kernels_contrasts.hip (plaid.test.contrasts): the same moments for C label columns per read of the matrix.  d_Y: n x C
// labels (0, 1, else excluded), leading dimension ldy; d_masks: contrast_mask_bytes(n, C) bytes, filled by
// launch_contrast_masks; ws: row_contrast_ws_doubles(rows, n, C) doubles of block partials [nblk][C][2][rows]; d_mean (null:
// sums; else sums of squared deviations from it), d_seed, d_out: [C][2][rows]
int64_t row_contrast_ws_doubles(int32_t rows, int32_t n, int32_t C);
int64_t contrast_mask_bytes(int32_t n, int32_t C);
int launch_contrast_masks(plaidhip_ctx* ctx, const int32_t* d_Y, int64_t ldy, int32_t n, int32_t C, void* d_masks);
int launch_row_contrast_partials(plaidhip_ctx* ctx, const double* S, int64_t ld, int32_t rows, int32_t n,
                                 const void* d_masks, int32_t C, const double* d_med, double add, const double* d_mean,
                                 double* ws);
int launch_reduce_blocks_flat(plaidhip_ctx* ctx, const double* ws, int64_t len, int32_t n, const double* d_seed,
                              double* d_out);
int launch_fold_change_contrasts(plaidhip_ctx* ctx, const double* d_mean, int32_t rows, int32_t C, int64_t ld2, double* d_F);
// kernels_lmfit.hip (plaid.limma): the weighted row sums of W = nfit (p + 1) weight columns (fit f: p columns of Q_f, then
// use / n_f) per read of the matrix in tiles of PLAIDHIP_LIMMA_TILE, and the residual sums of squares at the reduced effects.
// d_Q: n x p x nfit, d_use: n x nfit int8 or null, d_invn: nfit; d_masks / d_wt: lmfit_mask_bytes / lmfit_weight_bytes bytes,
// filled by launch_lmfit_masks; ws: row_design_ws_doubles(rows, n, W or nfit) doubles of block partials [nblk][cols][rows],
// reduced by launch_reduce_blocks_flat; d_E: [W][rows]
int64_t lmfit_tiles(int64_t W);
int64_t row_design_ws_doubles(int32_t rows, int32_t n, int64_t cols);
int64_t lmfit_mask_bytes(int32_t n, int64_t W);
int64_t lmfit_weight_bytes(int32_t n, int64_t W);
int launch_lmfit_masks(plaidhip_ctx* ctx, const double* d_Q, const int8_t* d_use, const double* d_invn, int32_t n, int32_t p,
                       int32_t nfit, void* d_masks, double* d_wt);
int launch_row_design_effects(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const void* d_masks,
                              const double* d_wt, int32_t W, double* ws, bool na = false);
int launch_row_design_rss(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* d_Q,
                          const void* d_masks, int32_t p, int32_t nfit, const double* d_E, double* ws, bool na = false);
// kernels_lmfit_w.hip (plaid.limma with weights, plaidhip_limma_w): fit f has lmfit_w_columns(p) = p (p + 1) / 2 + p + 1 weight
// columns (the products q_ck q_cl, Q_f's columns, 1 / n_f); d_masks / d_wt: lmfit_mask_bytes / lmfit_weight_bytes of n and W =
// nfit lmfit_w_columns(p), filled by launch_lmfit_w_table.  d_Wt: rows x n with A's leading dimension, or null; d_aw: n, or
// null.  _w_sums: ws [nblk][W][rows]; _w_counts: ws [nblk][2 nfit + 1][rows] (live, the mean's select, then the row's NaN);
// _w_solve: from the reduced sums d_S and counts d_cnt to d_G [nfit (p + 1)][rows], d_drow [nfit][rows], d_urow [nfit q][rows];
// _w_rss: ws [nblk][nfit][rows] at d_G.  p <= PLAIDHIP_LIMMA_NA_MAX_COEF.
int64_t lmfit_w_columns(int32_t p);
int launch_lmfit_w_table(plaidhip_ctx* ctx, const double* d_Q, const int8_t* d_use, const double* d_invn, int32_t n, int32_t p,
                         int32_t nfit, void* d_masks, double* d_wt);
int launch_row_design_w_sums(plaidhip_ctx* ctx, const double* A, const double* d_Wt, const double* d_aw, int64_t ld, int32_t rows,
                             int32_t n, const void* d_masks, const double* d_wt, int32_t p, int32_t nfit, double* ws);
int launch_lmfit_w_counts(plaidhip_ctx* ctx, const double* A, const double* d_Wt, const double* d_aw, int64_t ld, int32_t rows,
                          int32_t n, const int8_t* d_use, int32_t nfit, double* ws);
int launch_lmfit_w_solve(plaidhip_ctx* ctx, const double* d_S, const double* d_cnt, const double* d_v, const double* d_nf,
                         int32_t rows, int32_t n, int32_t p, int32_t nfit, int32_t q, double max_na, double* d_G, double* d_drow,
                         double* d_urow);
int launch_row_design_w_rss(plaidhip_ctx* ctx, const double* A, const double* d_Wt, const double* d_aw, int64_t ld, int32_t rows,
                            int32_t n, const double* d_Q, const void* d_masks, int32_t p, int32_t nfit, const double* d_G,
                            double* ws);
// kernels_voom.hip (plaid.voom): the check with the column sums (d_bad: one zeroed word), the row sums' block partials [nblk][rows],
// the log-CPM map, and the weights pass from the effects d_Eff [p + 1][rows], Q (n x p), the offsets (n) and nk knots
int launch_voom_check(plaidhip_ctx* ctx, const double* X, int64_t ld, int32_t rows, int32_t n, double* d_colsum, uint32_t* d_bad);
int launch_voom_rowsum(plaidhip_ctx* ctx, const double* X, int64_t ld, int32_t rows, int32_t n, double* part);
int launch_voom_logcpm(plaidhip_ctx* ctx, const double* X, int64_t ld, int32_t rows, int32_t n, const double* d_lib, double* E,
                       int64_t lde);
int launch_voom_weights(plaidhip_ctx* ctx, const double* d_Q, const double* d_off, int32_t n, int32_t p, const double* d_Eff,
                        int32_t rows, const double* d_kx, const double* d_ky, int32_t nk, double* W, int64_t ldw);
// na = "fit" (plaidhip_limma_na): `na` above extends the select by x == x.  The count pass: cnt[b][r] = the NaN of row r in
// column block b of 128 (d_off null; nblk x rows), then d_list[d_off[b][r] ..] = their columns (d_off: the exclusive prefix
// sums of cnt, row by row and block by block within a row, so a row's columns lie together and ascend).
// launch_lmfit_nan_pairs: the NaN of every (fit, row) inside the fit's used samples from the rows' lists (d_off: rows + 1
// row offsets), cnt [nfit][rows].  launch_lmfit_na_solve: Gram and solve over a work list of npairs (row, fit) pairs
// (lmfit_na.h): d_E [W][rows] changed in place, d_u npairs x q, d_ok npairs.  p <= PLAIDHIP_LIMMA_NA_MAX_COEF.
int launch_lmfit_nan_rows(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const int64_t* d_off,
                          int32_t* d_cnt, int32_t* d_list);
int launch_lmfit_nan_pairs(plaidhip_ctx* ctx, const int64_t* d_off, const int32_t* d_list, const int8_t* d_use, int32_t rows,
                           int32_t n, int32_t nfit, int32_t* d_cnt);
int launch_lmfit_na_solve(plaidhip_ctx* ctx, int64_t npairs, const int32_t* d_pairs, const int64_t* d_off, const int32_t* d_list,
                          const double* d_Q, const int8_t* d_use, int32_t n, int32_t p, int32_t q, const double* d_v,
                          const int32_t* d_nobs, const double* d_nf, int32_t rows, double* d_E, double* d_u, int32_t* d_ok);
// kernels_camera.hip (plaid.camera): Z (rows x n, leading dimension ldz) of fit f -- the residual chain of
// launch_row_design_rss with a store, scaled by the gene's sqrt(max(rss / d, 1e-8)) (camera.h) -- from d_E [W][rows] and
// d_rss [nfit][rows] of ALL samples; and the block partials part[block][set] (`stride` doubles from block to block) of the
// sums over the columns of T[set, c]^2 (T: m x n, leading dimension ldt), reduced by launch_reduce_blocks_flat
int launch_camera_residuals(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* d_Q,
                            const void* d_masks, int32_t p, int32_t f, const double* d_E, const double* d_rss, double d, double* Z,
                            int64_t ldz);
int64_t camera_sumsq_ws_doubles(int32_t n, int64_t len);
int launch_camera_sumsq(plaidhip_ctx* ctx, const double* T, int64_t ldt, int32_t m, int32_t n, double* part, int64_t stride);
// kernels_fry.hip (plaid.fry): camera's residual pass with the divisors d_cg [nfit][rows] read, not derived; the Gram matrix
// of the residual effects of sets s0 .. s0 + ns - 1 with its borders; the two eigenvalues of every M
int launch_fry_residuals(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* d_Q,
                         const void* d_masks, int32_t p, int32_t f, const double* d_E, const double* d_cg, double* Z,
                         int64_t ldz);
int launch_fry_gram(plaidhip_ctx* ctx, const double* d_rho, const double* d_e, int32_t d, int32_t q, const int32_t* d_Gp,
                    const int32_t* d_Gi, int32_t s0, int32_t ns, double* d_C, double* d_b, double* d_a, double* d_tr, double* d_fro);
int launch_fry_eigen(plaidhip_ctx* ctx, const double* d_M, const double* d_C, const double* d_b, const double* d_a, int32_t dim,
                     int32_t q, int64_t nprob, const int32_t* d_Dk, double* d_lam1, double* d_lamD, int32_t* d_sweeps,
                     int32_t* d_conv);
// kernels_roast.hip (plaid.roast): z of rotations k0 .. k1 - 1 (k0 a multiple of 64) as [tile from k0 / 64][rows][64]; the
// observed one-column tile; the four sides of every (set, rotation) and / or the counts against d_obs (mean50: d_sel and
// class_cnt[3] from roast.h's size classes)
struct RoastFit;
int launch_roast_rotate(plaidhip_ctx* ctx, const double* Rz, int64_t ldz, int32_t rows, int32_t n, const double* d_beta,
                        const double* d_rss, const double* d_W, int64_t ldw, int32_t k0, int32_t k1, RoastFit fit, int zscore,
                        double* Z);
int launch_roast_observed(plaidhip_ctx* ctx, const double* d_t, int32_t rows, double nu, int zscore, double* Z);
int launch_roast_stats(plaidhip_ctx* ctx, const double* Z, int32_t rows, const int32_t* d_Gp, const int32_t* d_Gi, int32_t m,
                       int set_statistic, int32_t k0, int32_t k1, int32_t nrot, const int32_t* d_sel, const int32_t* class_cnt,
                       double* d_stat, const double* d_obs, int32_t* d_cnt);
// kernels_romer.hip (plaid.romer): the keys of one chunk of rotated t ([tile][rows][64]) over the universe's index list as
// columns [nk][ldu]; from their average ranks the three int64 sides of every (set, rotation) and / or the counts against
// d_obs (mean, floormean: the rank crossprod on gs into S; mean50: d_sel and class_cnt[2] from romer.h's size classes)
int launch_romer_keys(plaidhip_ctx* ctx, const double* Z, int32_t rows, const int32_t* d_uidx, int32_t U, int64_t ldu,
                      int set_statistic, int32_t nk, double* Ka, double* Kb, double* Kc, uint32_t* d_flag);
int launch_romer_sides(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const double* Ra, const double* Rb, const double* Rc,
                       int64_t ldu, int32_t U, const int32_t* d_Gp, const int32_t* d_Gi, int32_t m, int set_statistic, int32_t nk,
                       int32_t kbase, int32_t nrot, const int32_t* d_sel, const int32_t* class_cnt, double* S, int64_t* d_stat,
                       const int64_t* d_obs, int32_t* d_cnt);
// stats.cpp (plaid.roast): W ((n + 1) x nrot row-major) of one fit from its thin Q
void roast_rotations(const double* Q, int32_t n, int32_t p, const int8_t* use, int32_t fit, int32_t nrot, uint64_t seed,
                     double* W);
// stats.cpp: eBayes and the tables of plaid.limma.  drow ([nfit][rows], NaN: the row is not fitted) and urow ([nfit q][rows])
// null: every row of fit f has nf[f] - p and u[f q + j] (plaidhip_limma_finish); hyper has hcols (4 or 5) values per fit
int limma_finish_rows(const char* what, int32_t rows, int32_t p, int32_t nfit, int32_t q, const double* E, const double* rss,
                      const int64_t* nf, const double* v, const double* u, const double* drow, const double* urow, double* out,
                      double* hyper, int hcols);
// stats.cpp: one design of plaid.limma (include/plaidhip.h: plaidhip_limma_design); what: the entry its messages name
int limma_design(const char* what, const double* D, int32_t n, int32_t p, const int8_t* use, const double* K, int32_t q,
                 int32_t fit, double* Q, double* R, double* v, double* u, int64_t* nf, double* Q2 = nullptr);
// stats.cpp: squeezeVar of one fit, shared by plaid.limma's tables and plaid.fry's divisors
struct LimmaPrior { double d0, s0, pool; int64_t nok; };
LimmaPrior limma_squeeze_fit(size_t R, double dfit, const double* dr, const double* rssf, double* s, double* po);
// stats.cpp (plaid.fry): the divisors c_g [nfit][rows] (NaN: the gene is outside the fit's universe); standardize as in
// include/plaidhip.h
void fry_divisors(int32_t rows, int32_t p, int32_t nfit, const double* rss, const int64_t* nf, int standardize, double* cg);
double t_two_sided_p(double t, double df);
double beta_upper(double x, double a, double b);
// kernels_csr.hip: the row view of a CSC matrix (replaid.gsva / plaid.test on a dgCMatrix).  All pointers are device
// pointers.  Transpose: Rp g + 1, Rx / Rj / perm Xp[n] entries each (Rj, perm optional), within a row ascending column
// order; *d_maxlen = the longest row.  Uses the context workspace.
int launch_csc_to_csr(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                      int32_t* Rp, int32_t* Rj, double* Rx, int32_t* perm, int32_t* d_maxlen);
// launch_row_group_moments over the CSR rows (implicit zeros counted); d_y null: every column in group 0 (Rj unused)
int launch_csr_row_group_moments(plaidhip_ctx* ctx, const int32_t* Rp, const int32_t* Rj, const double* Rx, int32_t rows,
                                 int32_t max_row_nnz, const int32_t* d_y, int64_t n0, int64_t n1, double* d_mean,
                                 double* d_ssd);
// #{x <= x_i} of every stored value (-> out[perm[p]], CSC order) and of each row's implicit zero (-> dflt[row]);
// Rrank: Rp[rows] doubles of scratch
int launch_csr_row_ecdf(plaidhip_ctx* ctx, const int32_t* Rp, const double* Rx, int32_t rows, int32_t n,
                        int32_t max_row_nnz, const int32_t* perm, double* Rrank, double* out, double* dflt);
// dflt[r] = the z transform (launch_row_ztransform_shard) of a zero in row r
int launch_row_z_defaults(plaidhip_ctx* ctx, const double* d_mean, const double* d_ssd, int32_t rows, int32_t n,
                          double* dflt);
// dense g x n (leading dimension ld) from row defaults and the stored entries: vals as they are, or z-transformed
// when d_mean / d_ssd are given
int launch_csc_expand(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* vals, int32_t g, int32_t n,
                      int64_t ld, const double* dflt, const double* d_mean, const double* d_ssd, double* out);
// the same over a column shard (ncols columns) of a matrix of n_total columns: the z transform's sd divides by n_total - 1
int launch_csc_expand_shard(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* vals, int32_t g,
                            int32_t ncols, int32_t n_total, int64_t ld, const double* dflt, const double* d_mean,
                            const double* d_ssd, double* out);
// the two passes of launch_csr_row_group_moments (one group) apart, over a column shard's rows: d_mean null: the sums of
// the rows' stored values; else the sums over them of (x - d_mean[row])^2 (the implicit zeros are the caller's)
int launch_csr_row_stored_moment(plaidhip_ctx* ctx, const int32_t* Rp, const double* Rx, int32_t rows, int32_t max_row_nnz,
                                 const double* d_mean, double* d_out);
// sample-sharded plaid.test on a dgCMatrix: d_out[k][row] = the unscaled sum of the row's stored values in group k
// (d_y indexed by Rj, the shard's column); the caller adds the shards and divides by the global group sizes
int launch_csr_row_group_stored_sums(plaidhip_ctx* ctx, const int32_t* Rp, const int32_t* Rj, const double* Rx, int32_t rows,
                                     int32_t max_row_nnz, const int32_t* d_y, double* d_out);
double onesample_p(double k, double s1, double s2, double* mean_out);
double twosample_p(double g, double k, double s1, double s2, double tot1, double tot2, double* diff_out);
double welch_p(double m0, double m1, double ssd0, double ssd1, double n0, double n1);
double clamp_p(double p);
double combine_p(const double* p, int np, int method);
void p_adjust_fdr(const double* p, int64_t m, double* q);

// kernels_spmm.hip
int alloc_pair_partial(plaidhip_ctx* ctx, plaidhip_geneset* gs);   // geneset.cpp: the pair plan's slice-partial scratch, once
int launch_spmm_dense_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const double* X,
                          int64_t ldx, int32_t n, int stat, double alpha, const double* alpha_div,
                          double beta, double* S, int64_t lds, uint32_t* flags,
                          int x_kind = 0);   // PLAIDHIP_X_*: what the caller knows about the values of X
// values of X as the internal callers know them (a compact exact staging is chosen from this, never a rounding one)
enum { PLAIDHIP_X_ANY = 0,        // arbitrary doubles
       PLAIDHIP_X_EXACT_F32 = 1,  // (half-)integers of magnitude <= 20,448, any sign (signed ranks): exact in fp32
       PLAIDHIP_X_RANKS = 2 };    // what colranks returns: half-integers in [0, nrow(X)]: 2x is a u16
int launch_spmm_mfma_f64(plaidhip_ctx* ctx, plaidhip_geneset* gs, const double* X, int64_t ldx, int32_t n, int stat,
                         double alpha, const double* alpha_div, double beta, double* S, int64_t lds, uint32_t* flags);
int launch_spmm_scatter_csc_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const int32_t* Xp,
                                const int32_t* Xi, const double* Xx, int32_t n, int stat, double alpha,
                                const double* alpha_div, double beta, double* S, int64_t lds, uint32_t* flags,
                                bool auto_select, bool bounded = false, const double* xmax_dev = nullptr, double xmax_host = 0.0,
                                int64_t nnz = -1, const struct plaidhip_scatter_med* med = nullptr);
// what the MED form of the scatter kernel needs (medians selected while the scores are written)
struct plaidhip_scatter_med {
  const double* pred;
  const double* cal;
  unsigned long long* cand;
  uint32_t* cnt;
  int32_t capc;
};
// the sparse crossprod + everything normalize_medians can know by then; launch_col_medians_resume finishes the medians
int launch_spmm_csc_fused_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const int32_t* Xp, const int32_t* Xi, const double* Xx,
                              int32_t n, int64_t nnz, int stat, double alpha, const double* alpha_div, double beta, double* S,
                              int64_t lds, uint32_t* flags, bool bounded, const double* xmax_dev, double xmax_host,
                              int64_t nnz_choice = -1 /* what picks scatter / gather when it is not nnz itself */);
// the dense crossprod (fp64 pair kernel) + everything normalize_medians can know by then (round 5); same resume call
int launch_spmm_dense_fused_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const double* X, int64_t ldx, int32_t n, int stat,
                                double alpha, const double* alpha_div, double beta, double* S, int64_t lds, uint32_t* flags,
                                int x_kind = 0);
int launch_col_medians_resume(plaidhip_ctx* ctx, const double* S, int64_t lds, int32_t m, int32_t n, int ignore_zero,
                              const uint32_t* flags, double* med, int64_t token = -1);
// {all values finite and >= 0 ? 0 : -1, max} of a device vector -> out[2] (kernels_norm.hip)
int launch_nonneg_range(plaidhip_ctx* ctx, const double* Xx, const int32_t* Xp, int32_t n, int64_t nnz_hint, double* out);
int launch_colsum_max(plaidhip_ctx* ctx, const double* Xx, const int32_t* Xp, int32_t n, double* out);
int launch_spmm_csc_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const int32_t* Xp,
                        const int32_t* Xi, const double* Xx, int32_t n, int64_t nnz /* -1: unknown */, int stat, double alpha,
                        const double* alpha_div, double beta, double* S, int64_t lds, uint32_t* flags,
                        // bounded: every stored value lies in [0, xmax] (rank weights; xmax = max(rX) on the device, or on
                        // the host when xmax_dev is null): the scatter kernel may use exact fixed-point accumulators
                        bool bounded = false, const double* xmax_dev = nullptr, double xmax_host = 0.0);
// kernels_wspmm.hip: t(x) %*% y for a sparse x with arbitrary values (device CSC slots); y dense (Yp == nullptr) or CSC
int launch_crossprod_weighted_f64(plaidhip_ctx* ctx, const int32_t* Wp, const int32_t* Wi, const double* Wx, int32_t g,
                                  int32_t m, const double* Y, int64_t ldy, const int32_t* Yp, const int32_t* Yi,
                                  const double* Yx, int32_t n, double* S, int64_t lds);
#ifdef PLAIDHIP_DIAG
void debug_set_ablation(int mode, void* dbg);   // diagnostic kernel variants (tools/ build only, make diag)
void debug_set_rank_stamps(void* dbg);          // per-phase cycle stamps of the bucket rank kernel
void debug_set_median_stamps(void* dbg);        // per-phase cycle stamps of the wave-per-column median kernel
#endif
// kernels_rank.hip
int launch_colranks_dense_f64(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t n,
                              int ties, int is_signed, double power, double* R, int64_t ldr,
                              double* colmax);
int launch_colranks_csc_f64(plaidhip_ctx* ctx, const int32_t* Xp, const double* Xx, int32_t n, int32_t max_col_nnz,
                            int ties, int is_signed, double power, double* Rx, double* colmax);
int32_t host_max_col_nnz(const int32_t* Xp, int32_t n);   // longest column of a host-side CSC pointer array
int launch_colranks_csc_dense_f64(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx,
                                  int32_t g, int32_t n, int ties, int is_signed, double power, double* R,
                                  int64_t ldr, double* colmax);
// dense ranks of CSC columns from the ranks of their stored values (zeros tie): any number of rows, every column at most
// max_sparse_rank_column() stored values; Rx_scratch: Xp[n] doubles
int launch_colranks_csc_dense_nz_f64(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g,
                                     int32_t n, int32_t max_col_nnz, int ties, int is_signed, double power,
                                     double* Rx_scratch, double* R, int64_t ldr, double* colmax);
int max_sparse_rank_column();
// whether colranks(ties = "average", power) on columns of g keys raises to a power of 1/4 steps by square roots
// (pow_quarters: the bucket and partitioned rankers) rather than by pow() (the sorting networks); the data-dependent
// fallback of clustered columns to the network aside
bool colranks_uses_power_quarters(plaidhip_ctx* ctx, int32_t g);
// ---- what the exact scorers share (the walk itself: bitmap_walk.h; the device loops: exact_common.h) ----------------------
// columns of a dense matrix (Xp == nullptr) or the stored values of CSC columns
struct RankCols {
  const int32_t* Xp;
  int32_t g, n;            // dense: rows; CSC: the longest column (what sizes the grid).  n columns
  int64_t ldx, ldr, lds;   // dense: leading dimensions of the input, of the ranks and of the scratch columns
};
inline RankCols dense_cols(int32_t g, int32_t n, int64_t ld) { return RankCols{nullptr, g, n, ld, ld, ld}; }
inline RankCols csc_cols(const int32_t* Xp, int32_t max_col_nnz, int32_t n) { return RankCols{Xp, max_col_nnz, n, 0, 0, 0}; }
// kernels_rank.hip: Q = rank(x, "last") from the min or average ranks R (a min-rank pass over the tie-free
// Y = (2 R - 1) 2^26 + (cnt - 1 - item)); R, Y, Q laid out as `cols` (dense: leading dimension ld); Q may be R; columns of
// fewer than 2^26 values.  Stream-ordered.
int launch_last_ranks(plaidhip_ctx* ctx, const RankCols& cols, const double* R, double* Y, double* Q);
// kernels_rank.hip: colnan[c] = 1 for a column holding a NaN: dense X (Xp == nullptr, g rows, leading dimension ldx) or the
// stored values of CSC columns (the longest max_col_nnz)
int launch_colnan(plaidhip_ctx* ctx, const double* X, int64_t ldx, const int32_t* Xp, int32_t g, int32_t n,
                  int32_t max_col_nnz, uint32_t* colnan);
// kernels_walk.hip: range_out[3] = {min, max, any NaN} of the m x n scores; part: 3 score_part_blocks(m n) doubles.
// score_part_blocks: the workgroups of the element-wise kernels over m x n scores
int score_part_blocks(plaidhip_ctx* ctx, int64_t count);
int launch_score_range(plaidhip_ctx* ctx, const double* S, int64_t lds, int32_t m, int32_t n, double* part, double* range_out);
// kernels_walk.hip: replaid.ssgsea.exact.  Operands of g x n columns (leading dimension ldq): Q = rank(x, "last"), and
// when alpha != 0 W = rank(x, "average")^alpha and P = W * Q; colnan[c] = 1 for a column holding a NaN.  Dense X
// (Xp == nullptr, leading dimension ldx; scratch 2 ldq n doubles) or CSC slots (rows increasing in each column; nnz =
// Xp[n], the longest column max_col_nnz; scratch 3 nnz doubles).  Two rank passes, stream-ordered.
int launch_ssgsea_exact_operands(plaidhip_ctx* ctx, const double* X, int64_t ldx, const int32_t* Xp, const int32_t* Xi,
                                 int32_t g, int32_t n, int32_t max_col_nnz, int64_t nnz, double alpha, double* Q, double* W,
                                 double* P, int64_t ldq, double* scratch, uint32_t* colnan);
// S (m x n, holding C on entry) <- the pinned epilogue of A, B (nullptr: alpha = 0) and kset (device int32 set sizes);
// part: 3 score_part_blocks(m n) doubles; range_out[3] = {min, max, any NaN} of the scores
int launch_ssgsea_exact_epilogue(plaidhip_ctx* ctx, const double* A, const double* B, double* S, int64_t lds, int32_t m,
                                 int32_t n, const int32_t* kset, int64_t N, int scale, const uint32_t* colnan, double* part,
                                 double* range_out);
int launch_ssgsea_exact_norm(plaidhip_ctx* ctx, double* S, int64_t lds, int32_t m, int32_t n, double range);
// multi.cpp: the walk kernel's row bound, which touches no device
int check_gsea_ks_genes(int32_t g);   // single = FALSE: PLAIDHIP_EUNSUPPORTED above PLAIDHIP_GSEA_KS_MAX_GENES rows
// kernels_ks.hip: replaid.ssgsea.exact(single = FALSE), the walk's value of largest magnitude (include/plaidhip.h:
// plaidhip_ssgsea_exact_ks) from the operands above; Gp / Gi on the device; Wpos: ldq n doubles of scratch when alpha != 0
// (the weights in walk order; may alias nothing the kernel reads).  g > PLAIDHIP_GSEA_KS_MAX_GENES: PLAIDHIP_EUNSUPPORTED.
int launch_gsea_ks(plaidhip_ctx* ctx, const double* Q, const double* W, double* Wpos, int64_t ldq, const uint32_t* colnan,
                   int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale, double* S,
                   int64_t lds);
// kernels_ks.hip: S (m x n, leading dimension lds) <- GSVA's random-walk statistic (replaid.gsva.exact) from the last ranks
// Q of the row-transformed columns; Gp / Gi on the device; T: g doubles of scratch for the weight table (tau != 0)
int launch_gsva_ks(plaidhip_ctx* ctx, const double* Q, int64_t ldq, const uint32_t* colnan, int32_t g, int32_t n,
                   const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int max_diff, double* T, double* S, int64_t lds);
// kernels_sing.hip: replaid.sing.exact (include/plaidhip.h: plaidhip_sing_exact).  All stream-ordered.
// Rpos[q - 1] = r per column (u32, leading dimension ldp), columns flagged in colnan skipped
int launch_sing_rpos(plaidhip_ctx* ctx, const double* R, const double* Q, int64_t ld, const uint32_t* colnan, int32_t g,
                     int32_t n, uint32_t* Rpos, int64_t ldp);
// the pinned score epilogue in place: Cu / Cd (nullable) hold the sums of min ranks of the up / down sets, ku / kd the set
// sizes on the device; tot (nullable, needs Cd) = up + down
int launch_sing_score(plaidhip_ctx* ctx, double* Cu, double* Cd, double* tot, int64_t lds, int32_t m, int32_t n,
                      const int32_t* ku, const int32_t* kd, int32_t g, int center, const uint32_t* colnan);
int launch_sing_add(plaidhip_ctx* ctx, const double* A, const double* B, double* out, int64_t lds, int32_t m, int32_t n);
// S (m x n, leading dimension lds) <- 1.4826 * median |s - median(s)| of every set's min ranks; Gp / Gi on the device.
// g > PLAIDHIP_GSEA_KS_MAX_GENES: PLAIDHIP_EUNSUPPORTED.
int launch_sing_mad(plaidhip_ctx* ctx, const double* Q, int64_t ldq, const uint32_t* Rpos, int64_t ldp, const uint32_t* colnan,
                    int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double* S, int64_t lds);
// kernels_trunc.hip: replaid.ucell.exact / replaid.aucell.exact (include/plaidhip.h: plaidhip_ucell_exact).  All stream-ordered.
// mode: PLAIDHIP_TRUNC_UCELL / _AUCELL; T: maxRank or aucMaxRank.  The most entries a column of g rows (a CSC column of len
// stored values) can get: what sizes the slots
int64_t truncated_bound(int mode, int64_t T, int64_t g, int64_t len, bool sparse);
// count, scan, fill: the compressed columns (Wp n + 1, Wi, Wx; rows ascending) of the non-zero weights from the ranks R --
// dense (Xp == nullptr: rank(x, "average") or, AUCell, rank(x, "last") of all g rows, leading dimension ldr) or of the stored
// values of CSC columns among themselves (rows increasing in each column).  cnt: n words of scratch; cap: the entries of
// Wi / Wx, behind which nothing is written.  u0 (CSC, UCell; n
// doubles): the zeros' weight, which the entries' weights are shifted by.
int launch_truncated_compact(plaidhip_ctx* ctx, int mode, int64_t T, const double* R, int64_t ldr, const int32_t* Xp,
                             const int32_t* Xi, const double* Xx, int32_t g, int32_t n, const uint32_t* colnan, int32_t* cnt,
                             int32_t* Wp, int32_t* Wi, double* Wx, int64_t cap, double* u0);
// the pinned epilogues in place: Cu / Cd (nullable) hold the weight sums of the up / down sets, ku / kd the aligned set sizes
// and Ku / Kd (nullable: k) the imputed ones; tot (nullable, needs Cu and Cd) = up - w_neg * down
int launch_ucell_exact(plaidhip_ctx* ctx, double* Cu, double* Cd, double* tot, int64_t lds, int32_t m, int32_t n,
                       const int32_t* ku, const int32_t* kd, const double* Ku, const double* Kd, const double* u0, int64_t T,
                       double w_neg, const uint32_t* colnan);
int launch_aucell_exact(plaidhip_ctx* ctx, double* C, int64_t lds, int32_t m, int32_t n, const int32_t* kset, int64_t A,
                        const uint32_t* colnan);
// the whole stage on device operands (what plaidhip_dev_truncated_ranks_f64 / _csc_f64 and the workers run): the
// NaN flags, the rank passes and launch_truncated_compact.  Dense: X g x n (ldx), R g x n doubles of scratch (ld g).  CSC:
// scratch 2 nnz doubles.
int truncated_ranks_stage(plaidhip_ctx* ctx, int mode, int64_t T, const double* X, int64_t ldx, const int32_t* Xp,
                          const int32_t* Xi, int32_t g, int32_t n, int32_t max_col_nnz, int64_t nnz, double* scratch,
                          uint32_t* colnan, int32_t* cnt, int32_t* Wp, int32_t* Wi, double* Wx, int64_t cap, double* u0);
// kernels_kcdf.hip: GSVA's Gaussian kernel CDF estimate (include/plaidhip.h: plaidhip_gsva_kcdf).  V (g x (j1 - j0), leading
// dimension ldv) <- the kernel sums of the test columns [j0, j1) of the dense device matrix X (g x n, leading dimension
// ldx) over ALL n samples; H: g doubles of scratch (the bandwidths).  Stream-ordered.
int launch_gsva_kcdf(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t n, int32_t j0, int32_t j1, double* H,
                     double* V, int64_t ldv);
void gsva_kcdf_table(double* out);   // the PLAIDHIP_GSVA_KCDF_TABLE values of Phi the kernels read
// H[i] <- the bandwidth h of row i alone (kcdf_row_moments_kernel, the launch launch_gsva_kcdf makes first)
int launch_gsva_kcdf_bandwidths(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t n, double* H);
int debug_gsva_kcdf_width(int32_t nj);             // test hook: the sub-group width kcdf_sum_kernel takes for nj test columns
void debug_gsva_kcdf_set_mode(int mode);           // test hooks: 0 fast index, 1 exact operations only, 2 fast and counting
unsigned long long debug_gsva_kcdf_slow_terms();   // mode 2: the last launch's terms that took the exact operations
// multi.cpp: columns [lo, lo + nloc) of V from the HOST matrix X (dense, or a dgCMatrix expanded on the device): all of X
// goes to this device.  dV: g x nloc on the device, leading dimension g.
int gsva_kcdf_columns(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                      int32_t lo, int32_t nloc, double* dV);
// kernels_gsea.hip: plaid.gsea (include/plaidhip.h: plaidhip_gsea).  All stream-ordered, all pointers device pointers.
// pos_obs (c x g int32) and Wpos (c x g) of every list from its last ranks Q and weights W (leading dimension ld; the
// outputs are packed, leading dimension g); a list flagged in listnan is skipped
int launch_gsea_operands(plaidhip_ctx* ctx, const double* Q, const double* W, int64_t ld, const uint32_t* listnan, int32_t g,
                         int32_t c, int32_t* pos_obs, double* Wpos);
// P (g x nb int32) <- the generated placements of the permutations b0 .. b0 + nb - 1; Y, R: g x nb doubles of scratch
int launch_gsea_placements(plaidhip_ctx* ctx, int32_t g, int64_t b0, int32_t nb, uint64_t seed, double* Y, double* R,
                           int32_t* P);
// the permutations one slab of the null holds: Y, R (fp64) and P (int32) of a slab stay within 256 MB, whole blocks of
// PLAIDHIP_GSEA_PERM_BLOCK, at least one (gsea_worker and plaidhip_gsea_permutations walk the same slabs)
inline int32_t gsea_slab_perms(int32_t g) {
  const int64_t fit = ((int64_t)256 << 20) / (20 * (int64_t)(g > 1 ? g : 1)) / PLAIDHIP_GSEA_PERM_BLOCK * PLAIDHIP_GSEA_PERM_BLOCK;
  return (int32_t)(fit > PLAIDHIP_GSEA_PERM_BLOCK ? fit : PLAIDHIP_GSEA_PERM_BLOCK);
}
// bad[0] |= 1 and bad[1] = max(bad[1], col0 + column + 1) for every column of P (g x nb) that is no permutation of 0..g-1
int launch_gsea_check_perm(plaidhip_ctx* ctx, const int32_t* P, int32_t g, int32_t nb, int32_t col0, uint32_t* bad);
// ES (c x m) <- the observed scores; weighted == 0: every weight is 1 (Wpos is not read); score_type: PLAIDHIP_GSEA_STD /
// _POS / _NEG, here and below
int launch_gsea_obs(plaidhip_ctx* ctx, int weighted, int score_type, const int32_t* pos_obs, const double* Wpos,
                    const uint32_t* listnan, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m, double* ES);
// the leading edges on the observed placements: le_len (c x m), le_idx (c x Gp[m]; the segment of (j, l) at l Gp[m] + Gp[j],
// -1 past the edge)
int launch_gsea_edges(plaidhip_ctx* ctx, int weighted, int score_type, const int32_t* pos_obs, const double* Wpos,
                      const uint32_t* listnan, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m,
                      int32_t* le_len, int32_t* le_idx);
// the null walks of the nbs placements in P (whole blocks of 64 but the call's last): their block partials into
// part[blk_at0 ..][c][6][m], the scores into null_out ([c][nbs][m]) when it is not null
int launch_gsea_null(plaidhip_ctx* ctx, int weighted, int score_type, const int32_t* P, int32_t nbs, const double* Wpos,
                     const uint32_t* listnan, const double* ES, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi,
                     int32_t m, double* part, int64_t blk_at0, double* null_out);
// out (m x 12 x c; padj left NaN) from all nblk blocks of partials, added in block order
int launch_gsea_null_reduce(plaidhip_ctx* ctx, const double* part, int32_t nblk, const double* ES, const int32_t* Gp, int32_t m,
                            int32_t c, int score_type, double* out);
// kernels_gsea_ml.hip: plaid.gsea's multilevel p-values (include/plaidhip.h: plaidhip_gsea_multilevel).  All stream-ordered,
// all pointers device pointers.  A ruler: one (list, side, set size) and the sets [set0, set0 + nset) of the per-set arrays.
struct GseaMlRuler {
  int32_t l;        // the list's Wpos on this device
  int32_t tag;      // the list's number in the Philox counter
  int32_t side;     // 0 positive, 1 negative
  int32_t k;
  int32_t set0, nset;
  double gmax;      // the largest target of its sets
};
struct GseaMlState {
  int32_t stage;    // stages recorded so far
  int32_t ended;
  int32_t status;   // when ended: PLAIDHIP_GSEA_ML_ESTIMATED (the level reached gmax) / _FLOOR / _STALLED
  int32_t pad;
  double level;     // m of the last stage recorded
  double P;         // P of the next stage (of the last one once ended)
};
inline int32_t gsea_ml_map_words(int32_t g) { return (g + 63) / 64; }   // words of one slot's map in global memory
// maps ([nr][n][gsea_ml_map_words(g)]) and H ([nr][n]) <- the initial states and their scores
int launch_gsea_ml_init(plaidhip_ctx* ctx, int weighted, int score_type, const GseaMlRuler* rulers, int32_t nr, int32_t n,
                        int32_t g, const double* Wpos, uint64_t seed, unsigned long long* maps, double* H);
// one stage of every unfinished ruler: level, count, trace (s_trace, m_trace: [nr][PLAIDHIP_GSEA_ML_MAX_STAGES]; h_trace
// nullable: [nr][MAX_STAGES][n]), read-off (gamma in; lstar, -1 before; cnt; est), end test, survivor copies; *unfinished +=
// the rulers that go on
int launch_gsea_ml_stage(plaidhip_ctx* ctx, const GseaMlRuler* rulers, GseaMlState* state, int32_t nr, int32_t n, int32_t g,
                         double eps, unsigned long long* maps, double* H, int32_t* s_trace, double* m_trace, double* h_trace,
                         const double* gamma, int32_t* lstar, int32_t* cnt, int32_t* est, uint32_t* unfinished);
// sweeps * k proposals of every slot of every unfinished ruler against the level of the stage just recorded
int launch_gsea_ml_mutate(plaidhip_ctx* ctx, int weighted, int score_type, const GseaMlRuler* rulers, const GseaMlState* state,
                          int32_t nr, int32_t n, int32_t g, const double* Wpos, uint64_t seed, int32_t sweeps,
                          unsigned long long* maps, double* H);
// kernels_fisher.hip: plaid.fisher (include/plaidhip.h: plaidhip_fisher).  All stream-ordered, all pointers device pointers.
// masks ([ceil(c / PLAIDHIP_FISHER_LIST_TILE)][g] u16: bit t up, bit 8 + t down in list tile * 8 + t) and tot ([c][2] int32:
// nUp, nDn; zeroed here) of the lists in sig (g x c int8, packed)
int launch_fisher_pack(plaidhip_ctx* ctx, const int8_t* sig, int32_t g, int32_t c, uint16_t* masks, int32_t* tot);
// ov ([c][2][m] int32: ovUp, ovDn) of every (list, set) from the masks; every Gi is in 0..g-1 (checked on the host)
int launch_fisher_count(plaidhip_ctx* ctx, const uint16_t* masks, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi,
                        int32_t m, int32_t* ov);
// out (m x 12 x c; the three padj columns left NaN) from the counts: hyper_tail.h's tail and odds ratio
int launch_fisher_tail(plaidhip_ctx* ctx, const int32_t* tot, const int32_t* ov, const int32_t* Gp, int32_t g, int32_t c,
                       int32_t m, double* out);
// the overlap lists: len (c x m), idx (c x Gp[m]; the segment of (j, l) at l Gp[m] + Gp[j], -1 past the overlap)
int launch_fisher_overlap(plaidhip_ctx* ctx, const int8_t* sig, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi,
                          int32_t m, int32_t* len, int32_t* idx);
// kernels_rankcor.hip: plaid.rankcor (include/plaidhip.h: plaidhip_rankcor).  All stream-ordered, all pointers device pointers.
// value mode: D (g x c, leading dimension g) <- stat - mu with NaN kept, vs ([c][4]) <- {n, T1, T2, flag (1: the list holds
// an infinity, 2: its values are all equal)}
int launch_rankcor_center(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t c, double* D, double* vs);
// tiles ([ceil(c / PLAIDHIP_RANKCOR_LIST_TILE)][g][8]: uint32 z = 2 rank, or doubles; 0 outside V) from R (g x c, leading
// dimension g: the ranks or the centred values, NaN outside V).  use_rank: sums ([c][3] u64 = n, T1, T2; zeroed here), vmask
// unused; else vmask ([ntile][g] bytes, bit t: in V of list tile * 8 + t), sums unused
int launch_rankcor_pack(plaidhip_ctx* ctx, int use_rank, const double* R, int32_t g, int32_t c, void* tiles, uint8_t* vmask,
                        unsigned long long* sums);
// kout ([c][m] int32: the members in V) and Aout ([c][m] int64 or double: their sum) of every (list, set); every Gi is in
// 0..g-1 and no set has more than g members (checked on the host)
int launch_rankcor_gather(plaidhip_ctx* ctx, int use_rank, const void* tiles, const uint8_t* vmask, int32_t g, int32_t c,
                          const int32_t* Gp, const int32_t* Gi, int32_t m, int32_t* kout, void* Aout);
// stats.cpp: the pinned epilogues of one (list, set), host only: o[0 .. 2] <- rho, t, p
void rankcor_rank_epilogue(int64_t n, int64_t T1, int64_t T2, int64_t k, int64_t A, double* o);
void rankcor_value_epilogue(int64_t n, double T1, double T2, int flag, int64_t k, double A, double* o);
// kernels_plage.hip: replaid.zscore and replaid.plage (include/plaidhip.h: plaidhip_zscore, plaidhip_plage).  All stream-ordered,
// all pointers device pointers unless said otherwise.  mean, sd: g doubles; flag: g int32 (0 kept, 1 constant, 2 sd not
// finite)
int launch_plage_moments(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t n, double* mean, double* sd,
                         int32_t* flag);
// Z (g x nj, leading dimension ldz) of the columns [j0, j0 + nj) of X: 0.0 in a constant row, NaN in a flagged one
int launch_plage_standardize_columns(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t j0, int32_t nj,
                                     const double* mean, const double* sd, const int32_t* flag, double* Z, int64_t ldz);
// Zg (g rows of ldz = plage_row_ld(n) doubles: a gene's n samples, then zeros) of all of X
int64_t plage_row_ld(int32_t n);
void debug_plage_set_gram(int mode);   // test hook: 0 the product's Gram kernel (rounded products), 1 the MFMA form
int launch_plage_standardize_rows(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t g, int32_t n, const double* mean,
                                  const double* sd, const int32_t* flag, double* Zg, int64_t ldz);
// per set: Ci / Cpos (Gp[m] int32 each: the kept members' rows and their positions in the set's segment, G's order), keff
// and nanflag (m int32 each); every Gi is in 0..g-1 (checked on the host)
int launch_plage_compact(plaidhip_ctx* ctx, const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* flag, int32_t* Ci,
                         int32_t* Cpos, int32_t* keff, int32_t* nanflag);
// the Gram matrices and the power iteration of every set: U (Gp[m] doubles: the oriented unit vector over the kept members),
// stats (m x 6, column-major), L (Gp[m] doubles or null: the loadings by member position).  hGp: the host's Gp.  Synchronizes.
int launch_plage_sets(plaidhip_ctx* ctx, const double* Zg, int64_t ldz, const int32_t* hGp, const int32_t* Gp, const int32_t* Ci,
                      const int32_t* Cpos, const int32_t* keff, const int32_t* nanflag, int32_t m, double tol, int32_t maxit,
                      double* U, double* stats, double* L);
// S (m x nj, leading dimension lds) <- the scores of the samples [j0, j0 + nj)
int launch_plage_project(plaidhip_ctx* ctx, const double* Zg, int64_t ldz, const int32_t* Gp, const int32_t* Ci,
                         const int32_t* keff, const int32_t* nanflag, const double* U, const double* stats, int32_t m, int32_t j0,
                         int32_t nj, double* S, int64_t lds);
// S (m x n sums of z over every set) <- S / sqrt(k); NaN for k = 0 and for a set with a flagged member
int launch_zscore_epilogue(plaidhip_ctx* ctx, double* S, int64_t lds, int32_t m, int32_t n, const int32_t* keff,
                           const int32_t* nanflag);
// kernels_norm.hip
int launch_minflags(plaidhip_ctx* ctx, const double* S, int64_t count, uint32_t* flags);
// kernels_medians.hip
int launch_col_medians(plaidhip_ctx* ctx, const double* S, int64_t lds, int32_t m, int32_t n,
                       int ignore_zero, const uint32_t* flags, double* med,
                       // non-null (streaming kernel, m > 6,144 only): columns with status[c] != 0 already have their median
                       const int32_t* status = nullptr);
// medians selected inside the sparse crossprod launch (kernels_medians.hip / kernels_spmm.hip: MED)
int launch_colmean_predict(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t n, const double* u,
                           double alpha, const double* alpha_div, double beta_kappa, double* pred);
int launch_median_calibrate(plaidhip_ctx* ctx, const double* medK, const double* pred, int32_t K, const uint32_t* flagsK,
                            double* cal);
int launch_median_select(plaidhip_ctx* ctx, const unsigned long long* cand, const uint32_t* cnt, int32_t n, int32_t nslice,
                         int32_t capc, int32_t m, const double* cal, int ignore_zero, const uint32_t* flags, double* med,
                         int32_t* status);
// kernels_norm.hip
int launch_sum(plaidhip_ctx* ctx, const double* v, int64_t count, double* out);
int launch_max(plaidhip_ctx* ctx, const double* v, int64_t count, double* out);
int launch_shift_columns(plaidhip_ctx* ctx, double* S, int64_t lds, int32_t m, int32_t n,
                         const double* med, double add, const double* red);
int launch_shift_columns_cast_f32(plaidhip_ctx* ctx, const double* S, int64_t lds, int32_t m, int32_t n, const double* med,
                                  double add, const double* red, float* out, int64_t ldo);

// element-wise / column helpers (replaid.ucell / aucell / scse)
int launch_map(plaidhip_ctx* ctx, double* v, int64_t count, int op, double p0, const double* scalar);
int launch_col_abs_sums(plaidhip_ctx* ctx, const double* X, int64_t ldx, int32_t len, const int32_t* Xp,
                        int32_t n, double* out);
int launch_affine(plaidhip_ctx* ctx, double* S, int64_t lds, int32_t m, int32_t n, double mul,
                  const double* col_div, double div_scale, const double* row_add, double add);
int launch_minmax(plaidhip_ctx* ctx, const double* v, int64_t count, double* out);

}  // namespace plaidhip
