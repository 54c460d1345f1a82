// replaid.ucell.exact / replaid.aucell.exact: the truncated-rank stage and the two pinned epilogues
// (include/plaidhip.h: plaidhip_ucell_exact, plaidhip_aucell_exact, plaidhip_dev_truncated_ranks_f64 / _csc_f64; DESIGN.md
// section 15).
//
// Both statistics read only the top T genes of a cell, so their rank weights are sparse whatever X is: at most about T
// entries per column.  The stage turns ranks into compressed columns (row, weight) of the non-zero weights -- device CSC
// slots the existing sparse crossprod multiplies with the prepared gene sets.
//
//   count pass -> exclusive scan on the device -> fill pass.  Nothing is read back; the slots are sized on the host from a
//   bound per column (truncated_bound), the scan places the columns back to back.  Rows ascend inside a column: a
//   workgroup walks its column in tiles of 256 items and a workgroup scan keeps the order.
//
//   UCell mode (0):  d = N + 1 - rank(x, "average"),  u = d <= T ? T + 1 - d : 0.  A tie group has one d, so it is
//                    weighted as a whole or not at all.
//   AUCell mode (1): pos = N + 1 - rank(x, "last"),   w = pos < A ? A - pos : 0.
//
// Dense X: the rank passes of kernels_rank.hip over all rows, then trunc_items_kernel over the rows.
// A dgCMatrix: the stored values are ranked among themselves (launch_colranks_csc_f64), no g x n buffer of any type.  With
// npos / nneg stored values above / below zero and len stored values, a stored v > 0 has d = len + 1 - r, a stored v < 0 has
// d = N + 1 - r, and all Z = N - npos - nneg zeros (stored or not) form one tie group at d0 = npos + (Z + 1) / 2.
//   UCell: the zeros' weight u0 is not enumerated: every stored non-zero entry carries u - u0 (possibly negative), stored
//          zeros carry 0, and the epilogue adds k * u0 per set.  All half-integers: exact in fp64 in any order.
//   AUCell: the zeros take the positions npos + 1 .. in row order.  trunc_aucell_csc_kernel walks the column in words of 64
//          rows (a lane per word: the mask of its stored non-zero rows by a binary search into the column's row indices),
//          scans the words' zero counts and emits the first A - 1 - npos zero rows between the stored ones, as far as
//          they are needed and no further.
//
// The epilogues are integer work closed by one division (and, for UCell's total, one product and one subtraction: fp
// contraction is off for the whole file).
#pragma clang fp contract(off)
#include <algorithm>

#include "common.h"
#include "exact_common.h"

namespace plaidhip {

namespace {

constexpr int kTruncBlock = 256;

// exclusive scan of one count per thread over the workgroup (NW wavefronts); *total: the sum.  s_w: NW words of LDS, free
// to reuse when the call returns on every thread (two barriers inside).
template <int NW>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  __syncthreads();   // (the readers of the previous call are done)
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const uint32_t x = s_w[w];
    base += (w < wave) ? x : 0u;
    tot += x;
  }
  *total = tot;
  return base + inc - v;
}

struct TruncArgs {
  const double* R;       // dense: the ranks of the g rows of every column (leading dimension ldr); CSC: of the stored values
  int64_t ldr;
  const int32_t* Xp;     // CSC slots (null: dense)
  const int32_t* Xi;
  const double* Xx;
  const uint32_t* colnan;
  int32_t g, n;
  int mode;              // 0 UCell, 1 AUCell
  double T;              // maxRank or aucMaxRank, an integer in 1..g
  int32_t* cnt;          // count pass: the entries of every column
  const int32_t* ptr;    // fill pass: where every column starts
  int32_t* rows;
  double* w;
  double* u0;            // CSC, UCell: the zeros' weight per column (count pass; may be null)
  int64_t cap;           // entries of rows / w: nothing is written at or behind it
  int fill;
};

__device__ __forceinline__ int64_t imin64(int64_t x, int64_t y) { return x < y ? x : y; }
__device__ __forceinline__ int64_t imax64(int64_t x, int64_t y) { return x > y ? x : y; }

__device__ __forceinline__ double trunc_weight(int mode, double T, double d) {   // d: descending rank or position
  if (mode == 0) return d <= T ? T + 1.0 - d : 0.0;
  return d < T ? T - d : 0.0;
}

// {stored values above zero, below zero} of a CSC column, on every thread
__device__ __forceinline__ void trunc_sign_counts(const double* __restrict__ x, int32_t len, uint32_t* s_w, uint32_t* npos,
                                                  uint32_t* nneg) {
  uint32_t p = 0, q = 0;
  for (int32_t i = threadIdx.x; i < len; i += kTruncBlock) {
    const double v = x[i];
    p += (v > 0.0) ? 1u : 0u;
    q += (v < 0.0) ? 1u : 0u;
  }
  (void)block_excl_scan<kTruncBlock / 64>(p, s_w, npos);
  (void)block_excl_scan<kTruncBlock / 64>(q, s_w, nneg);
}

// One item per row of a dense column, or per stored value of a CSC column in UCell mode: at most one entry each.
__global__ void __launch_bounds__(kTruncBlock)
trunc_items_kernel(TruncArgs a) {
  __shared__ uint32_t s_w[kTruncBlock / 64];
  const int tid = threadIdx.x;
  const bool sparse = a.Xp != nullptr;
  const double N = (double)a.g;
  for (int c = blockIdx.x; c < a.n; c += gridDim.x) {
    const int64_t base = sparse ? (int64_t)a.Xp[c] : (int64_t)c * a.ldr;
    const int32_t len = sparse ? a.Xp[c + 1] - a.Xp[c] : a.g;
    const bool bad = a.colnan[c] != 0u;
    double u0 = 0.0;
    if (sparse) {
      uint32_t npos = 0, nneg = 0;
      trunc_sign_counts(a.Xx + base, len, s_w, &npos, &nneg);
      const double Z = N - (double)npos - (double)nneg;
      const double d0 = (double)npos + (Z + 1.0) / 2.0;   // a half-integer: exact
      u0 = (Z > 0.0 && !bad) ? trunc_weight(0, a.T, d0) : 0.0;
      if (!a.fill && a.u0 != nullptr && tid == 0) a.u0[c] = u0;
    }
    uint32_t run = 0;
    for (int32_t b0 = 0; b0 < len; b0 += kTruncBlock) {
      const int32_t i = b0 + tid;
      double w = 0.0;
      int32_t row = i;
      if (i < len && !bad) {
        const double r = a.R[base + i];
        if (!sparse) {
          w = trunc_weight(a.mode, a.T, N + 1.0 - r);
        } else {
          const double v = a.Xx[base + i];
          row = a.Xi[base + i];
          const double d = (v > 0.0) ? (double)len + 1.0 - r : N + 1.0 - r;
          w = (v != 0.0) ? trunc_weight(0, a.T, d) - u0 : 0.0;
        }
      }
      const uint32_t flag = (w != 0.0) ? 1u : 0u;   // (false for a NaN, which only a flagged column could hold)
      uint32_t tot = 0;
      const uint32_t excl = block_excl_scan<kTruncBlock / 64>(flag, s_w, &tot);
      if (a.fill && flag) {
        const int64_t o = (int64_t)a.ptr[c] + run + excl;
        if (o < a.cap) {
          a.rows[o] = row;
          a.w[o] = w;
        }
      }
      run += tot;
    }
    if (!a.fill && tid == 0) a.cnt[c] = (int32_t)run;
  }
}

// AUCell mode on CSC columns: R holds rank(x, "last") of the stored values among themselves.  A lane per word of 64 rows.
__global__ void __launch_bounds__(kTruncBlock)
trunc_aucell_csc_kernel(TruncArgs a) {
  __shared__ uint32_t s_w[kTruncBlock / 64];
  const int tid = threadIdx.x;
  const int64_t N = a.g;
  const double A = a.T;
  for (int c = blockIdx.x; c < a.n; c += gridDim.x) {
    const int64_t base = a.Xp[c];
    const int32_t len = a.Xp[c + 1] - a.Xp[c];
    if (a.colnan[c] != 0u) {
      if (!a.fill && tid == 0) a.cnt[c] = 0;
      continue;
    }
    const int32_t* __restrict__ xi = a.Xi + base;
    const double* __restrict__ xx = a.Xx + base;
    const double* __restrict__ rq = a.R + base;
    uint32_t npos = 0, nneg = 0;
    trunc_sign_counts(xx, len, s_w, &npos, &nneg);
    const int64_t Z = N - (int64_t)npos - (int64_t)nneg;
    // zero rows that take a position below A: the first F of them in row order
    const int64_t F = imin64(Z, imax64((int64_t)A - 1 - (int64_t)npos, 0));
    const int64_t last_row = len > 0 ? (int64_t)xi[len - 1] : -1;
    int64_t zrun = 0;      // zero rows before this tile
    uint32_t erun = 0;     // entries before this tile
    for (int64_t r0t = 0; r0t < N && (zrun < F || r0t <= last_row); r0t += (int64_t)kTruncBlock * 64) {
      const int64_t row0 = r0t + (int64_t)tid * 64;
      unsigned long long nzmask = 0ull, emask = 0ull, valid = 0ull;
      int32_t p0 = 0;
      if (row0 < N) {
        const int64_t nv = imin64(64, N - row0);
        valid = nv == 64 ? ~0ull : ((1ull << nv) - 1ull);
        int32_t lo = 0, hi = len;   // the first stored entry with a row >= row0
        while (lo < hi) {
          const int32_t mid = (lo + hi) >> 1;
          if ((int64_t)xi[mid] < row0) lo = mid + 1; else hi = mid;
        }
        p0 = lo;
        for (int32_t p = p0; p < len && (int64_t)xi[p] < row0 + 64; ++p) {
          const double v = xx[p];
          if (v != 0.0) {
            const unsigned long long bit = 1ull << ((int64_t)xi[p] - row0);
            nzmask |= bit;
            const double pos = (v > 0.0) ? (double)len + 1.0 - rq[p] : (double)N + 1.0 - rq[p];
            if (trunc_weight(1, A, pos) != 0.0) emask |= bit;
          }
        }
      }
      const unsigned long long zmask = ~nzmask & valid;
      const uint32_t zc = (uint32_t)__popcll(zmask);
      uint32_t ztot = 0, etot = 0;
      const int64_t zi0 = zrun + block_excl_scan<kTruncBlock / 64>(zc, s_w, &ztot);
      const int64_t ze = imin64(zc, imax64(F - zi0, 0));   // this word's zero rows with a position
      unsigned long long zsel = 0ull;
      {
        unsigned long long t = zmask;
        for (int64_t k = 0; k < ze; ++k) { zsel |= t & (0ull - t); t &= t - 1ull; }
      }
      const uint32_t ec = (uint32_t)__popcll(emask) + (uint32_t)ze;
      const uint32_t eexcl = block_excl_scan<kTruncBlock / 64>(ec, s_w, &etot);
      if (a.fill && ec != 0u) {
        int64_t o = (int64_t)a.ptr[c] + erun + eexcl;
        int64_t zk = 0;
        int32_t p = p0;
        unsigned long long mm = emask | zsel;
        while (mm != 0ull) {
          const int b = __ffsll((long long)mm) - 1;
          mm &= mm - 1ull;
          const int64_t row = row0 + b;
          double w;
          if ((zsel >> b) & 1ull) {
            w = A - (double)((int64_t)npos + 1 + zi0 + zk);
            ++zk;
          } else {
            while (p < len && (int64_t)xi[p] != row) ++p;   // (row is a stored row of this word)
            if (p >= len) break;
            const double v = xx[p];
            w = trunc_weight(1, A, (v > 0.0) ? (double)len + 1.0 - rq[p] : (double)N + 1.0 - rq[p]);
          }
          if (o < a.cap) {
            a.rows[o] = (int32_t)row;
            a.w[o] = w;
          }
          ++o;
        }
      }
      zrun += ztot;
      erun += etot;
    }
    if (!a.fill && tid == 0) a.cnt[c] = (int32_t)erun;
    __syncthreads();
  }
}

// ptr[0..n] = the exclusive scan of cnt[0..n): one workgroup, a running carry
__global__ void __launch_bounds__(1024)
trunc_scan_kernel(const int32_t* __restrict__ cnt, int32_t n, int32_t* __restrict__ ptr) {
  __shared__ uint32_t s_w[16];
  uint32_t carry = 0;
  for (int32_t b0 = 0; b0 < n; b0 += 1024) {
    const int32_t i = b0 + (int32_t)threadIdx.x;
    const uint32_t v = i < n ? (uint32_t)cnt[i] : 0u;
    uint32_t tot = 0;
    const uint32_t excl = block_excl_scan<16>(v, s_w, &tot);
    if (i < n) ptr[i] = (int32_t)(carry + excl);
    carry += tot;
  }
  if (threadIdx.x == 0) ptr[n] = (int32_t)carry;
}

// ---- the pinned epilogues (include/plaidhip.h) -------------------------------------------------------------------------
// UCell.  C holds sum (u - u0) over the aligned members (a half-integer, exact); S2 = 2 C + 2 k u0 in integers.
__device__ __forceinline__ double ucell_exact_one(double C, double u0, int64_t k, int64_t K, int64_t T, bool bad) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (bad || K == 0) return nan;
  const int64_t S2 = (int64_t)(C + C) + k * (int64_t)(u0 + u0);
  const int64_t U2 = 2 * K * (T + 1) - S2 - K * (K + 1);
  const double auc = 1.0 - (double)U2 / (double)(2 * K * T);
  return auc < 0.0 ? 0.0 : auc;
}

__global__ void __launch_bounds__(256)
ucell_exact_kernel(double* __restrict__ Cu, double* __restrict__ Cd, double* __restrict__ tot, int64_t lds, int32_t m, int32_t n,
                   const int32_t* __restrict__ ku, const int32_t* __restrict__ kd, const double* __restrict__ Ku,
                   const double* __restrict__ Kd, const double* __restrict__ u0, int64_t T, double w_neg,
                   const uint32_t* __restrict__ colnan) {
  for_each_score(m, n, lds, [&](int64_t c, int64_t j, int64_t at) {
    const bool bad = colnan[c] != 0u;
    const double z0 = u0 != nullptr ? u0[c] : 0.0;
    double up = 0.0;
    if (Cu != nullptr) {
      const int64_t k = ku[j];
      up = ucell_exact_one(bad ? 0.0 : Cu[at], z0, k, Ku != nullptr ? (int64_t)Ku[j] : k, T, bad);
      Cu[at] = up;
    }
    if (Cd != nullptr) {
      const int64_t k = kd[j];
      const double dn = ucell_exact_one(bad ? 0.0 : Cd[at], z0, k, Kd != nullptr ? (int64_t)Kd[j] : k, T, bad);
      Cd[at] = dn;
      if (tot != nullptr) {
        const double prod = w_neg * dn;
        const double t = up - prod;
        tot[at] = t < 0.0 ? 0.0 : t;   // (a NaN stays)
      }
    }
  });
}

// AUCell.  C holds the area sum (A - pos), an exact integer.
__global__ void __launch_bounds__(256)
aucell_exact_kernel(double* __restrict__ C, int64_t lds, int32_t m, int32_t n, const int32_t* __restrict__ kset, int64_t A,
                    const uint32_t* __restrict__ colnan) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for_each_score(m, n, lds, [&](int64_t c, int64_t j, int64_t at) {
    const int64_t k = kset[j];
    const int64_t kk = k < A - 1 ? k : A - 1;
    const int64_t max_auc = kk * A - kk * (kk + 1) / 2;
    const int64_t area = (int64_t)C[at];
    double s = (double)area / (double)max_auc;   // (k = 0 or A = 1: 0 / 0)
    if (colnan[c] != 0u) s = nan;
    C[at] = s;
  });
}

}  // namespace

// the most entries a column can get: what the caller sizes the slots by
int64_t truncated_bound(int mode, int64_t T, int64_t g, int64_t len, bool sparse) {
  if (mode == 1) return std::min<int64_t>(g, T - 1);
  if (sparse) return len;                       // the shifted weights: every stored non-zero value may carry one
  return std::min<int64_t>(g, 2 * T - 1);       // the boundary tie group, whose average is <= T, ends at 2 T - 1 at most
}

int launch_truncated_compact(plaidhip_ctx* ctx, int mode, int64_t T, const double* R, int64_t ldr, const int32_t* Xp,
                             const int32_t* Xi, const double* Xx, int32_t g, int32_t n, const uint32_t* colnan, int32_t* cnt,
                             int32_t* Wp, int32_t* Wi, double* Wx, int64_t cap, double* u0) {
  if (n == 0) return PLAIDHIP_OK;
  TruncArgs a{};
  a.cap = cap;
  a.R = R;
  a.ldr = ldr;
  a.Xp = Xp;
  a.Xi = Xi;
  a.Xx = Xx;
  a.colnan = colnan;
  a.g = g;
  a.n = n;
  a.mode = mode;
  a.T = (double)T;
  a.cnt = cnt;
  a.ptr = Wp;
  a.rows = Wi;
  a.w = Wx;
  a.u0 = u0;
  const int grid_cap = ctx->num_cu * 8;
  const dim3 grid((unsigned)(n < grid_cap ? n : grid_cap));
  const bool words = Xp != nullptr && mode == 1;
  for (int fill = 0; fill < 2; ++fill) {
    a.fill = fill;
    if (words) hipLaunchKernelGGL(trunc_aucell_csc_kernel, grid, dim3(kTruncBlock), 0, ctx->stream, a);
    else hipLaunchKernelGGL(trunc_items_kernel, grid, dim3(kTruncBlock), 0, ctx->stream, a);
    PH_HIP(hipGetLastError());
    if (fill == 0) {
      hipLaunchKernelGGL(trunc_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, cnt, n, Wp);
      PH_HIP(hipGetLastError());
    }
  }
  return PLAIDHIP_OK;
}

int launch_ucell_exact(plaidhip_ctx* ctx, double* Cu, double* Cd, double* tot, int64_t lds, int32_t m, int32_t n,
                       const int32_t* ku, const int32_t* kd, const double* Ku, const double* Kd, const double* u0, int64_t T,
                       double w_neg, const uint32_t* colnan) {
  const int64_t total = (int64_t)m * n;
  if (total == 0) return PLAIDHIP_OK;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)ctx->num_cu * 16);
  hipLaunchKernelGGL(ucell_exact_kernel, dim3(grid), dim3(256), 0, ctx->stream, Cu, Cd, tot, lds, m, n, ku, kd, Ku, Kd, u0, T,
                     w_neg, colnan);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_aucell_exact(plaidhip_ctx* ctx, double* C, int64_t lds, int32_t m, int32_t n, const int32_t* kset, int64_t A,
                        const uint32_t* colnan) {
  const int64_t total = (int64_t)m * n;
  if (total == 0) return PLAIDHIP_OK;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)ctx->num_cu * 16);
  hipLaunchKernelGGL(aucell_exact_kernel, dim3(grid), dim3(256), 0, ctx->stream, C, lds, m, n, kset, A, colnan);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// the whole stage on device operands: the NaN flags, the rank passes, count / scan / fill
int truncated_ranks_stage(plaidhip_ctx* ctx, int mode, int64_t T, const double* X, int64_t ldx, const int32_t* Xp,
                          const int32_t* Xi, int32_t g, int32_t n, int32_t max_col_nnz, int64_t nnz, double* scratch,
                          uint32_t* colnan, int32_t* cnt, int32_t* Wp, int32_t* Wi, double* Wx, int64_t cap, double* u0) {
  if (n == 0 || g == 0) return PLAIDHIP_OK;
  int rc = launch_colnan(ctx, X, ldx, Xp, g, n, max_col_nnz, colnan);
  if (rc != PLAIDHIP_OK) return rc;
  double* R = scratch;
  if (Xp == nullptr) {
    rc = launch_colranks_dense_f64(ctx, X, ldx, g, n, mode == PLAIDHIP_TRUNC_UCELL ? PLAIDHIP_TIES_AVERAGE : PLAIDHIP_TIES_LAST,
                                   0, 1.0, R, g, nullptr);
    if (rc != PLAIDHIP_OK) return rc;
    return launch_truncated_compact(ctx, mode, T, R, g, nullptr, nullptr, nullptr, g, n, colnan, cnt, Wp, Wi, Wx, cap, nullptr);
  }
  if (max_col_nnz == 0) {   // no stored value anywhere: nothing to rank
  } else if (mode == PLAIDHIP_TRUNC_UCELL) {
    rc = launch_colranks_csc_f64(ctx, Xp, X, n, max_col_nnz, PLAIDHIP_TIES_AVERAGE, 0, 1.0, R, nullptr);
  } else {   // rank(x, "last") of the stored values: two min-rank passes, stream-ordered (the size of Y is the caller's nnz)
    double* Y = scratch + std::max<int64_t>(nnz, 1);
    rc = launch_colranks_csc_f64(ctx, Xp, X, n, max_col_nnz, PLAIDHIP_TIES_MIN, 0, 1.0, R, nullptr);
    if (rc == PLAIDHIP_OK) rc = launch_last_ranks(ctx, csc_cols(Xp, max_col_nnz, n), R, Y, R);
  }
  if (rc != PLAIDHIP_OK) return rc;
  return launch_truncated_compact(ctx, mode, T, R, 0, Xp, Xi, X, g, n, colnan, cnt, Wp, Wi, Wx, cap, u0);
}

}  // namespace plaidhip
