// plaid.fry: the device passes that plaid.camera does not already have (include/plaidhip.h: plaidhip_fry; DESIGN.md
// section 26).
//
// fry_residual_kernel is camera_residual_kernel (kernels_camera.hip), the residual store of row_pair.h, with the gene's
// divisor read from c_g [nfit][rows] (stats.cpp: fry_divisors) instead of derived from rss / d, and 0.0 for a gene outside
// the universe (fry.h).
// fry_gram_kernel, one workgroup per set: C = sum over the members of rho_g rho_g' (d x d), and for every contrast j the
// border b_j = sum e_gj rho_g and a_j = sum e_gj^2 -- every entry one accumulator that takes the members in the set's own
// order, product rounded, then added -- and from them tr M_j and |M_j|_F^2 in a fixed order.
// fry_eigen_kernel, one workgroup per problem: the largest and the D-th largest eigenvalue of the symmetric M (dim <= 128,
// held in LDS with an odd row stride) by cyclic two-sided Jacobi in the round-robin tournament order.
#include "common.h"
#include "fry.h"
#include "row_pair.h"

#pragma clang fp contract(off)

namespace plaidhip {

template <int kP, bool kWide>
__global__ void __launch_bounds__(256)
fry_residual_kernel(const double* __restrict__ A, int64_t ld, int32_t rows, int32_t n, const double* __restrict__ Q,
                    const uint32_t* __restrict__ masks, int32_t p, int32_t f, const double* __restrict__ E,
                    const double* __restrict__ cg, double* __restrict__ Z, int64_t ldz) {
  const double* __restrict__ cf = cg + (int64_t)f * rows;
  row_pair_residual_store<kP, kWide>(
      A, ld, rows, n, Q, masks, p, f, E, Z, ldz, [&](int r) { return cf[r]; },
      [](double r, double c, bool used) { return fry_standardise(r, c, used); });
}

// Z' (rows x n, leading dimension ldz >= rows) of fit f; the operands of launch_camera_residuals with d_cg [nfit][rows] in
// place of d_rss and d
int launch_fry_residuals(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* d_Q,
                         const void* d_masks, int32_t p, int32_t f, const double* d_E, const double* d_cg, double* Z,
                         int64_t ldz) {
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 511) / 512, nblk);
  const uint32_t* mk = static_cast<const uint32_t*>(d_masks);
  dispatch_p(p, [&](auto kp) {
    dispatch_flag(row_pair_wide(rows, {ld, ldz}, {A, Z}), [&](auto wide) {
      hipLaunchKernelGGL((fry_residual_kernel<decltype(kp)::value, decltype(wide)::value>), grid, dim3(256), 0, ctx->stream, A, ld,
                         rows, n, d_Q, mk, p, f, d_E, d_cg, Z, ldz);
    });
  });
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// ---- the Gram matrix of a set's residual effects and its borders ------------------------------------------------------------
constexpr int kGramChunk = 16;   // members staged in LDS at a time: 16 x (127 + 32) doubles
static_assert(PLAIDHIP_FRY_MIXED_MAX <= 256 && PLAIDHIP_FRY_MAX_CONTRASTS <= 256,
              "fry_gram_kernel gives a row of C and a contrast to one thread of its 256 each");

// rho: rows x d row-major (gene g's residual effects at rho + g d; 0.0 for a gene outside the universe); e: rows x q
// row-major (0.0 likewise).  Set s = blockIdx.x + s0: C at Cm + (s - s0) d d, b at bm + ((s - s0) q + j) d, a, tr, fro at
// [(s - s0) q + j].  The d d + q d + q entries are dealt to the threads; an entry's accumulator starts at 0.0 and takes the
// members in the order of Gi.
__global__ void __launch_bounds__(256)
fry_gram_kernel(const double* __restrict__ rho, const double* __restrict__ e, int32_t d, int32_t q, const int32_t* __restrict__ Gp,
                const int32_t* __restrict__ Gi, int32_t s0, double* __restrict__ Cm, double* __restrict__ bm,
                double* __restrict__ am, double* __restrict__ trm, double* __restrict__ from) {
  __shared__ double srho[kGramChunk * (PLAIDHIP_FRY_MIXED_MAX - 1)];
  __shared__ double se[kGramChunk * PLAIDHIP_FRY_MAX_CONTRASTS];   // (check_fry_call and the device entry hold q to it)
  __shared__ double srow[PLAIDHIP_FRY_MIXED_MAX];
  const int s = blockIdx.x + s0, tid = threadIdx.x;
  const int g0 = Gp[s], g1 = Gp[s + 1];
  const int nC = d * d, nB = q * d, nE = nC + nB + q;
  double* __restrict__ C = Cm + (int64_t)blockIdx.x * nC;
  double* __restrict__ b = bm + (int64_t)blockIdx.x * nB;
  double* __restrict__ a = am + (int64_t)blockIdx.x * q;
  auto out = [&](int idx) -> double* { return idx < nC ? C + idx : idx < nC + nB ? b + (idx - nC) : a + (idx - nC - nB); };
  for (int idx = tid; idx < nE; idx += 256) *out(idx) = 0.0;
  for (int h0 = g0; h0 < g1; h0 += kGramChunk) {
    const int nh = g1 - h0 < kGramChunk ? g1 - h0 : kGramChunk;
    __syncthreads();
    for (int t = tid; t < nh * d; t += 256) srho[t] = rho[(int64_t)Gi[h0 + t / d] * d + t % d];
    for (int t = tid; t < nh * q; t += 256) se[t] = e[(int64_t)Gi[h0 + t / q] * q + t % q];
    __syncthreads();
    for (int idx = tid; idx < nE; idx += 256) {
      double* o = out(idx);
      double acc = *o;
      if (idx < nC) {
        const int i = idx / d, k = idx % d;
        for (int h = 0; h < nh; ++h) {
          const double pr = srho[h * d + i] * srho[h * d + k];
          acc += pr;
        }
      } else if (idx < nC + nB) {
        const int j = (idx - nC) / d, i = (idx - nC) % d;
        for (int h = 0; h < nh; ++h) {
          const double pr = se[h * q + j] * srho[h * d + i];
          acc += pr;
        }
      } else {
        const int j = idx - nC - nB;
        for (int h = 0; h < nh; ++h) {
          const double pr = se[h * q + j] * se[h * q + j];
          acc += pr;
        }
      }
      *o = acc;
    }
  }
  __syncthreads();   // (every entry was written by the thread that read it back; now the rows are read across threads)
  // rs_i = sum_k C_ik^2 ascending k; sc = sum_i rs_i, dg = sum_i C_ii ascending i; tr_j = a_j + dg;
  // fro_j = (a_j a_j + 2 sum_i b_ji^2) + sc
  if (tid < d) {
    double rs = 0.0;
    for (int k = 0; k < d; ++k) {
      const double c = C[tid * d + k];
      const double sq = c * c;
      rs += sq;
    }
    srow[tid] = rs;
  }
  __syncthreads();
  if (tid < q) {
    double sc = 0.0, dg = 0.0, sb = 0.0;
    for (int i = 0; i < d; ++i) {
      sc += srow[i];
      dg += C[i * d + i];
      const double bb = b[tid * d + i];
      const double sq = bb * bb;
      sb += sq;
    }
    const double aj = a[tid];
    const double aa = aj * aj, b2 = 2.0 * sb;
    trm[(int64_t)blockIdx.x * q + tid] = aj + dg;
    from[(int64_t)blockIdx.x * q + tid] = (aa + b2) + sc;
  }
}

// sets s0 .. s0 + ns - 1; every output is indexed from s0
int launch_fry_gram(plaidhip_ctx* ctx, const double* d_rho, const double* d_e, int32_t d, int32_t q, const int32_t* d_Gp,
                    const int32_t* d_Gi, int32_t s0, int32_t ns, double* d_C, double* d_b, double* d_a, double* d_tr, double* d_fro) {
  if (ns == 0 || q == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(fry_gram_kernel, dim3(ns), dim3(256), 0, ctx->stream, d_rho, d_e, d, q, d_Gp, d_Gi, s0, d_C, d_b, d_a, d_tr,
                     d_fro);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// ---- the two eigenvalues of M ------------------------------------------------------------------------------------------------
constexpr int kEigMaxSweeps = 30;
constexpr int kEigHalf = PLAIDHIP_FRY_MIXED_MAX / 2;              // the pairs of a round, at most
constexpr size_t kEigFixedLds = (256 + 5 * kEigHalf) * 8;        // what the kernel keeps in LDS beside M

// sum over the block of v (every thread gets it); the order is fixed by the block size
__device__ inline double fry_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return red[0];
}

// Problem blockIdx.x.  Either M (dim x dim, at M + problem dim dim) or, M == nullptr, the parts of fry_gram_kernel: problem =
// set * q + j, dim = d + 1, M = [a_j, b_j'; b_j, C].  Dk[problem]: which eigenvalue, counted from 1 in decreasing order, goes
// to lamD (clamped to 1 .. dim).  sweeps / conv: the sweeps run, and whether the off-diagonal mass fell below 2^-53 |M|_F.
__global__ void __launch_bounds__(256)
fry_eigen_kernel(const double* __restrict__ M, const double* __restrict__ Cm, const double* __restrict__ bm,
                 const double* __restrict__ am, int32_t dim, int32_t q, const int32_t* __restrict__ Dk, double* __restrict__ lam1,
                 double* __restrict__ lamD, int32_t* __restrict__ sweeps, int32_t* __restrict__ conv) {
  // all LDS is dynamic (the opt-in to the full 160 KiB counts static LDS against it): [the reduction's 256 doubles | a
  // round's c, s and new pivots, kEigHalf each | its pairs | M, dim x ld, ld odd: a column walk meets every bank]
  extern __shared__ double fry_lds[];
  double* red = fry_lds;
  double *sc = red + 256, *ss = sc + kEigHalf, *spp = ss + kEigHalf, *sqq = spp + kEigHalf;
  int* sp = reinterpret_cast<int*>(sqq + kEigHalf);
  int* sq = sp + kEigHalf;
  double* sA = sqq + kEigHalf + kEigHalf;   // (2 kEigHalf ints = kEigHalf doubles)
  const int tid = threadIdx.x, n = dim, ld = dim | 1;
  const int64_t prob = blockIdx.x;
  if (M != nullptr) {
    const double* src = M + prob * n * n;
    for (int t = tid; t < n * n; t += 256) sA[(t / n) * ld + t % n] = src[t];
  } else {
    const int d = n - 1;
    const int64_t set = prob / q;
    const double* C = Cm + set * d * d;
    const double* b = bm + prob * d;
    for (int t = tid; t < n * n; t += 256) {
      const int i = t / n, k = t % n;
      sA[i * ld + k] = i == 0 && k == 0 ? am[prob] : i == 0 ? b[k - 1] : k == 0 ? b[i - 1] : C[(i - 1) * d + (k - 1)];
    }
  }
  __syncthreads();
  double part = 0.0;
  for (int t = tid; t < n * n; t += 256) {
    const double v = sA[(t / n) * ld + t % n];
    part += v * v;
  }
  const double norm = sqrt(fry_block_sum(part, red));
  const double tol = 0x1p-53 * norm;
  const int N = n + (n & 1), half = N / 2;   // the tournament's players: an odd dim plays with one that sits out
  int sweep = 0, done = 0;
  if (!(norm - norm == 0.0)) done = -1;      // NaN or Inf inside: no eigenvalue
  while (done == 0) {
    part = 0.0;
    for (int t = tid; t < n * n; t += 256) {
      const int i = t / n, k = t % n;
      if (i != k) {
        const double v = sA[i * ld + k];
        part += v * v;
      }
    }
    const double off = sqrt(fry_block_sum(part, red));
    if (off <= tol) { done = 1; break; }
    if (sweep == kEigMaxSweeps) { done = 2; break; }
    ++sweep;
    for (int round = 0; round < N - 1; ++round) {
      // the circle method: player N - 1 stays, the others turn
      if (tid < half) {
        int x = tid == 0 ? N - 1 : (round + tid) % (N - 1);
        int y = tid == 0 ? round : (round - tid + (N - 1)) % (N - 1);
        if (x > y) { const int t = x; x = y; y = t; }
        double c = 1.0, s = 0.0, app = 0.0, aqq = 0.0;
        if (y < n) {
          app = sA[x * ld + x];
          aqq = sA[y * ld + y];
          const double apq = sA[x * ld + y];
          if (apq != 0.0) {
            const double tau = (aqq - app) / (2.0 * apq);
            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            s = t * c;
            app = app - t * apq;
            aqq = aqq + t * apq;
          }
        } else {
          x = y = -1;
        }
        sp[tid] = x;
        sq[tid] = y;
        sc[tid] = c;
        ss[tid] = s;
        spp[tid] = app;
        sqq[tid] = aqq;
      }
      __syncthreads();
      for (int t = tid; t < half * n; t += 256) {   // J'A: rows x and y
        const int k = t / n, j = t % n, x = sp[k], y = sq[k];
        if (x < 0 || ss[k] == 0.0) continue;
        const double u = sA[x * ld + j], v = sA[y * ld + j];
        sA[x * ld + j] = sc[k] * u - ss[k] * v;
        sA[y * ld + j] = ss[k] * u + sc[k] * v;
      }
      __syncthreads();
      for (int t = tid; t < half * n; t += 256) {   // (J'A)J: columns x and y
        const int k = t / n, i = t % n, x = sp[k], y = sq[k];
        if (x < 0 || ss[k] == 0.0) continue;
        const double u = sA[i * ld + x], v = sA[i * ld + y];
        sA[i * ld + x] = sc[k] * u - ss[k] * v;
        sA[i * ld + y] = ss[k] * u + sc[k] * v;
      }
      __syncthreads();
      if (tid < half && sp[tid] >= 0 && ss[tid] != 0.0) {   // the closed forms of the pivot block
        const int x = sp[tid], y = sq[tid];
        sA[x * ld + x] = spp[tid];
        sA[y * ld + y] = sqq[tid];
        sA[x * ld + y] = 0.0;
        sA[y * ld + x] = 0.0;
      }
      __syncthreads();
    }
  }
  // the diagonal in decreasing order: entry i has rank = the entries above it (ties by index)
  int want = Dk[prob];
  want = want < 1 ? 1 : want > n ? n : want;
  if (done < 0) {
    if (tid == 0) {
      lam1[prob] = lamD[prob] = __builtin_nan("");
      sweeps[prob] = 0;
      conv[prob] = 0;
    }
    return;
  }
  if (tid < n) {
    const double v = sA[tid * ld + tid];
    int rank = 0;
    for (int k = 0; k < n; ++k) {
      const double w = sA[k * ld + k];
      rank += (w > v || (w == v && k < tid)) ? 1 : 0;
    }
    if (rank == 0) lam1[prob] = v;
    if (rank == want - 1) lamD[prob] = v;
  }
  if (tid == 0) {
    sweeps[prob] = sweep;
    conv[prob] = done == 1 ? 1 : 0;
  }
}

// nprob problems of dimension dim <= PLAIDHIP_FRY_MIXED_MAX; d_M, or (d_M == nullptr) the parts d_C / d_b / d_a with q
// contrasts per set
int launch_fry_eigen(plaidhip_ctx* ctx, const double* d_M, const double* d_C, const double* d_b, const double* d_a, int32_t dim,
                     int32_t q, int64_t nprob, const int32_t* d_Dk, double* d_lam1, double* d_lamD, int32_t* d_sweeps,
                     int32_t* d_conv) {
  if (nprob == 0 || dim == 0) return PLAIDHIP_OK;
  const size_t lds = kEigFixedLds + (size_t)dim * (size_t)(dim | 1) * 8;   // at most 4,608 + 132,096 bytes
  if (lds > 48 * 1024) PH_FULL_LDS(ctx, fry_eigen_kernel);
  hipLaunchKernelGGL(fry_eigen_kernel, dim3((unsigned)nprob), dim3(256), lds, ctx->stream, d_M, d_C, d_b, d_a, dim, q, d_Dk, d_lam1,
                     d_lamD, d_sweeps, d_conv);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
