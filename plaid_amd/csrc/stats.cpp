// Host-side tail of plaid.test() (R/plaid.R:392-537): from per-set sufficient statistics (O(sets)
// numbers reduced on the device) to t statistics, p-values, the combined p and the FDR.
// Distribution functions are plain double-precision implementations of the textbook forms R uses:
//   2*pt(|t|, df, lower=FALSE)  = I_{df/(df+t^2)}(df/2, 1/2)     regularised incomplete beta
//   pchisq(x, 2k, lower=FALSE)  = exp(-x/2) * sum_{i<k} (x/2)^i / i!
//   qnorm / pnorm upper tails   = Wichura's AS241 (PPND16) / erfc
#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>
#include <numeric>
#include <thread>
#include <functional>
#include <vector>

#include "camera.h"
#include "common.h"
#include "fry.h"
#include "lmfit_na.h"
#include "lowess.h"
#include "roast.h"
#include "romer.h"

namespace plaidhip {

namespace {

// continued fraction of the incomplete beta function (modified Lentz)
double betacf(double a, double b, double x) {
  const double tiny = 1e-300, eps = 1e-16;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (std::fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= 10000; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) < eps) break;
  }
  return h;
}

// The even part of that fraction (DiDonato & Morris 1992, the form TOMS 708 calls BFRAC):
//   I_x(a, b) = x^a y^b / B(a, b) / (b0 + a1 / (b1 + a2 / (b2 + ...)))
//   a_m = (a + m - 1)(a + b + m - 1) m (b - m) x^2 / (a + 2m - 1)^2
//   b_m = m + m (b - m) x / (a + 2m - 1) + (a + m)(a y - b x + 1 + m (2 - x)) / (a + 2m + 1)
// It takes y = 1 - x as given, so for large a and y = O(1 / a) no step forms 1 - (1 - O(y)), which costs betacf ~u / y
// (5e-10 at a = 5e6, |t| ~ 1.7).  Returns the denominator.
double betacf_even(double a, double b, double x, double y) {
  const double tiny = 1e-300, eps = 2.3e-16;
  const double ayb = a * y - b * x + 1.0;
  double f = a * ayb / (a + 1.0);
  if (std::fabs(f) < tiny) f = tiny;
  double c = f, d = 0.0;
  for (int m = 1; m <= 10000; ++m) {
    const double den = a + 2.0 * m - 1.0;
    const double an = (a + m - 1.0) * (a + b + m - 1.0) * m * (b - m) * x * x / (den * den);
    const double bn = m + m * (b - m) * x / den + (a + m) * (ayb + m * (2.0 - x)) / (a + 2.0 * m + 1.0);
    d = bn + an * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = bn + an / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = c * d;
    f *= del;
    if (std::fabs(del - 1.0) < eps) break;
  }
  return f;
}

// regularised incomplete beta I_x(a, b); y = 1 - x is passed in separately so that it keeps its
// digits when x rounds to 1
double betai(double a, double b, double x, double y) {
  if (!(x > 0.0)) return 0.0;
  if (!(y > 0.0)) return 1.0;
  // log(1 / B(a, b)); for b = 1/2 and large a the three lgamma values are ~a ln a each and their
  // difference loses digits, so use the Stirling series of ln Gamma(a + 1/2) - ln Gamma(a)
  double lnorm;
  if (b == 0.5 && a >= 100.0) {
    const double ia = 1.0 / a, ia2 = ia * ia;
    lnorm = 0.5 * std::log(a) - ia * (0.125 - ia2 * (1.0 / 192.0 - ia2 * (1.0 / 640.0))) - 0.5 * std::log(M_PI);
  } else {
    lnorm = std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b);
  }
  // log of the argument nearer to 1 from the other one: log(x) of a rounded x = 1 - 3e-7 has lost seven digits, and
  // a = 5e6 multiplies what is left (large Welch degrees of freedom, |t| of order 1)
  const double lx = y < 0.5 ? std::log1p(-y) : std::log(x);
  const double ly = x < 0.5 ? std::log1p(-x) : std::log(y);
  const double lbt = lnorm + a * lx + b * ly;
  if (x < (a + 1.0) / (a + b + 2.0)) {
    if (a >= 100.0) return std::exp(lbt) / betacf_even(a, b, x, y);
    return std::exp(lbt) * betacf(a, b, x) / a;
  }
  return 1.0 - std::exp(lbt) * betacf(b, a, y) / b;
}

}  // namespace

double chisq_upper_even(double x, int k);
double qnorm_lower(double p);
double pnorm_upper(double z);

// 2 * pt(|t|, df, lower.tail = FALSE)
double t_two_sided_p(double t, double df) {
  if (std::isnan(t) || std::isnan(df) || !(df > 0.0)) return std::numeric_limits<double>::quiet_NaN();
  if (std::isinf(t)) return 0.0;
  const double t2 = t * t;
  // I_x(df/2, 1/2) at x = df / (df + t^2): small p <=> small x, which betai evaluates directly (no 1 - ...)
  return betai(0.5 * df, 0.5, df / (df + t2), t2 / (df + t2));
}

// pbeta(x, a, b, lower.tail = FALSE) = I_{1 - x}(b, a): betai takes both arguments, so neither tail forms 1 - (1 - ...)
double beta_upper(double x, double a, double b) {
  if (std::isnan(x) || !(a > 0.0) || !(b > 0.0)) return std::numeric_limits<double>::quiet_NaN();
  return betai(b, a, 1.0 - x, x);
}

// pchisq(x, 2k, lower.tail = FALSE), k a positive integer
double chisq_upper_even(double x, int k) {
  if (std::isnan(x)) return x;
  if (!(x > 0.0)) return 1.0;
  const double h = 0.5 * x;
  double term = 1.0, sum = 1.0;
  for (int i = 1; i < k; ++i) {
    term *= h / i;
    sum += term;
  }
  return std::exp(-h) * sum;
}

// qnorm(p): Wichura (1988) AS241, PPND16
double qnorm_lower(double p) {
  if (std::isnan(p) || p < 0.0 || p > 1.0) return std::numeric_limits<double>::quiet_NaN();
  if (p == 0.0) return -std::numeric_limits<double>::infinity();
  if (p == 1.0) return std::numeric_limits<double>::infinity();
  const double q = p - 0.5;
  if (std::fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2509.0809287301226727 * r + 33430.575583588128105) * r + 67265.770927008700853) * r +
                            45921.953931549871457) * r + 13731.693765509461125) * r + 1971.5909503065514427) * r +
                          133.14166789178437745) * r + 3.387132872796366608);
    const double den = (((((((5226.495278852545925 * r + 28729.085735721942674) * r + 39307.89580009271061) * r +
                            21213.794301586595867) * r + 5394.1960214247511077) * r + 687.1870074920579083) * r +
                          42.313330701600911252) * r + 1.0);
    return q * num / den;
  }
  double r = q < 0.0 ? p : 1.0 - p;
  r = std::sqrt(-std::log(r));
  double val;
  if (r <= 5.0) {
    r -= 1.6;
    const double num = (((((((7.7454501427834140764e-4 * r + 0.0227238449892691845833) * r + 0.24178072517745061177) * r +
                            1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.7694972214606914055) * r +
                          4.6303378461565452959) * r + 1.42343711074968357734);
    const double den = (((((((1.05075007164441684324e-9 * r + 5.475938084995344946e-4) * r + 0.0151986665636164571966) * r +
                            0.14810397642748007459) * r + 0.68976733498510000455) * r + 1.6763848301838038494) * r +
                          2.05319162663775882187) * r + 1.0);
    val = num / den;
  } else {
    r -= 5.0;
    const double num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 0.0012426609473880784386) * r +
                            0.026532189526576123093) * r + 0.29656057182850489123) * r + 1.7848265399172913358) * r +
                          5.4637849111641143699) * r + 6.6579046435011037772);
    const double den = (((((((2.04426310338993978564e-15 * r + 1.4215117583164458887e-7) * r + 1.8463183175100546818e-5) * r +
                            7.868691311456132591e-4) * r + 0.0148753612908506148525) * r + 0.13692988092273580531) * r +
                          0.59983224619603520104) * r + 1.0);
    val = num / den;
    // polish in the far tail (two Newton steps on the tail probability, which erfc gives to full
    // relative accuracy): the rational approximation alone is good to ~1e-8 here
    const double tail = q < 0.0 ? p : 1.0 - p;   // P(Z > val)
    for (int it = 0; it < 2; ++it) {
      const double pt = 0.5 * std::erfc(val / std::sqrt(2.0));
      const double dens = std::exp(-0.5 * val * val) / std::sqrt(2.0 * M_PI);
      if (!(dens > 0.0)) break;
      val += (pt - tail) / dens;
    }
  }
  return q < 0.0 ? -val : val;
}

double pnorm_upper(double z) { return 0.5 * std::erfc(z / std::sqrt(2.0)); }

// stats::p.adjust(p, method = "fdr") (Benjamini-Hochberg); NaN stay NaN and do not count
void p_adjust_fdr(const double* p, int64_t m, double* q) {
  std::vector<int64_t> idx;
  idx.reserve(m);
  for (int64_t i = 0; i < m; ++i) {
    if (std::isnan(p[i])) q[i] = p[i];
    else idx.push_back(i);
  }
  const int64_t n = (int64_t)idx.size();
  std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return p[a] > p[b]; });   // decreasing
  double run = std::numeric_limits<double>::infinity();
  for (int64_t k = 0; k < n; ++k) {
    const int64_t i = idx[k];
    const double v = p[i] * (double)n / (double)(n - k);   // rank (n - k) in increasing order
    run = std::min(run, v);
    q[i] = std::min(1.0, run);
  }
}

// One set's tests.  k sets size, s1 = sum fc, s2 = sum fc^2 over the set; totals over all genes.
// R/plaid.R:476-486
double onesample_p(double k, double s1, double s2, double* mean_out) {
  const double meanx = s1 / (1e-8 + k);
  const double sdx = std::sqrt((s2 - meanx * meanx * k) / (k - 1.0));
  const double t = meanx / (1e-8 + sdx) * std::sqrt(k);
  *mean_out = meanx;
  return t_two_sided_p(std::fabs(t), std::max(k - 1.0, 1.0));
}

// R/plaid.R:488-520
double twosample_p(double g, double k, double s1, double s2, double tot1, double tot2, double* diff_out) {
  const double sum1 = k, sum0 = g - k;
  const double ssq1 = s2, ssq0 = tot2 - s2;
  const double mean1 = s1 / (1e-8 + sum1), mean0 = (tot1 - s1) / (1e-8 + sum0);
  const double var0 = (ssq0 - mean0 * mean0 * sum0) / (sum0 - 1.0);
  const double var1 = (ssq1 - mean1 * mean1 * sum1) / (sum1 - 1.0);
  const double varsum = var0 / sum0 + var1 / sum1;
  const double dof = varsum * varsum / (var0 / sum0 * (sum0 - 1.0) + var1 / sum1 * (sum1 - 1.0));
  const double f = mean1 - mean0;
  const double t = f / std::sqrt(varsum);
  *diff_out = f;
  return t_two_sided_p(std::fabs(t), std::max(dof, 1.0));
}

// Welch test from group means / sums of squared deviations (Rfast::ttests(x, ina), R/plaid.R:429)
double welch_p(double m0, double m1, double ssd0, double ssd1, double n0, double n1) {
  const double v0 = ssd0 / (n0 - 1.0), v1 = ssd1 / (n1 - 1.0);
  const double a = v0 / n0, b = v1 / n1;
  const double t = (m0 - m1) / std::sqrt(a + b);
  const double dof = (a + b) * (a + b) / (a * a / (n0 - 1.0) + b * b / (n1 - 1.0));
  return t_two_sided_p(std::fabs(t), dof);
}

// P1[is.na(P1)] <- 1; pmin(pmax(P1, 1e-99), 1 - 1e-99)   (R/plaid.R:441-446)
double clamp_p(double p) {
  if (std::isnan(p)) p = 1.0;
  return std::min(std::max(p, 1e-99), 1.0 - 1e-99);
}

// matrix_combine_p, R/plaid.R:522-537.  method 0 = fisher / sumlog, 1 = stouffer / sumz
double combine_p(const double* p, int np, int method) {
  if (method == 0) {
    double chisq = 0.0;
    for (int i = 0; i < np; ++i) chisq += std::log(p[i]);
    return chisq_upper_even(-2.0 * chisq, np);
  }
  double zz = 0.0;
  for (int i = 0; i < np; ++i) zz += -qnorm_lower(p[i]);   // qnorm(p, lower.tail = FALSE)
  return pnorm_upper(zz / std::sqrt((double)np));
}


// ---- plaid.limma (include/plaidhip.h: plaidhip_limma): the design on the host, the empirical-Bayes tail --------------------

namespace {

// digamma, trigamma and tetragamma in plain fp64: the recurrence up to an argument >= 10, then the asymptotic series
double lm_digamma(double x) {
  double s = 0.0;
  while (x < 10.0) { s -= 1.0 / x; x += 1.0; }
  const double i2 = 1.0 / (x * x);
  const double tail = i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0 -
                      i2 * (691.0 / 32760.0 - i2 * (1.0 / 12.0)))))));
  return s + (std::log(x) - 0.5 / x - tail);
}

double lm_trigamma(double x) {
  double s = 0.0;
  while (x < 10.0) { s += 1.0 / (x * x); x += 1.0; }
  const double i1 = 1.0 / x, i2 = i1 * i1;
  const double tail = i1 * i2 * (1.0 / 6.0 - i2 * (1.0 / 30.0 - i2 * (1.0 / 42.0 - i2 * (1.0 / 30.0 - i2 * (5.0 / 66.0 -
                      i2 * (691.0 / 2730.0 - i2 * (7.0 / 6.0)))))));
  return s + (i1 + 0.5 * i2 + tail);
}

double lm_tetragamma(double x) {   // (only steers the Newton steps below: the root does not depend on its last bits)
  double s = 0.0;
  while (x < 10.0) { s -= 2.0 / (x * x * x); x += 1.0; }
  const double i1 = 1.0 / x, i2 = i1 * i1;
  return s - i2 * (1.0 + i1 + i2 * (0.5 - i2 * (1.0 / 6.0 - i2 * (1.0 / 6.0 - i2 * (3.0 / 10.0 - i2 * (5.0 / 6.0))))));
}

// y with trigamma(y) = v, v > 0: limma's closed forms at the two ends, else Newton on 1 / trigamma from 0.5 + 1 / v (the
// function is convex there, so the steps rise monotonically to the root); stopped when a step is below 1e-14 y
double lm_trigamma_inverse(double v) {
  if (v > 1e7) return 1.0 / std::sqrt(v);
  if (v < 1e-6) return 1.0 / v;
  double y = 0.5 + 1.0 / v;
  for (int it = 0; it < 60; ++it) {
    const double tri = lm_trigamma(y);
    const double dif = tri * (1.0 - tri / v) / lm_tetragamma(y);
    y += dif;
    if (!(std::fabs(dif) > 1e-14 * y)) break;
  }
  return y;
}

constexpr int kLimmaThreads = 8;              // host threads of the tails and of the Benjamini-Hochberg columns, at most
constexpr int64_t kLimmaWork = 1 << 15;       // rows per thread below which another thread is not worth its start

// fn(t, nth) on nth threads (t = 0 .. nth - 1); false: a thread could not be started or ran out of memory
template <typename Fn>
bool lm_threads(int64_t nth, Fn&& fn) {
  if (nth <= 1) { fn((int64_t)0, (int64_t)1); return true; }
  std::vector<std::thread> th;
  std::atomic<int> failed{0};
  try {
    for (int64_t t = 0; t < nth; ++t)
      th.emplace_back([&, t] {
        try { fn(t, nth); } catch (...) { failed.store(1); }
      });
  } catch (...) { failed.store(1); }
  for (auto& t : th) t.join();
  return failed.load() == 0;
}

}  // namespace

int limma_design(const char* what, const double* D, int32_t n, int32_t p, const int8_t* use, const double* K, int32_t q,
                 int32_t fit, double* Q, double* R, double* v, double* u, int64_t* nf_out, double* Q2) {
  std::vector<int32_t> sel;
  for (int32_t c = 0; c < n; ++c)
    if (use == nullptr || use[c] != 0) sel.push_back(c);
  const int64_t nf = (int64_t)sel.size();
  for (int64_t i = 0; i < nf; ++i)
    for (int32_t k = 0; k < p; ++k)
      PH_REQUIRE(std::isfinite(D[(int64_t)k * n + sel[(size_t)i]]), "%s: the design of fit %d is not finite at sample %d, column %d",
                 what, fit, sel[(size_t)i] + 1, k + 1);
  PH_REQUIRE(nf - p >= 1, "%s: fit %d has %lld samples for %d coefficients (at least %d: no residual degree of freedom)", what,
             fit, (long long)nf, p, p + 1);
  std::vector<double> a((size_t)nf * p), v0((size_t)p), vn((size_t)p), Rm((size_t)p * p, 0.0);
  for (int32_t k = 0; k < p; ++k)
    for (int64_t i = 0; i < nf; ++i) a[(size_t)(k * nf + i)] = D[(int64_t)k * n + sel[(size_t)i]];
  for (int32_t k = 0; k < p; ++k) {
    double* x = a.data() + (size_t)k * nf;
    double col2 = 0.0, sub2 = 0.0;
    for (int64_t i = 0; i < nf; ++i) col2 += D[(int64_t)k * n + sel[(size_t)i]] * D[(int64_t)k * n + sel[(size_t)i]];
    for (int64_t i = k; i < nf; ++i) sub2 += x[i] * x[i];
    const double alpha = x[k] >= 0.0 ? -std::sqrt(sub2) : std::sqrt(sub2);
    PH_REQUIRE(std::fabs(alpha) > 1e-7 * std::sqrt(col2),
               "%s: column %d of the design of fit %d is rank-deficient (|R_kk| = %g, the column's norm %g)", what, k + 1, fit,
               std::fabs(alpha), std::sqrt(col2));
    // the reflector's vector x - alpha e_1 stays in x[k ..], its first entry in v0 and its squared norm in vn
    v0[(size_t)k] = x[k] - alpha;
    double n2 = v0[(size_t)k] * v0[(size_t)k];
    for (int64_t i = k + 1; i < nf; ++i) n2 += x[i] * x[i];
    vn[(size_t)k] = n2;
    for (int32_t j = k + 1; j < p; ++j) {
      double* y = a.data() + (size_t)j * nf;
      double dot = v0[(size_t)k] * y[k];
      for (int64_t i = k + 1; i < nf; ++i) dot += x[i] * y[i];
      const double s = 2.0 * dot / n2;
      y[k] -= s * v0[(size_t)k];
      for (int64_t i = k + 1; i < nf; ++i) y[i] -= s * x[i];
    }
    Rm[(size_t)k * p + k] = alpha;
    for (int32_t j = k + 1; j < p; ++j) Rm[(size_t)j * p + k] = a[(size_t)j * nf + k];
  }
  if (Q != nullptr) {   // the thin Q: the reflectors applied to the first p columns of the identity, last reflector first
    std::vector<double> qs((size_t)nf * p, 0.0);
    for (int32_t j = 0; j < p; ++j) qs[(size_t)j * nf + j] = 1.0;
    for (int32_t k = p - 1; k >= 0; --k) {
      const double* x = a.data() + (size_t)k * nf;
      for (int32_t j = k; j < p; ++j) {
        double* y = qs.data() + (size_t)j * nf;
        double dot = v0[(size_t)k] * y[k];
        for (int64_t i = k + 1; i < nf; ++i) dot += x[i] * y[i];
        const double s = 2.0 * dot / vn[(size_t)k];
        y[k] -= s * v0[(size_t)k];
        for (int64_t i = k + 1; i < nf; ++i) y[i] -= s * x[i];
      }
    }
    std::fill(Q, Q + (size_t)n * p, 0.0);
    for (int32_t k = 0; k < p; ++k)
      for (int64_t i = 0; i < nf; ++i) Q[(int64_t)k * n + sel[(size_t)i]] = qs[(size_t)k * nf + i];
  }
  if (Q2 != nullptr) {   // the other n_f - p columns of the full Q (plaid.fry): every reflector, last first, on e_p .. e_{n_f - 1}
    const int64_t d = nf - p;
    std::vector<double> y((size_t)nf);
    std::fill(Q2, Q2 + (size_t)n * d, 0.0);
    for (int64_t j = 0; j < d; ++j) {
      std::fill(y.begin(), y.end(), 0.0);
      y[(size_t)(p + j)] = 1.0;
      for (int32_t k = p - 1; k >= 0; --k) {
        const double* x = a.data() + (size_t)k * nf;
        double dot = v0[(size_t)k] * y[(size_t)k];
        for (int64_t i = k + 1; i < nf; ++i) dot += x[i] * y[(size_t)i];
        const double s = 2.0 * dot / vn[(size_t)k];
        y[(size_t)k] -= s * v0[(size_t)k];
        for (int64_t i = k + 1; i < nf; ++i) y[(size_t)i] -= s * x[i];
      }
      for (int64_t i = 0; i < nf; ++i) Q2[j * n + sel[(size_t)i]] = y[(size_t)i];
    }
  }
  if (R != nullptr) std::copy(Rm.begin(), Rm.end(), R);
  if (nf_out != nullptr) *nf_out = nf;
  std::vector<double> vj((size_t)p);
  for (int32_t j = 0; j < q && (v != nullptr || u != nullptr); ++j) {   // R' v_j = K_j, forward; u_j = |v_j|
    double s2 = 0.0;
    for (int32_t i = 0; i < p; ++i) {
      double acc = K != nullptr ? K[(size_t)j * p + i] : (i == j ? 1.0 : 0.0);
      for (int32_t l = 0; l < i; ++l) acc -= Rm[(size_t)i * p + l] * vj[(size_t)l];
      vj[(size_t)i] = acc / Rm[(size_t)i * p + i];
      s2 += vj[(size_t)i] * vj[(size_t)i];
    }
    if (v != nullptr) std::copy(vj.begin(), vj.end(), v + (size_t)j * p);
    if (u != nullptr) u[j] = std::sqrt(s2);
  }
  return PLAIDHIP_OK;
}

// squeezeVar of one fit (step 3 of plaid.limma), for plaid.limma's tables and for plaid.fry's divisors: s[r] = rss[r] / d_r,
// the prior (d0, s0^2) from the ok rows, po[r] = s2.post (NaN for a row that is not ok).  dr == nullptr: every row has d = dfit.
LimmaPrior limma_squeeze_fit(size_t R, double dfit, const double* dr, const double* rssf, double* s, double* po) {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::vector<double> xs;
  double d = dfit, dsum = 0.0;   // d: the ok rows' residual df where they share one
  bool alleq = true;
  for (size_t r = 0; r < R; ++r) {
    const double di = dr != nullptr ? dr[r] : dfit;
    s[r] = rssf[r] / di;
    if (!std::isfinite(s[r])) continue;
    if (dr != nullptr) {
      if (xs.empty()) d = di;
      else if (di != d) alleq = false;
      dsum += di;
    }
    xs.push_back(s[r]);
  }
  const int64_t nok = (int64_t)xs.size();
  const double pool = alleq ? (double)nok * d : dsum;   // df.pooled
  double d0 = 0.0, s0 = nan;
  if (nok >= 2) {
    const size_t h = (size_t)nok / 2;
    std::nth_element(xs.begin(), xs.begin() + h, xs.end());
    double med = xs[h];
    if (nok % 2 == 0) med = (*std::max_element(xs.begin(), xs.begin() + h) + med) / 2.0;
    if (med == 0.0) med = 1.0;
    const double floor_x = 1e-5 * med, shift = -lm_digamma(0.5 * d) + std::log(0.5 * d);
    double esum = 0.0, xsum = 0.0, trisum = 0.0;
    std::vector<double> e;
    e.reserve((size_t)nok);
    for (size_t r = 0; r < R; ++r) {   // (in row order: the sums below are pinned as ascending)
      if (!std::isfinite(s[r])) continue;
      const double x = std::max(s[r], floor_x);
      if (alleq) {
        e.push_back(std::log(x) + shift);
      } else {
        e.push_back(std::log(x) + (-lm_digamma(0.5 * dr[r]) + std::log(0.5 * dr[r])));
        trisum += lm_trigamma(0.5 * dr[r]);
      }
      esum += e.back();
      xsum += x;
    }
    const double ebar = esum / (double)nok;
    double ss = 0.0;
    for (double ei : e) ss += (ei - ebar) * (ei - ebar);
    const double var = ss / (double)(nok - 1) - (alleq ? lm_trigamma(0.5 * d) : trisum / (double)nok);
    if (var > 0.0) {
      const double y = lm_trigamma_inverse(var);
      d0 = 2.0 * y;
      s0 = std::exp(ebar + lm_digamma(y) - std::log(y));
    } else {
      d0 = inf;
      s0 = xsum / (double)nok;
    }
  }
  for (size_t r = 0; r < R; ++r) {
    const double di = dr != nullptr ? dr[r] : dfit;
    po[r] = !std::isfinite(s[r]) ? nan : std::isinf(d0) ? s0 : d0 == 0.0 ? s[r] : (di * s[r] + d0 * s0) / (di + d0);
  }
  return LimmaPrior{d0, s0, pool, nok};
}

// plaid.fry's divisors (include/plaidhip.h: plaidhip_fry, step 1): c_g = sqrt(s2.post), sqrt(s2) or 1.0 of an ok gene; a
// divisor that is 0 or not finite, and every gene that is not ok, becomes NaN: the gene is outside the fit's universe
void fry_divisors(int32_t rows, int32_t p, int32_t nfit, const double* rss, const int64_t* nf, int standardize, double* cg) {
  const size_t R = (size_t)rows;
  std::vector<double> s(R), po(R);
  for (int32_t f = 0; f < nfit; ++f) {
    limma_squeeze_fit(R, (double)(nf[f] - p), nullptr, rss + R * f, s.data(), po.data());
    for (size_t r = 0; r < R; ++r) {
      double c = std::numeric_limits<double>::quiet_NaN();
      if (std::isfinite(s[r]))
        c = standardize == PLAIDHIP_FRY_STANDARDIZE_POSTERIOR ? std::sqrt(po[r])
            : standardize == PLAIDHIP_FRY_STANDARDIZE_RESIDUAL ? std::sqrt(s[r]) : 1.0;
      cg[R * f + r] = fry_in_universe(c) ? c : std::numeric_limits<double>::quiet_NaN();
    }
  }
}

// Philox4x32-10 (Salmon et al. 2011): one block of four words from a counter and a key
static void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// A sum of squares in double-double, fp64 operations only (the same bits on every IEEE host): a square is split exactly
// into its rounded product and the fma's remainder, the sum runs through Knuth's two-sum; root() is sqrt(hi) corrected once
// by (hi - s0 s0 + lo) / (2 s0), the residual taken with an fma.
struct DoubleSum {
  double hi = 0.0, lo = 0.0;
  void add_square(double x) {
#pragma clang fp contract(off)
    const double pr = x * x, pe = std::fma(x, x, -pr);
    const double s = hi + pr, bb = s - hi;
    const double err = (hi - (s - bb)) + (pr - bb);
    hi = s;
    lo += err + pe;
  }
  double root() const {
#pragma clang fp contract(off)
    const double s0 = std::sqrt(hi);
    if (!(s0 > 0.0)) return s0;
    const double res = std::fma(-s0, s0, hi) + lo;
    return s0 + res / (2.0 * s0);
  }
};

// plaid.roast's standard normal of (seed, fit, rotation k, index i) (include/plaidhip.h: plaidhip_roast, step 2)
static double roast_normal(uint64_t seed, int32_t fit, int32_t k, int32_t i) {
  const uint32_t ctr[4] = {(uint32_t)i, (uint32_t)k, (uint32_t)fit, 0x726f6173u};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t x[4];
  philox4x32_10(ctr, key, x);
  const double u1 = (double)(((((uint64_t)x[0] << 32) | x[1]) >> 11) + 1) * 0x1p-53;
  const double u2 = (double)((((uint64_t)x[2] << 32) | x[3]) >> 11) * 0x1p-53;
  return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586476925286766559 * u2);
}

// plaid.roast, step 2: W ((n + 1) x nrot row-major) of one fit from its thin Q (n x p column-major, 0.0 on the samples left
// out); rotations dealt to the threads, each a function of (seed, fit, k) alone
void roast_rotations(const double* Q, int32_t n, int32_t p, const int8_t* use, int32_t fit, int32_t nrot, uint64_t seed,
                     double* W) {
  auto work = [&](int64_t t, int64_t nth) {
    std::vector<double> nu((size_t)n), a((size_t)p);
    for (int64_t k = nrot * t / nth; k < nrot * (t + 1) / nth; ++k) {
      const double nu0 = roast_normal(seed, fit, (int32_t)k, 0);
      for (int32_t c = 0; c < n; ++c) nu[(size_t)c] = use == nullptr || use[c] != 0 ? roast_normal(seed, fit, (int32_t)k, c + 1) : 0.0;
      for (int32_t j = 0; j < p; ++j) {
        double acc = 0.0;
        for (int32_t c = 0; c < n; ++c) acc += Q[(size_t)j * n + c] * nu[(size_t)c];
        a[(size_t)j] = acc;
      }
      DoubleSum ss;   // (double-double: s is the rounded root of the exact sum but for a part in 2^100)
      ss.add_square(nu0);
      for (int32_t c = 0; c < n; ++c) {
        if (use != nullptr && use[c] == 0) continue;
        double proj = 0.0;
        for (int32_t j = 0; j < p; ++j) proj += Q[(size_t)j * n + c] * a[(size_t)j];
        nu[(size_t)c] -= proj;
        ss.add_square(nu[(size_t)c]);
      }
      const double s = ss.root();
      W[k] = nu0 / s;
      for (int32_t c = 0; c < n; ++c) W[(size_t)(c + 1) * nrot + k] = use == nullptr || use[c] != 0 ? nu[(size_t)c] / s : 0.0;
    }
  };
  const int64_t nth = std::max<int64_t>(1, std::min<int64_t>({(int64_t)kLimmaThreads, (int64_t)nrot * n * p / kLimmaWork}));
  if (!lm_threads(nth, work)) work(0, 1);   // (no thread to be had: on the calling one)
}

// Step 3 of plaid.limma and its tables.  drow == nullptr is plaidhip_limma_finish: every row of fit f has d = n_f - p and
// the fit's u_j.  Otherwise (plaidhip_limma_finish_na) row r of fit f has d_r = drow[f][r] (NaN: not fitted) and its own
// u_j, and squeezeVar's moments take a vector df1; where all ok rows share one d the operations are those of the first form.
int limma_finish_rows(const char* what, int32_t rows, int32_t p, int32_t nfit, int32_t q, const double* E, const double* rss,
                      const int64_t* nf, const double* v, const double* u, const double* drow, const double* urow, double* out,
                      double* hyper, int hcols) {
  PH_REQUIRE(rows >= 0 && nfit >= 0 && q >= 0, "%s: bad dims rows=%d nfit=%d q=%d", what, rows, nfit, q);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "%s: p = %d coefficients (1 <= p <= %d)", what, p, PLAIDHIP_LIMMA_MAX_COEF);
  if (rows == 0 || nfit == 0 || q == 0) return PLAIDHIP_OK;
  PH_REQUIRE(E && rss && nf && v && u && out && hyper, "%s: null argument", what);
  for (int32_t f = 0; f < nfit; ++f)
    PH_REQUIRE(nf[f] - p >= 1, "%s: fit %d has %lld samples for %d coefficients", what, f + 1, (long long)nf[f], p);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const size_t R = (size_t)rows;
  // per fit: s2, the prior, s2.post and df.total
  std::vector<double> s2(R * nfit), post(R * nfit), d0s((size_t)nfit), pooled((size_t)nfit);
  for (int32_t f = 0; f < nfit; ++f) {
    const double dfit = (double)(nf[f] - p);
    const LimmaPrior pr = limma_squeeze_fit(R, dfit, drow != nullptr ? drow + R * f : nullptr, rss + R * f, s2.data() + R * f,
                                            post.data() + R * f);
    hyper[(size_t)hcols * f] = dfit;
    hyper[(size_t)hcols * f + 1] = pr.d0;
    hyper[(size_t)hcols * f + 2] = pr.s0;
    hyper[(size_t)hcols * f + 3] = (double)pr.nok;
    if (hcols > 4) hyper[(size_t)hcols * f + 4] = pr.pool;
    d0s[(size_t)f] = pr.d0;
    pooled[(size_t)f] = pr.pool;
  }
  // logFC, AveExpr, t, P.Value and sigma2 of every (fit, contrast, row): row chunks dealt to the threads
  const int64_t ncol = (int64_t)nfit * q, items = ncol * rows;
  const int32_t W1 = p + 1;
  auto tails = [&](int64_t t, int64_t nth) {
    const int64_t lo = items * t / nth, hi = items * (t + 1) / nth;
    for (int64_t e = lo; e < hi; ++e) {
      const int64_t col = e / rows;
      const size_t r = (size_t)(e % rows);
      const int32_t f = (int32_t)(col / q), j = (int32_t)(col % q);
      double* o = out + (size_t)col * 6 * R;
      const double sr = s2[R * f + r];
      if (!std::isfinite(sr)) {
        for (int c = 0; c < 6; ++c) o[(size_t)c * R + r] = nan;
        continue;
      }
      const double* vj = v + ((size_t)f * q + j) * p;
      double fc = 0.0;
      for (int32_t k = 0; k < p; ++k) fc = std::fma(vj[k], E[((size_t)f * W1 + k) * R + r], fc);
      const double uj = urow != nullptr ? urow[(size_t)col * R + r] : u[(size_t)f * q + j];
      const double di = drow != nullptr ? drow[R * f + r] : (double)(nf[f] - p);
      const double d0 = d0s[(size_t)f], pool = pooled[(size_t)f];
      const double tt = fc / (uj * std::sqrt(post[R * f + r]));
      o[r] = fc;
      o[R + r] = E[((size_t)f * W1 + p) * R + r];
      o[2 * R + r] = tt;
      o[3 * R + r] = t_two_sided_p(tt, std::isinf(d0) ? pool : std::min(di + d0, pool));
      o[5 * R + r] = sr;
    }
  };
  const int64_t nth = std::max<int64_t>(1, std::min<int64_t>({(int64_t)kLimmaThreads, items / kLimmaWork}));
  if (!lm_threads(nth, tails)) { set_error("out of host memory"); return PLAIDHIP_ENOMEM; }
  auto adjust = [&](int64_t t, int64_t nt) {
    for (int64_t col = t; col < ncol; col += nt) {
      double* o = out + (size_t)col * 6 * R;
      p_adjust_fdr(o + 3 * R, rows, o + 4 * R);
    }
  };
  const int64_t nbh = std::max<int64_t>(1, std::min<int64_t>({(int64_t)kLimmaThreads, items / kLimmaWork, ncol}));
  if (!lm_threads(nbh, adjust)) { set_error("out of host memory"); return PLAIDHIP_ENOMEM; }
  return PLAIDHIP_OK;
}

// ---- plaid.rankcor: the pinned epilogues (include/plaidhip.h: plaidhip_rankcor) -------------------------
namespace {

typedef unsigned __int128 u128;

// an unsigned 128-bit integer to the nearest double, ties to even, in one rounding: the top 64 bits with the bits below
// them folded into the last one (far below the 53 that are kept), converted by the hardware and scaled by a power of two
double u128_to_double(u128 v) {
  const uint64_t hi = (uint64_t)(v >> 64), lo = (uint64_t)v;
  if (hi == 0) return (double)lo;
  const int shift = 64 - __builtin_clzll(hi);   // 1 .. 64: the bits above 64
  uint64_t top = (uint64_t)(v >> shift);
  if ((v & ((((u128)1) << shift) - 1)) != 0) top |= 1ull;
  return std::ldexp((double)top, shift);
}

}  // namespace

void rankcor_rank_epilogue(int64_t n, int64_t T1, int64_t T2, int64_t k, int64_t A, double* o) {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  o[0] = o[1] = o[2] = nan;
  if (n <= 1 || k <= 0 || k >= n) return;
  const int64_t num = n * A - k * T1;
  const u128 D = (u128)(uint64_t)n * (u128)(uint64_t)T2 - (u128)(uint64_t)T1 * (u128)(uint64_t)T1;
  const u128 P = (u128)((uint64_t)k * (uint64_t)(n - k)) * D;
  if (P == 0) return;
  const uint64_t an = (uint64_t)(num < 0 ? -num : num);
  const u128 num2 = (u128)an * (u128)an;
  const u128 Q = P - num2;
  if (Q == 0) {
    o[0] = num < 0 ? -1.0 : 1.0;
    if (n > 2) { o[1] = num < 0 ? -inf : inf; o[2] = 0.0; }
    return;
  }
  o[0] = (double)num / std::sqrt(u128_to_double(P));
  if (n <= 2) return;
  const double tsq = ((double)(n - 2) * u128_to_double(num2)) / u128_to_double(Q);
  const double t = std::copysign(std::sqrt(tsq), (double)num);
  o[1] = t;
  o[2] = 2.0 * pnorm_upper(std::fabs(t));
}

void rankcor_value_epilogue(int64_t n, double T1, double T2, int flag, int64_t k, double A, double* o) {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  o[0] = o[1] = o[2] = nan;
  if (flag != 0 || n <= 1 || k <= 0 || k >= n) return;
  const double nd = (double)n, kd = (double)k;
  const double num = A - (kd * T1) / nd;
  const double den = std::sqrt(((kd * (double)(n - k)) / nd) * (T2 - (T1 * T1) / nd));
  if (!(den > 0.0) || !std::isfinite(den)) return;
  const double rho = num / den;
  o[0] = rho;
  if (n <= 2 || rho != rho) return;
  const double w = (1.0 - rho) * (1.0 + rho);
  if (w <= 0.0) {
    o[1] = std::copysign(inf, rho);
    o[2] = 0.0;
    return;
  }
  const double t = rho * std::sqrt((double)(n - 2) / w);
  o[1] = t;
  o[2] = 2.0 * pnorm_upper(std::fabs(t));
}

}  // namespace plaidhip

extern "C" {

int plaidhip_rankcor_finish(int32_t m, int32_t c, const int64_t* n, const int64_t* T1, const int64_t* T2, const int64_t* k,
                            const int64_t* A, double* out) try {
  using namespace plaidhip;
  PH_REQUIRE(m >= 0 && c >= 0, "rankcor_finish: bad dims m=%d c=%d", m, c);
  if (m == 0 || c == 0) return PLAIDHIP_OK;
  PH_REQUIRE(n && T1 && T2 && k && A && out, "rankcor_finish: null argument");
  for (int32_t l = 0; l < c; ++l) {
    PH_REQUIRE(n[l] >= 0 && n[l] <= PLAIDHIP_RANKCOR_MAX_GENES && T1[l] >= 0 && T2[l] >= 0 &&
                   T1[l] <= 2 * n[l] * n[l] && T2[l] <= 4 * n[l] * n[l] * n[l],
               "rankcor_finish: list %d: n = %lld, T1 = %lld, T2 = %lld", l + 1, (long long)n[l], (long long)T1[l],
               (long long)T2[l]);
    PH_REQUIRE((unsigned __int128)n[l] * (unsigned __int128)T2[l] >= (unsigned __int128)T1[l] * (unsigned __int128)T1[l],
               "rankcor_finish: list %d: n T2 < T1^2", l + 1);
    for (int32_t j = 0; j < m; ++j) {
      const int64_t kk = k[(size_t)l * m + j], a = A[(size_t)l * m + j];
      PH_REQUIRE(kk >= 0 && kk <= n[l] && a >= 0 && a <= T1[l], "rankcor_finish: list %d, set %d: k = %lld, A = %lld", l + 1, j + 1,
                 (long long)kk, (long long)a);
      const unsigned __int128 D = (unsigned __int128)n[l] * (unsigned __int128)T2[l] - (unsigned __int128)T1[l] * (unsigned __int128)T1[l];
      const int64_t num = n[l] * a - kk * T1[l];
      const unsigned __int128 an = (unsigned __int128)(num < 0 ? -num : num);
      PH_REQUIRE((unsigned __int128)(kk * (n[l] - kk)) * D >= an * an, "rankcor_finish: list %d, set %d: P < num^2", l + 1, j + 1);
    }
  }
  for (int32_t l = 0; l < c; ++l) {
    double* o = out + (size_t)l * 5 * m;
    for (int32_t j = 0; j < m; ++j) {
      double r[3];
      rankcor_rank_epilogue(n[l], T1[l], T2[l], k[(size_t)l * m + j], A[(size_t)l * m + j], r);
      o[j] = (double)k[(size_t)l * m + j];
      o[(size_t)m + j] = r[0];
      o[2 * (size_t)m + j] = r[1];
      o[3 * (size_t)m + j] = r[2];
    }
    p_adjust_fdr(o + 3 * (size_t)m, m, o + 4 * (size_t)m);
  }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_design(const double* D, int32_t n, int32_t p, const int8_t* use, const double* K, int32_t q, int32_t fit,
                          double* Q, double* R, double* v, double* u, int64_t* nf) try {
  using namespace plaidhip;
  PH_REQUIRE(n >= 0 && q >= 0, "limma_design: bad dims n=%d q=%d", n, q);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "limma_design: p = %d coefficients (1 <= p <= %d)", p,
             PLAIDHIP_LIMMA_MAX_COEF);
  PH_REQUIRE(K != nullptr || q == p, "limma_design: q = %d without K (the p = %d unit vectors)", q, p);
  PH_REQUIRE(D != nullptr || n == 0, "limma_design: null design");
  if (K != nullptr)
    for (int64_t e = 0; e < (int64_t)p * q; ++e)
      PH_REQUIRE(std::isfinite(K[e]), "limma_design: K[%lld] = %g (the contrasts are finite)", (long long)e, K[e]);
  return limma_design("limma_design", D, n, p, use, K, q, fit, Q, R, v, u, nf);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_finish(int32_t rows, int32_t p, int32_t nfit, int32_t q, const double* E, const double* rss,
                          const int64_t* nf, const double* v, const double* u, double* out, double* hyper) try {
  return plaidhip::limma_finish_rows("limma_finish", rows, p, nfit, q, E, rss, nf, v, u, nullptr, nullptr, out, hyper, 4);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_finish_na(int32_t rows, int32_t p, int32_t nfit, int32_t q, const double* E, const double* rss,
                             const int64_t* nf, const double* v, const double* drow, const double* urow, double* out,
                             double* hyper) try {
  using namespace plaidhip;
  PH_REQUIRE(rows == 0 || nfit == 0 || q == 0 || (drow != nullptr && urow != nullptr), "limma_finish_na: null argument");
  return limma_finish_rows("limma_finish_na", rows, p, nfit, q, E, rss, nf, v, urow, drow, urow, out, hyper, 5);
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_na_solve(int32_t p, int32_t nmis, const double* qmis, const double* Ep, int64_t nobs, const double* v,
                            int32_t q, double* gamma, double* u, double* pivots, int32_t* ok) try {
  using namespace plaidhip;
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_NA_MAX_COEF, "limma_na_solve: p = %d coefficients (1 <= p <= %d)", p,
             PLAIDHIP_LIMMA_NA_MAX_COEF);
  PH_REQUIRE(nmis >= 0 && q >= 0, "limma_na_solve: bad dims nmis=%d q=%d", nmis, q);
  PH_REQUIRE((qmis || nmis == 0) && Ep && (v || q == 0) && gamma && (u || q == 0) && ok, "limma_na_solve: null argument");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  constexpr int P = PLAIDHIP_LIMMA_NA_MAX_COEF;
  double H[P * P], w[P];
  for (int k = 0; k < p; ++k)
    for (int l = 0; l <= k; ++l) H[k * P + l] = (k == l ? 1.0 : 0.0) - lmfit_na_gram_chain(qmis + k, qmis + l, p, nmis);
  double piv[P];
  for (int k = 0; k < p; ++k) piv[k] = nan;
  *ok = lmfit_na_factor_solve(p, H, P, Ep, gamma, piv, PLAIDHIP_LMNA_PIVOT_MIN, false) && nobs - p >= 1 ? 1 : 0;
  if (!*ok)
    for (int k = 0; k < p; ++k) gamma[k] = nan;
  if (pivots != nullptr) std::copy(piv, piv + p, pivots);
  for (int32_t j = 0; j < q; ++j) u[j] = *ok ? lmfit_na_unscaled(p, H, P, v + (size_t)j * p, w) : nan;
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_lowess(const double* x, const double* y, int64_t n, double f, int32_t iter, double delta, double* ys,
                    int8_t* anchor) try {
  using namespace plaidhip;
  PH_REQUIRE(n >= 1 && iter >= 0, "lowess: bad dims n=%lld iter=%d", (long long)n, iter);
  PH_REQUIRE(x && y && ys, "lowess: null argument");
  PH_REQUIRE(f > 0.0 && std::isfinite(f) && delta >= 0.0, "lowess: f = %g, delta = %g (f > 0, delta >= 0)", f, delta);
  for (int64_t i = 0; i < n; ++i) {
    PH_REQUIRE(std::isfinite(x[i]) && std::isfinite(y[i]), "lowess: point %lld is not finite", (long long)i + 1);
    PH_REQUIRE(i == 0 || x[i] >= x[i - 1], "lowess: x is not ascending at point %lld", (long long)i + 1);
  }
  lowess_run(x, y, n, f, iter, delta, ys, anchor);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_w_solve(int32_t p, const double* Htri, const double* b, int64_t nlive, const double* v, int32_t q,
                           double* gamma, double* u, double* pivots, int32_t* ok) try {
  using namespace plaidhip;
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_NA_MAX_COEF, "limma_w_solve: p = %d coefficients (1 <= p <= %d)", p,
             PLAIDHIP_LIMMA_NA_MAX_COEF);
  PH_REQUIRE(q >= 0 && nlive >= 0, "limma_w_solve: bad dims q=%d nlive=%lld", q, (long long)nlive);
  PH_REQUIRE(Htri && b && (v || q == 0) && gamma && (u || q == 0) && ok, "limma_w_solve: null argument");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  constexpr int P = PLAIDHIP_LIMMA_NA_MAX_COEF;
  double H[P * P], g[P], w[P], piv[P];
  for (int k = 0, j = 0; k < p; ++k) {
    for (int l = 0; l <= k; ++l, ++j) H[k * P + l] = Htri[j];
    g[k] = b[k];
    piv[k] = nan;
  }
  *ok = lmfit_w_row_solve(p, H, P, g, (double)nlive, v, q, u, 1, w, piv) ? 1 : 0;
  for (int k = 0; k < p; ++k) gamma[k] = *ok ? g[k] : nan;
  if (!*ok)
    for (int32_t j = 0; j < q; ++j) u[j] = nan;
  if (pivots != nullptr) std::copy(piv, piv + p, pivots);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// plaid.camera, step 2 for one gene (include/plaidhip.h): the functions the device runs (camera.h)
int plaidhip_camera_residual_row(int32_t n, int32_t p, const double* x, const double* Q, const int8_t* use, const double* E,
                                 double rss, double d, double* z) try {
  using namespace plaidhip;
  PH_REQUIRE(n >= 0, "camera_residual_row: bad dims n=%d", n);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "camera_residual_row: p = %d coefficients (1 <= p <= %d)", p,
             PLAIDHIP_LIMMA_MAX_COEF);
  PH_REQUIRE(d >= 1.0, "camera_residual_row: d = %g residual degrees of freedom (at least 1)", d);
  if (n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(x && Q && E && z, "camera_residual_row: null argument");
  const double scale = camera_gene_scale(rss, d);
  for (int32_t c = 0; c < n; ++c) {
    double r = x[c];
    for (int32_t k = 0; k < p; ++k) r = camera_chain_step(Q[(size_t)k * n + c], E[k], r);
    z[c] = camera_standardise(r, scale, use == nullptr || use[c] != 0);
  }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// plaid.camera, step 5 (include/plaidhip.h): the test of every (fit, contrast, set), fp64, every sum over the genes in
// ascending order
int plaidhip_camera_finish(int32_t g, int32_t m, int32_t nfit, int32_t q, const double* t, const int8_t* ok, const double* sumt,
                           const double* cnt, const double* ss, const double* dfres, const double* dfprior,
                           double inter_gene_cor, int allow_neg_cor, double* out, double* gdf) try {
  using namespace plaidhip;
  PH_REQUIRE(g >= 0 && m >= 0 && nfit >= 0 && q >= 0, "camera_finish: bad dims g=%d m=%d nfit=%d q=%d", g, m, nfit, q);
  if (nfit == 0) return PLAIDHIP_OK;
  PH_REQUIRE(dfres && dfprior && gdf, "camera_finish: null argument");
  PH_REQUIRE(g == 0 || ok, "camera_finish: null argument");
  PH_REQUIRE(m == 0 || q == 0 || ((g == 0 || t) && sumt && cnt && out), "camera_finish: null argument");
  PH_REQUIRE(ss != nullptr || (inter_gene_cor > -1.0 && inter_gene_cor < 1.0),
             "camera_finish: inter_gene_cor = %g without sums of squares (a correlation inside (-1, 1))", inter_gene_cor);
  for (int32_t f = 0; f < nfit; ++f)
    PH_REQUIRE(dfres[f] >= 1.0 && dfprior[f] >= 0.0, "camera_finish: fit %d: df.residual = %g, df.prior = %g", f + 1, dfres[f],
               dfprior[f]);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const size_t R = (size_t)g, M = (size_t)m;
  for (int32_t f = 0; f < nfit; ++f) {
    const int8_t* okf = ok + R * f;
    int64_t Gn = 0;
    for (size_t r = 0; r < R; ++r) Gn += okf[r] != 0 ? 1 : 0;
    const double G = (double)Gn, d = dfres[f];
    const double dfc = std::min(d + dfprior[f], G - 2.0);   // df.camera
    gdf[2 * (size_t)f] = G;
    gdf[2 * (size_t)f + 1] = dfc;
    for (int32_t j = 0; j < q; ++j) {
      const size_t col = (size_t)f * q + j;
      const double* tj = t + col * R;
      double* o = out + col * 8 * M;
      double sum = 0.0;
      for (size_t r = 0; r < R; ++r)
        if (okf[r] != 0) sum += tj[r];
      const double mean = sum / G;
      double dev = 0.0;
      for (size_t r = 0; r < R; ++r)
        if (okf[r] != 0) {
          const double e = tj[r] - mean;
          dev += e * e;
        }
      const double var = dev / (G - 1.0);
      for (size_t s = 0; s < M; ++s) {
        const double mm = cnt[M * f + s];
        double vif = nan, cor = nan;
        if (ss != nullptr) {
          if (mm > 1.0) {
            vif = ss[M * f + s] / (mm * d);
            cor = (vif - 1.0) / (mm - 1.0);
          } else if (mm == 1.0) {
            vif = 1.0;
          }
        } else if (mm >= 1.0) {
          vif = 1.0 + (mm - 1.0) * inter_gene_cor;
          cor = inter_gene_cor;
        }
        o[s] = mm;
        o[M + s] = cor;
        o[2 * M + s] = vif;
        double T = nan, down = nan, up = nan, pv = nan;
        const double m2 = G - mm;
        if (mm >= 1.0 && m2 >= 1.0 && Gn >= 3) {
          const double used = ss != nullptr && !allow_neg_cor ? std::max(vif, 1.0) : vif;
          const double delta = (G / m2) * (sumt[col * M + s] / mm - mean);
          const double pooled = ((G - 1.0) * var - ((delta * delta) * mm * m2) / G) / (G - 2.0);
          const double scale2 = pooled * (used / mm + 1.0 / m2);
          if (pooled > 0.0 && scale2 > 0.0) {
            T = delta / std::sqrt(scale2);
            const double half = 0.5 * t_two_sided_p(T, dfc);   // pt(-|T|, df.camera)
            down = T < 0.0 ? half : 1.0 - half;
            up = T < 0.0 ? 1.0 - half : half;
            pv = 2.0 * std::min(down, up);
          }
        }
        o[3 * M + s] = T;
        o[4 * M + s] = down;
        o[5 * M + s] = up;
        o[6 * M + s] = pv;
      }
      p_adjust_fdr(o + 6 * M, m, o + 7 * M);
    }
  }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// plaid.fry, step 2 for one gene (include/plaidhip.h): the functions the device runs (camera.h, fry.h)
int plaidhip_fry_residual_row(int32_t n, int32_t p, const double* x, const double* Q, const int8_t* use, const double* E,
                              double c, double* z) try {
  using namespace plaidhip;
  PH_REQUIRE(n >= 0, "fry_residual_row: bad dims n=%d", n);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "fry_residual_row: p = %d coefficients (1 <= p <= %d)", p,
             PLAIDHIP_LIMMA_MAX_COEF);
  if (n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(x && Q && E && z, "fry_residual_row: null argument");
  for (int32_t s = 0; s < n; ++s) {
    double r = x[s];
    for (int32_t k = 0; k < p; ++k) r = camera_chain_step(Q[(size_t)k * n + s], E[k], r);
    z[s] = fry_standardise(r, c, use == nullptr || use[s] != 0);
  }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// plaid.fry (include/plaidhip.h): Q2 of one design, n x (n_f - p) column-major, the rows of unused samples zero
int plaidhip_fry_q2(const double* D, int32_t n, int32_t p, const int8_t* use, int32_t fit, double* Q2, int64_t* nf) try {
  using namespace plaidhip;
  PH_REQUIRE(n >= 0, "fry_q2: bad dims n=%d", n);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "fry_q2: p = %d coefficients (1 <= p <= %d)", p, PLAIDHIP_LIMMA_MAX_COEF);
  PH_REQUIRE(D != nullptr || n == 0, "fry_q2: null design");
  PH_REQUIRE(Q2 != nullptr, "fry_q2: null Q2");
  return limma_design("fry_q2", D, n, p, use, nullptr, 0, fit, nullptr, nullptr, nullptr, nullptr, nf, Q2);
} catch (...) { return plaidhip::on_exception(); }

// plaid.fry, step 1 (include/plaidhip.h): the divisors of every (fit, gene) from the residual sums of squares of ALL samples
int plaidhip_fry_divisors(int32_t rows, int32_t p, int32_t nfit, const double* rss, const int64_t* nf, int standardize,
                          double* cg) try {
  using namespace plaidhip;
  PH_REQUIRE(rows >= 0 && nfit >= 0, "fry_divisors: bad dims rows=%d nfit=%d", rows, nfit);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "fry_divisors: p = %d coefficients (1 <= p <= %d)", p,
             PLAIDHIP_LIMMA_MAX_COEF);
  PH_REQUIRE(standardize >= 0 && standardize <= 2, "fry_divisors: standardize = %d (0 posterior.sd, 1 residual.sd, 2 none)",
             standardize);
  if (rows == 0 || nfit == 0) return PLAIDHIP_OK;
  PH_REQUIRE(rss && nf && cg, "fry_divisors: null argument");
  for (int32_t f = 0; f < nfit; ++f)
    PH_REQUIRE(nf[f] - p >= 1, "fry_divisors: fit %d has %lld samples for %d coefficients", f + 1, (long long)nf[f], p);
  fry_divisors(rows, p, nfit, rss, nf, standardize, cg);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// plaid.fry, step 5 (include/plaidhip.h): the tests of every (fit, contrast, set), fp64
int plaidhip_fry_finish(int32_t m, int32_t nfit, int32_t q, const double* dres, const double* cnt, const double* sume,
                        const double* ss, const double* sume2, const double* lam1, const double* lamD, const double* trM,
                        const double* froM, const int8_t* mixed, double* out) try {
  using namespace plaidhip;
  PH_REQUIRE(m >= 0 && nfit >= 0 && q >= 0, "fry_finish: bad dims m=%d nfit=%d q=%d", m, nfit, q);
  if (m == 0 || nfit == 0 || q == 0) return PLAIDHIP_OK;
  PH_REQUIRE(dres && cnt && sume && ss && out, "fry_finish: null argument");
  const bool any_mixed = mixed != nullptr;
  PH_REQUIRE(!any_mixed || (sume2 && lam1 && lamD && trM && froM), "fry_finish: null argument of the mixed test");
  for (int32_t f = 0; f < nfit; ++f) PH_REQUIRE(dres[f] >= 1.0, "fry_finish: fit %d: df.residual = %g", f + 1, dres[f]);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const size_t M = (size_t)m;
  for (int32_t f = 0; f < nfit; ++f) {
    const double d = dres[f];
    const bool mix = any_mixed && mixed[f] != 0;
    for (int32_t j = 0; j < q; ++j) {
      const size_t col = (size_t)f * q + j;
      double* o = out + col * 7 * M;
      for (size_t s = 0; s < M; ++s) {
        const double mm = cnt[M * f + s];
        double dir = nan, t = nan, pv = nan, pm = nan;
        if (mm >= 1.0) {
          const double mean = sume[col * M + s] / mm;
          t = mean / std::sqrt(ss[M * f + s] / ((mm * mm) * d));
          pv = t_two_sided_p(t, d);
          if (t == t) dir = t < 0.0 ? -1.0 : 1.0;
          if (mix && mm == 1.0) {
            pm = pv;
          } else if (mix) {
            const double D = std::min(mm, d + 1.0), l1 = lam1[col * M + s], lD = lamD[col * M + s];
            const double A = trM[col * M + s], A2 = froM[col * M + s], den = l1 - lD;
            const double Fobs = (sume2[col * M + s] - lD) / den;
            const double bm = 1.0 / D, bv = (D - 1.0) / (D * D) / (D / 2.0 + 1.0);
            const double Fm = (A * bm - lD) / den;
            const double Fv = (bv * A2 - bv / (D - 1.0) * (A * A - A2)) / (den * den);
            const double ab = Fm * (1.0 - Fm) / Fv - 1.0, alpha = ab * Fm, beta = ab - alpha;
            if (std::isfinite(alpha) && std::isfinite(beta) && alpha > 0.0 && beta > 0.0 && Fobs == Fobs)
              pm = beta_upper(Fobs, alpha, beta);
          }
        }
        o[s] = mm;
        o[M + s] = dir;
        o[2 * M + s] = t;
        o[3 * M + s] = pv;
        o[5 * M + s] = pm;
      }
      p_adjust_fdr(o + 3 * M, m, o + 4 * M);
      p_adjust_fdr(o + 5 * M, m, o + 6 * M);
    }
  }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// plaid.roast, step 2 (include/plaidhip.h): the rotations of one design in sample space, W (n + 1) x nrot row-major
int plaidhip_roast_rotations(const double* design, int32_t n, int32_t p, const int8_t* use, int32_t fit, int32_t nrot,
                             uint64_t seed, double* W) try {
  using namespace plaidhip;
  PH_REQUIRE(n >= 0 && fit >= 0, "roast_rotations: bad dims n=%d fit=%d", n, fit);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "roast_rotations: p = %d coefficients (1 <= p <= %d)", p,
             PLAIDHIP_LIMMA_MAX_COEF);
  PH_REQUIRE(nrot >= 1 && nrot <= PLAIDHIP_ROAST_MAX_ROTATIONS, "roast_rotations: nrot = %d (1 <= nrot <= %d)", nrot,
             PLAIDHIP_ROAST_MAX_ROTATIONS);
  PH_REQUIRE(design != nullptr || n == 0, "roast_rotations: null design");
  PH_REQUIRE(W != nullptr, "roast_rotations: null W");
  std::vector<double> Q((size_t)n * p);
  const int rc = limma_design("roast_rotations", design, n, p, use, nullptr, 0, fit + 1, Q.data(), nullptr, nullptr, nullptr, nullptr);
  if (rc != PLAIDHIP_OK) return rc;
  roast_rotations(Q.data(), n, p, use, fit, nrot, seed, W);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// plaid.roast, step 6 (include/plaidhip.h): the tables of every (fit, contrast) from the exact counts
int plaidhip_roast_finish(int32_t m, int32_t nfit, int32_t q, int32_t nrot, int set_statistic, int midp, const int32_t* cnt,
                          const double* msize, const double* ndown, const double* nup, double* out) try {
  using namespace plaidhip;
  PH_REQUIRE(m >= 0 && nfit >= 0 && q >= 0, "roast_finish: bad dims m=%d nfit=%d q=%d", m, nfit, q);
  PH_REQUIRE(set_statistic >= 0 && set_statistic <= 3, "roast_finish: set_statistic = %d (0 mean, 1 floormean, 2 msq, 3 mean50)",
             set_statistic);
  PH_REQUIRE(nrot >= 1, "roast_finish: nrot = %d (at least 1)", nrot);
  if (m == 0 || nfit == 0 || q == 0) return PLAIDHIP_OK;
  PH_REQUIRE(cnt && msize && ndown && nup && out, "roast_finish: null argument");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const size_t M = (size_t)m;
  const double den = (double)nrot + 1.0, half = 0.5 / den;
  std::vector<double> pm(M), fm(M);
  for (int32_t f = 0; f < nfit; ++f)
    for (int32_t j = 0; j < q; ++j) {
      const size_t col = (size_t)f * q + j;
      double* o = out + col * 8 * M;
      const int32_t* b = cnt + col * 4 * M;
      for (size_t s = 0; s < M; ++s) {
        const double mm = msize[M * f + s];
        const bool has = mm >= 1.0 && !(set_statistic == PLAIDHIP_ROAST_STAT_MEAN50 && mm > (double)PLAIDHIP_ROAST_MEAN50_MAX);
        const double pd = ((double)b[4 * s] + 1.0) / den, pu = ((double)b[4 * s + 1] + 1.0) / den;
        o[s] = mm;
        o[M + s] = mm >= 1.0 ? ndown[col * M + s] / mm : nan;
        o[2 * M + s] = mm >= 1.0 ? nup[col * M + s] / mm : nan;
        o[3 * M + s] = !has ? nan : pu < pd ? 1.0 : -1.0;
        o[4 * M + s] = has ? ((double)b[4 * s + 2] + 1.0) / den : nan;
        o[6 * M + s] = has ? ((double)b[4 * s + 3] + 1.0) / den : nan;
      }
      for (int c = 4; c <= 6; c += 2) {   // FDR of PValue, then of PValue.Mixed
        if (!midp) {
          p_adjust_fdr(o + (size_t)c * M, m, o + (size_t)(c + 1) * M);
          continue;
        }
        for (size_t s = 0; s < M; ++s) pm[s] = o[(size_t)c * M + s] - half;
        p_adjust_fdr(pm.data(), m, fm.data());
        for (size_t s = 0; s < M; ++s) {
          const double pv = o[(size_t)c * M + s];
          o[(size_t)(c + 1) * M + s] = pv != pv ? nan : fm[s] > pv ? fm[s] : pv;
        }
      }
    }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// 2 P(T_nu > |t|), with the normal limit for nu infinite or > 10^6 (plaid.romer's shrink)
static double romer_two_sided(double t, double nu) {
  return nu > 1e6 ? 2.0 * plaidhip::pnorm_upper(std::fabs(t)) : plaidhip::t_two_sided_p(t, nu);
}

// the q >= 0 with 2 P(T_nu > q) = p for 0 < p < 1: the normal quantile in the limit, else a bisection on the t tail (the
// bracket is doubled up from 1; it ends when the midpoint is one of the ends)
static double romer_upper_quantile(double p, double nu) {
  if (nu > 1e6) return -plaidhip::qnorm_lower(0.5 * p);
  double lo = 0.0, hi = 1.0;
  while (plaidhip::t_two_sided_p(hi, nu) > p && hi < 1e300) {
    lo = hi;
    hi *= 2.0;
  }
  for (int it = 0; it < 200; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (mid == lo || mid == hi) break;
    if (plaidhip::t_two_sided_p(mid, nu) > p) lo = mid;
    else hi = mid;
  }
  return 0.5 * (lo + hi);
}

// plaid.romer's shrink (include/plaidhip.h: plaidhip_romer, "Shrink"): c_g of the U genes of one (fit, contrast) from their
// moderated t, u = stdev.unscaled, the prior variance s0^2 and nu = df0 + d (may be infinite); *prop takes pi
int plaidhip_romer_shrink(int32_t U, const double* t, double u, double s02, double nu, double* c, double* prop) try {
  using namespace plaidhip;
  PH_REQUIRE(U >= 0, "romer_shrink: U = %d", U);
  PH_REQUIRE(u > 0.0 && std::isfinite(u), "romer_shrink: stdev.unscaled = %g", u);
  PH_REQUIRE(nu > 0.0, "romer_shrink: df.total = %g", nu);
  PH_REQUIRE(prop != nullptr, "romer_shrink: null prop");
  *prop = 0.0;
  if (U == 0) return PLAIDHIP_OK;
  PH_REQUIRE(t && c, "romer_shrink: null argument");
  const size_t n = (size_t)U;
  const double Ud = (double)U, u2 = u * u;
  std::vector<double> tv(t, t + n);
  for (size_t i = 0; i < n; ++i)
    if (std::isnan(tv[i])) tv[i] = 0.0;   // (0 / 0: keyed as 0.0 on the device too)
  t = tv.data();
  // propTrueNull, "lfdr"
  std::vector<double> p(n);
  for (size_t i = 0; i < n; ++i) p[i] = romer_two_sided(t[i], nu);
  std::sort(p.begin(), p.end(), std::greater<double>());
  double acc = 0.0;
  for (size_t j = 0; j < n; ++j) {
    const double i = Ud - (double)j;
    acc += i * std::min(Ud / i * p[j], 1.0);
  }
  const double pi = 1.0 - 2.0 * acc / (Ud * (Ud + 1.0));
  *prop = pi;
  if (!(pi > 0.0)) {
    for (size_t i = 0; i < n; ++i) c[i] = 1.0;
    return PLAIDHIP_OK;
  }
  // tmixture.vector
  const double ntarget = std::ceil(0.5 * pi * Ud);
  const size_t nt = (size_t)std::min(std::max(ntarget, 1.0), Ud);
  const double P = std::max((double)nt / Ud, pi);
  std::vector<double> at(n);
  for (size_t i = 0; i < n; ++i) at[i] = std::fabs(t[i]);
  std::partial_sort(at.begin(), at.begin() + (ptrdiff_t)nt, at.end(), std::greater<double>());
  const double vlo = 0.01 / s02, vhi = 16.0 / s02;
  double vsum = 0.0;
  for (size_t r = 0; r < nt; ++r) {
    const double p0 = romer_two_sided(at[r], nu);
    const double pt = (((double)r + 0.5) / Ud - (1.0 - P) * p0) / P;
    double v = 0.0;
    if (pt > p0) {
      const double qr = romer_upper_quantile(pt, nu), ratio = at[r] / qr;
      v = u2 * (ratio * ratio - 1.0);
    }
    vsum += std::min(std::max(v, vlo), vhi);
  }
  const double v0 = vsum / (double)nt;
  // ProbDE from the log-odds, then the factor
  const double r = (u2 + v0) / u2;
  const double prior = std::log(pi / (1.0 - pi)) - 0.5 * std::log(r);
  for (size_t i = 0; i < n; ++i) {
    double pde = 1.0;
    if (pi < 1.0) {
      const double t2 = t[i] * t[i];
      const double kern = nu > 1e6 ? 0.5 * t2 * (1.0 - 1.0 / r) : 0.5 * (1.0 + nu) * std::log((t2 + nu) / (t2 / r + nu));
      pde = 1.0 / (1.0 + std::exp(-(prior + kern)));
      if (std::isnan(pde)) pde = 1.0;
    }
    c[i] = std::sqrt(u2 / (u2 + v0 * pde));
  }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// plaid.romer's tables (include/plaidhip.h: plaidhip_romer, "Counts and tables") from the exact counts: cnt int32
// [nfit q][m][3] (Up, Down, Mixed), msize m x nfit
int plaidhip_romer_finish(int32_t m, int32_t nfit, int32_t q, int32_t nrot, int set_statistic, const int32_t* cnt,
                          const double* msize, double* out) try {
  using namespace plaidhip;
  PH_REQUIRE(m >= 0 && nfit >= 0 && q >= 0, "romer_finish: bad dims m=%d nfit=%d q=%d", m, nfit, q);
  PH_REQUIRE(set_statistic >= 0 && set_statistic <= 2, "romer_finish: set_statistic = %d (0 mean, 1 floormean, 2 mean50)",
             set_statistic);
  PH_REQUIRE(nrot >= 1, "romer_finish: nrot = %d (at least 1)", nrot);
  if (m == 0 || nfit == 0 || q == 0) return PLAIDHIP_OK;
  PH_REQUIRE(cnt && msize && out, "romer_finish: null argument");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const size_t M = (size_t)m;
  const double den = (double)nrot + 1.0;
  for (int32_t f = 0; f < nfit; ++f)
    for (int32_t j = 0; j < q; ++j) {
      const size_t col = (size_t)f * q + j;
      double* o = out + col * 7 * M;
      const int32_t* b = cnt + col * 3 * M;
      for (size_t s = 0; s < M; ++s) {
        const double mm = msize[M * f + s];
        const bool has = mm >= 1.0 && !(set_statistic == PLAIDHIP_ROMER_STAT_MEAN50 && mm > (double)PLAIDHIP_ROAST_MEAN50_MAX);
        o[s] = mm;
        for (int e = 0; e < 3; ++e) o[(size_t)(1 + e) * M + s] = has ? ((double)b[3 * s + e] + 1.0) / den : nan;
      }
      for (int e = 0; e < 3; ++e) p_adjust_fdr(o + (size_t)(1 + e) * M, m, o + (size_t)(4 + e) * M);
    }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

}  // extern "C"

// Test hook (not part of include/plaidhip.h): plaid.roast's standard normals of (seed, fit, rotation k), indices i0 .. i0 + count - 1
extern "C" void plaidhip_debug_roast_normals(uint64_t seed, int32_t fit, int32_t k, int32_t i0, int32_t count, double* out) {
  for (int32_t i = 0; i < count; ++i) out[i] = plaidhip::roast_normal(seed, fit, k, i0 + i);
}

// Test hook (not part of include/plaidhip.h): pbeta(x, a, b, lower.tail = FALSE) as plaid.fry's mixed test takes it
extern "C" double plaidhip_debug_beta_upper(double x, double a, double b) { return plaidhip::beta_upper(x, a, b); }

// Test hook (not part of include/plaidhip.h): the distribution functions above, so that the CPU-side
// tests can check them against scipy without a device.  kind 0: 2*pt(|x|, a, lower=FALSE);
// 1: pchisq(x, 2*a, lower=FALSE); 2: qnorm(x); 3: pnorm(x, lower=FALSE)
extern "C" double plaidhip_debug_pvalue(int kind, double x, double a) {
  switch (kind) {
    case 0: return plaidhip::t_two_sided_p(x, a);
    case 1: return plaidhip::chisq_upper_even(x, (int)a);
    case 2: return plaidhip::qnorm_lower(x);
    case 3: return plaidhip::pnorm_upper(x);
    default: return std::numeric_limits<double>::quiet_NaN();
  }
}
