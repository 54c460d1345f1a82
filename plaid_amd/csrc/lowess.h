// lowess as pinned in include/plaidhip.h (plaidhip_lowess): Cleveland's locally weighted regression with the anchor walk of
// `delta`, AS RECALLED from R's lowess().  Host only, fp64, every sum in ascending index order from 0.0, no fused operation.
// plaid.voom's mean-variance trend runs it (shard_voom.cpp); its knots are the anchors of the last pass.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace plaidhip {

// the local fit at xs over the window [nleft, nright] (the header's words).  w: n doubles of scratch.  false: sum of weights <= 0
inline bool lowess_local_fit(const double* x, const double* y, int64_t n, double xs, int64_t nleft, int64_t nright, double* w,
                             bool robust, const double* rw, double* ys) {
  const double range = x[n - 1] - x[0];
  const double h = std::max(xs - x[nleft], x[nright] - xs);
  const double h9 = 0.999 * h, h1 = 0.001 * h;
  double a = 0.0;
  int64_t j = nleft;
  for (; j < n; ++j) {
    w[j] = 0.0;
    const double r = fabs(x[j] - xs);
    if (r <= h9) {
      if (r <= h1) {
        w[j] = 1.0;
      } else {
        const double t = r / h, t3 = (t * t) * t, u = 1.0 - t3;
        w[j] = (u * u) * u;
      }
      if (robust) w[j] = w[j] * rw[j];
      a = a + w[j];
    } else if (x[j] > xs) {
      break;
    }
  }
  const int64_t nrt = j;   // one past the last point that got a weight
  if (!(a > 0.0)) return false;
  for (j = nleft; j < nrt; ++j) w[j] = w[j] / a;
  if (h > 0.0) {
    a = 0.0;
    for (j = nleft; j < nrt; ++j) a = a + w[j] * x[j];
    double c = 0.0;
    for (j = nleft; j < nrt; ++j) c = c + w[j] * ((x[j] - a) * (x[j] - a));
    if (sqrt(c) > 0.001 * range) {
      const double b = (xs - a) / c;
      for (j = nleft; j < nrt; ++j) w[j] = w[j] * (b * (x[j] - a) + 1.0);
    }
  }
  double s = 0.0;
  for (j = nleft; j < nrt; ++j) s = s + w[j] * y[j];
  *ys = s;
  return true;
}

// x ascending, n >= 1.  ys: the n fitted values.  anchor (may be null): n flags, 1 where the LAST pass made the local fit or a
// tie copy.  iter robustness passes after the first fit (iter + 1 fitting passes).
inline void lowess_run(const double* x, const double* y, int64_t n, double f, int iter, double delta, double* ys, int8_t* anchor) {
  if (n < 2) {
    ys[0] = y[0];
    if (anchor != nullptr) anchor[0] = 1;
    return;
  }
  const int64_t ns = std::max<int64_t>(2, std::min<int64_t>(n, (int64_t)floor(f * (double)n + 1e-7)));
  std::vector<double> rw((size_t)n, 1.0), res((size_t)n), w((size_t)n), srt((size_t)n);
  for (int it = 1; it <= iter + 1; ++it) {
    if (anchor != nullptr) std::fill(anchor, anchor + n, (int8_t)0);
    int64_t nleft = 0, nright = ns - 1, last = -1, i = 0;
    for (;;) {
      if (nright < n - 1) {
        const double d1 = x[i] - x[nleft], d2 = x[nright + 1] - x[i];
        if (d1 > d2) {
          ++nleft;
          ++nright;
          continue;
        }
      }
      if (!lowess_local_fit(x, y, n, x[i], nleft, nright, w.data(), it > 1, rw.data(), &ys[i])) ys[i] = y[i];
      if (anchor != nullptr) anchor[i] = 1;
      if (last < i - 1) {
        const double denom = x[i] - x[last];
        for (int64_t j = last + 1; j < i; ++j) {
          const double alpha = (x[j] - x[last]) / denom;
          ys[j] = alpha * ys[i] + (1.0 - alpha) * ys[last];
        }
      }
      last = i;
      const double cut = x[last] + delta;
      for (i = last + 1; i < n; ++i) {
        if (x[i] > cut) break;
        if (x[i] == x[last]) {
          ys[i] = ys[last];
          if (anchor != nullptr) anchor[i] = 1;
          last = i;
        }
      }
      i = std::max(last + 1, i - 1);
      if (last >= n - 1) break;
    }
    for (int64_t j = 0; j < n; ++j) res[(size_t)j] = y[j] - ys[j];
    if (it > iter) break;
    double sc = 0.0;
    for (int64_t j = 0; j < n; ++j) {
      srt[(size_t)j] = fabs(res[(size_t)j]);
      sc = sc + srt[(size_t)j];
    }
    sc = sc / (double)n;
    std::sort(srt.begin(), srt.end());
    const double med = (n % 2) ? srt[(size_t)(n / 2)] : (srt[(size_t)(n / 2 - 1)] + srt[(size_t)(n / 2)]) / 2.0;
    const double cmad = 6.0 * med;
    if (cmad < 1e-7 * sc) break;
    const double c9 = 0.999 * cmad, c1 = 0.001 * cmad;
    for (int64_t j = 0; j < n; ++j) {
      const double r = fabs(res[(size_t)j]);
      if (r <= c1) {
        rw[(size_t)j] = 1.0;
      } else if (r <= c9) {
        const double t = r / cmad, u = 1.0 - t * t;
        rw[(size_t)j] = u * u;
      } else {
        rw[(size_t)j] = 0.0;
      }
    }
  }
}

}  // namespace plaidhip
