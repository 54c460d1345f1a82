// `make -C plaid_amd/csrc host-asan-limma-w`: plaidhip_limma_w_solve (stats.cpp, csrc/lmfit_na.h: lmfit_w_row_solve) and
// plaidhip_lowess (csrc/lowess.h) under AddressSanitizer and UBSan as a program of its own, on exactly sized heap buffers.  Without arguments: built-in decks at every
// p -- H summed from a random orthonormal-ish basis and weights, so that H gamma = b can be checked --, the estimability
// rule (a deficient triangle, |live| = p, a NaN pivot) and power-of-two scalings.  With a file (tests/test_limma_w_host_asan.py
// writes the decks of tests/test_limma_w_ref.py): int32 count, then per deck int32 p, q, ok, int64 nlive and the doubles
// Htri[p (p + 1) / 2], b[p], v[p q], gamma[p], u[q]; then int32 count of lowess decks, per deck int64 n, int32 iter, doubles f,
// delta, x[n], y[n], ys[n] and n bytes of anchor flags -- the expected values are the Python restatements' and are met bit
// for bit.  Built in for lowess: ties, clumps, constant y, n = 1 and 2, delta = 0 and the default, with and without the flags.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/plaidhip.h"

#define REQUIRE(cond)                                                              \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      fprintf(stderr, "[host-asan-limma-w] FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }

static void built_in() {
  std::mt19937_64 rng(28);
  std::normal_distribution<double> N(0.0, 1.0);
  std::uniform_real_distribution<double> Uw(std::log(0.25), std::log(4.0));
  for (int p = 1; p <= PLAIDHIP_LIMMA_NA_MAX_COEF; ++p) {
    const int n = 40, q = 2, T = p * (p + 1) / 2;
    std::vector<double> Q((size_t)n * p), om((size_t)n), x((size_t)n), v((size_t)p * q);
    for (auto& t : Q) t = N(rng) / std::sqrt((double)n);
    for (auto& t : om) t = std::exp(Uw(rng));
    for (auto& t : x) t = N(rng);
    for (auto& t : v) t = N(rng);
    for (int dead : {0, 5, n - p - 1, n - p}) {   // (n - p dead observations: no residual degree of freedom)
      std::vector<double> Htri((size_t)T), b((size_t)p), gamma((size_t)p), u((size_t)q), piv((size_t)p);
      for (int k = 0, j = 0; k < p; ++k) {
        for (int l = 0; l <= k; ++l, ++j) {
          double s = 0.0;
          for (int c = dead; c < n; ++c) s += om[(size_t)c] * Q[(size_t)c * p + k] * Q[(size_t)c * p + l];
          Htri[(size_t)j] = s;
        }
        double s = 0.0;
        for (int c = dead; c < n; ++c) s += om[(size_t)c] * x[(size_t)c] * Q[(size_t)c * p + k];
        b[(size_t)k] = s;
      }
      int32_t ok = -1;
      REQUIRE(plaidhip_limma_w_solve(p, Htri.data(), b.data(), n - dead, v.data(), q, gamma.data(), u.data(), piv.data(), &ok) ==
              PLAIDHIP_OK);
      REQUIRE(ok == (n - dead - p >= 1 ? 1 : 0));
      if (!ok) {
        for (int k = 0; k < p; ++k) REQUIRE(std::isnan(gamma[(size_t)k]));
        continue;
      }
      for (int k = 0; k < p; ++k) {   // H gamma = b
        double s = 0.0, mag = 0.0;
        for (int l = 0; l < p; ++l) {
          const double h = k >= l ? Htri[(size_t)(k * (k + 1) / 2 + l)] : Htri[(size_t)(l * (l + 1) / 2 + k)];
          s += h * gamma[(size_t)l];
          mag += std::fabs(h * gamma[(size_t)l]);
        }
        REQUIRE(std::fabs(s - b[(size_t)k]) <= 1e-9 * (mag + std::fabs(b[(size_t)k])));
      }
      for (int j = 0; j < q; ++j) REQUIRE(u[(size_t)j] > 0.0);
      // every weight times 2^e: the same gamma to the bit, pivots scaled; NULL pivots are accepted
      for (int e : {2, -40, 300}) {
        std::vector<double> Hs(Htri), bs(b), g2((size_t)p), u2((size_t)q);
        for (auto& t : Hs) t = std::ldexp(t, e);
        for (auto& t : bs) t = std::ldexp(t, e);
        REQUIRE(plaidhip_limma_w_solve(p, Hs.data(), bs.data(), n - dead, v.data(), q, g2.data(), u2.data(), nullptr, &ok) == PLAIDHIP_OK);
        REQUIRE(ok == 1);
        for (int k = 0; k < p; ++k) REQUIRE(same_bits(g2[(size_t)k], gamma[(size_t)k]));
      }
    }
    if (p >= 2) {   // a deficient triangle (two equal directions) and a NaN entry: not ok, NaN out, the pivots up to the break
      std::vector<double> Htri((size_t)T, 0.0), b((size_t)p, 1.0), gamma((size_t)p), u((size_t)q), piv((size_t)p);
      for (int k = 0; k < p; ++k) Htri[(size_t)(k * (k + 1) / 2 + k)] = 4.0;
      Htri[1] = 4.0;   // H_10 = H_00 = H_11: L_00 = L_10 = 2 and the second pivot is exactly 0
      int32_t ok = -1;
      REQUIRE(plaidhip_limma_w_solve(p, Htri.data(), b.data(), 30, v.data(), q, gamma.data(), u.data(), piv.data(), &ok) == PLAIDHIP_OK);
      REQUIRE(ok == 0 && piv[0] == 4.0 && piv[1] == 0.0 && std::isnan(gamma[0]) && std::isnan(u[0]));
      for (int k = 2; k < p; ++k) REQUIRE(std::isnan(piv[(size_t)k]));
      Htri[0] = NAN;
      REQUIRE(plaidhip_limma_w_solve(p, Htri.data(), b.data(), 30, v.data(), q, gamma.data(), u.data(), piv.data(), &ok) == PLAIDHIP_OK);
      REQUIRE(ok == 0);
    }
    REQUIRE(plaidhip_limma_w_solve(p, nullptr, nullptr, 3, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == PLAIDHIP_EINVAL);
  }
  REQUIRE(plaidhip_limma_w_solve(PLAIDHIP_LIMMA_NA_MAX_COEF + 1, nullptr, nullptr, 3, nullptr, 0, nullptr, nullptr, nullptr, nullptr) ==
          PLAIDHIP_EINVAL);
  printf("  built-in: 1 .. %d coefficients, 0 to n - p dead observations, scalings, deficient and NaN triangles\n",
         PLAIDHIP_LIMMA_NA_MAX_COEF);
}

static void lowess_built_in() {
  std::mt19937_64 rng(5);
  std::normal_distribution<double> N(0.0, 1.0);
  for (int n : {1, 2, 3, 17, 400}) {
    for (int kind = 0; kind < 3; ++kind) {   // plain, heavy ties, constant y
      std::vector<double> x((size_t)n), y((size_t)n), ys((size_t)n);
      std::vector<int8_t> anchor((size_t)n);
      for (auto& t : x) t = kind == 1 ? std::floor(2.0 * N(rng)) : N(rng);
      std::sort(x.begin(), x.end());
      for (int i = 0; i < n; ++i) y[(size_t)i] = kind == 2 ? 0.5 : 1.0 + 0.3 * x[(size_t)i] + 0.1 * N(rng);
      for (double f : {0.05, 0.5, 1.0, 7.0})
        for (double delta : {0.0, 0.01 * (x[(size_t)n - 1] - x[0]), 1e9}) {
          REQUIRE(plaidhip_lowess(x.data(), y.data(), n, f, 3, delta, ys.data(), anchor.data()) == PLAIDHIP_OK);
          REQUIRE(anchor[0] == 1 && anchor[(size_t)n - 1] == 1);
          for (int i = 0; i < n; ++i) REQUIRE(std::isfinite(ys[(size_t)i]));
          if (kind == 2) for (int i = 0; i < n; ++i) REQUIRE(std::fabs(ys[(size_t)i] - 0.5) < 1e-12);
          REQUIRE(plaidhip_lowess(x.data(), y.data(), n, f, 0, delta, ys.data(), nullptr) == PLAIDHIP_OK);
        }
    }
  }
  double two[2] = {2.0, 1.0}, out[2];
  REQUIRE(plaidhip_lowess(two, two, 2, 0.5, 3, 0.0, out, nullptr) == PLAIDHIP_EINVAL);   // not ascending
  REQUIRE(plaidhip_lowess(two, two, 0, 0.5, 3, 0.0, out, nullptr) == PLAIDHIP_EINVAL);
  printf("  lowess built-in: n = 1 .. 400, ties, constant y, spans 0.05 .. 7, delta 0 .. 1e9\n");
}

static void lowess_from_file(FILE* f, const char* path) {
  int32_t count = 0;
  REQUIRE(fread(&count, 4, 1, f) == 1 && count >= 0);
  for (int32_t i = 0; i < count; ++i) {
    int64_t n = 0;
    int32_t iter = 0;
    double fd[2];
    REQUIRE(fread(&n, 8, 1, f) == 1 && fread(&iter, 4, 1, f) == 1 && fread(fd, 8, 2, f) == 2 && n >= 1 && n < (1 << 24));
    std::vector<double> x((size_t)n), y((size_t)n), want((size_t)n), ys((size_t)n);
    std::vector<int8_t> wanta((size_t)n), anchor((size_t)n);
    REQUIRE(fread(x.data(), 8, (size_t)n, f) == (size_t)n && fread(y.data(), 8, (size_t)n, f) == (size_t)n);
    REQUIRE(fread(want.data(), 8, (size_t)n, f) == (size_t)n && fread(wanta.data(), 1, (size_t)n, f) == (size_t)n);
    REQUIRE(plaidhip_lowess(x.data(), y.data(), n, fd[0], iter, fd[1], ys.data(), anchor.data()) == PLAIDHIP_OK);
    for (int64_t j = 0; j < n; ++j) REQUIRE(same_bits(ys[(size_t)j], want[(size_t)j]) && anchor[(size_t)j] == wanta[(size_t)j]);
  }
  printf("  %s: %d lowess decks met bit for bit\n", path, count);
}

static void from_file(const char* path) {
  FILE* f = fopen(path, "rb");
  REQUIRE(f != nullptr);
  int32_t count = 0;
  REQUIRE(fread(&count, 4, 1, f) == 1 && count >= 0);
  for (int32_t i = 0; i < count; ++i) {
    int32_t head[3];
    int64_t nlive = 0;
    REQUIRE(fread(head, 4, 3, f) == 3 && fread(&nlive, 8, 1, f) == 1);
    const int32_t p = head[0], q = head[1], want = head[2];
    REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_NA_MAX_COEF && q >= 0 && q <= 64);
    const size_t T = (size_t)p * (p + 1) / 2;
    std::vector<double> Htri(T), b((size_t)p), v((size_t)p * q), eg((size_t)p), eu((size_t)q), gamma((size_t)p), u((size_t)q),
        piv((size_t)p);
    REQUIRE(fread(Htri.data(), 8, T, f) == T && fread(b.data(), 8, (size_t)p, f) == (size_t)p);
    REQUIRE(fread(v.data(), 8, v.size(), f) == v.size());
    REQUIRE(fread(eg.data(), 8, eg.size(), f) == eg.size() && fread(eu.data(), 8, eu.size(), f) == eu.size());
    int32_t ok = -1;
    REQUIRE(plaidhip_limma_w_solve(p, Htri.data(), b.data(), nlive, v.data(), q, gamma.data(), u.data(), piv.data(), &ok) == PLAIDHIP_OK);
    REQUIRE(ok == want);
    for (int k = 0; k < p; ++k) REQUIRE(same_bits(gamma[(size_t)k], eg[(size_t)k]));
    for (int j = 0; j < q; ++j) REQUIRE(same_bits(u[(size_t)j], eu[(size_t)j]));
  }
  printf("  %s: %d decks met bit for bit\n", path, count);
  lowess_from_file(f, path);
  fclose(f);
}

int main(int argc, char** argv) {
  built_in();
  lowess_built_in();
  for (int a = 1; a < argc; ++a) from_file(argv[a]);
  printf("[host-asan-limma-w] ok\n");
  return 0;
}
