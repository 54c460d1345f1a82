// Sanitizer run of plaid.gsea's host argument checks (multi.cpp: check_gsea_call behind plaidhip_gsea_scored and its
// _multi form): the score type, the le_len / le_idx pair, then the checks plaidhip_gsea already had, in the order
// include/plaidhip.h states, and the scans of weight and stat those checks make.  Every call here ends in the checks or at
// the missing context, so no device is touched.  Built and run by `make -C plaid_amd/csrc host-asan-gsea` (api.cpp and
// multi.cpp compiled with -fsanitize=address,undefined on the host side); any sanitizer report aborts with a non-zero status.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/plaidhip.h"

#define REQUIRE(cond)                                                          \
  do {                                                                         \
    if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, plaidhip_last_error_string()); exit(1); } \
  } while (0)

static bool says(const char* what) { return strstr(plaidhip_last_error_string(), what) != nullptr; }

int main() {
  const int32_t g = 65, c = 3, m = 4;
  // exactly sized buffers: a read past any of them is the sanitizer's to find
  std::vector<double> stat((size_t)g * c), weight((size_t)g * c, 1.0), out((size_t)m * 12 * c, -7.0);
  for (size_t e = 0; e < stat.size(); ++e) stat[e] = std::sin((double)e);
  std::vector<int32_t> Gp = {0, 1, 3, 3, 68}, Gi;
  for (int32_t i = 0; i < 3; ++i) Gi.push_back(i);
  for (int32_t i = 0; i < g; ++i) Gi.push_back(i);
  std::vector<int32_t> le_len((size_t)m * c, -7), le_idx((size_t)Gp[m] * c, -7);
  std::vector<double> wneg = weight;
  wneg[(size_t)g * 2 + 3] = -1.0;
  std::vector<double> wnan = weight;
  wnan.back() = std::nan("");

  auto call = [&](int st, int32_t* ln, int32_t* ix, int32_t nperm, int32_t lists, const double* w) {
    return plaidhip_gsea_scored(nullptr, stat.data(), w, g, lists, Gp.data(), Gi.data(), m, nullptr, nperm, 1, st, out.data(),
                                nullptr, ln, ix);
  };
  // 1. the score type first, whatever else is wrong
  for (int st : {-1, 3, 1 << 30}) REQUIRE(call(st, le_len.data(), nullptr, 0, 0, wneg.data()) == PLAIDHIP_EINVAL && says("score_type"));
  // 2. one edge buffer without the other
  REQUIRE(call(1, le_len.data(), nullptr, 0, 0, wneg.data()) == PLAIDHIP_EINVAL && says("le_len and le_idx"));
  REQUIRE(call(2, nullptr, le_idx.data(), 0, 0, wneg.data()) == PLAIDHIP_EINVAL && says("le_len and le_idx"));
  // 3. the existing order: nperm, the lists, the genes' bound, a weight
  for (int st = 0; st <= 2; ++st) {
    REQUIRE(call(st, le_len.data(), le_idx.data(), 0, 0, wneg.data()) == PLAIDHIP_EINVAL && says("nperm"));
    REQUIRE(call(st, le_len.data(), le_idx.data(), 10, 0, wneg.data()) == PLAIDHIP_EINVAL && says("ranked lists"));
    REQUIRE(call(st, le_len.data(), le_idx.data(), 10, c, wneg.data()) == PLAIDHIP_EINVAL && says("weight"));
    REQUIRE(call(st, nullptr, nullptr, 10, c, wnan.data()) == PLAIDHIP_EINVAL && says("weight"));
    // all arguments good, with and without the edge buffers: the whole of weight and stat is scanned, then the context is missed
    REQUIRE(call(st, le_len.data(), le_idx.data(), 10, c, weight.data()) == PLAIDHIP_EINVAL && says("null plaidhip_ctx"));
    REQUIRE(call(st, nullptr, nullptr, 10, c, weight.data()) == PLAIDHIP_EINVAL && says("null plaidhip_ctx"));
  }
  {
    std::vector<double> big((size_t)PLAIDHIP_GSEA_KS_MAX_GENES + 1, 1.0);
    REQUIRE(plaidhip_gsea_scored(nullptr, big.data(), big.data(), PLAIDHIP_GSEA_KS_MAX_GENES + 1, 1, Gp.data(), Gi.data(), m, nullptr,
                                 10, 1, 1, out.data(), nullptr, le_len.data(), le_idx.data()) == PLAIDHIP_EUNSUPPORTED);
  }
  // the several-device form: its own checks of the device list come first, then the same order
  const int twice[2] = {0, 0};
  REQUIRE(plaidhip_gsea_scored_multi(twice, 2, stat.data(), weight.data(), g, c, Gp.data(), Gi.data(), m, nullptr, 10, 1, 3,
                                     out.data(), nullptr, nullptr, nullptr) == PLAIDHIP_EINVAL && says("listed twice"));
  const int dev0[1] = {0};
  REQUIRE(plaidhip_gsea_scored_multi(dev0, 1, stat.data(), wneg.data(), g, c, Gp.data(), Gi.data(), m, nullptr, 0, 1, 3,
                                     out.data(), nullptr, le_len.data(), nullptr) == PLAIDHIP_EINVAL && says("score_type"));
  REQUIRE(plaidhip_gsea_scored_multi(dev0, 1, stat.data(), wneg.data(), g, c, Gp.data(), Gi.data(), m, nullptr, 0, 1, 2,
                                     out.data(), nullptr, le_len.data(), nullptr) == PLAIDHIP_EINVAL && says("le_len and le_idx"));
  REQUIRE(plaidhip_gsea_scored_multi(dev0, 1, stat.data(), wneg.data(), g, c, Gp.data(), Gi.data(), m, nullptr, 10, 1, 2,
                                     out.data(), nullptr, le_len.data(), le_idx.data()) == PLAIDHIP_EINVAL && says("weight"));
  // the entries that were there before keep their order
  REQUIRE(plaidhip_gsea(nullptr, stat.data(), wneg.data(), g, c, Gp.data(), Gi.data(), m, nullptr, 0, 1, out.data(), nullptr) ==
              PLAIDHIP_EINVAL && says("nperm"));
  // nothing was written by any of it
  for (double v : out) REQUIRE(v == -7.0);
  for (int32_t v : le_len) REQUIRE(v == -7);
  for (int32_t v : le_idx) REQUIRE(v == -7);
  printf("[host-asan-gsea] ok\n");
  return 0;
}
