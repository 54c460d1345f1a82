// The pair plan's flex steps under AddressSanitizer + UBSan (`make -C plaid_amd/csrc host-asan-flex`): geneset.cpp compiled
// for the host with the sanitizers, this program and the HIP stand-ins.  For every collection -- files in plan_probe's
// format (int32 g, int32 m, int32 Gp[m + 1], int32 Gi[Gp[m]]) given on the command line, or two built-in ones -- it builds the
// plan with and without flex steps and holds the self-check (plaidhip_debug_pair_flex_probe): every membership scheduled
// exactly once, own or guest; no host lane with an own gene on a flex step, no guest gene on a normal step; owner <-> host
// one to one inside a tile; overflow <= T/8, host length <= 7T/8.  Prints one line per collection, then "[host-asan-flex] ok".
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" int plaidhip_debug_pair_flex_probe(int32_t g, int32_t m, const int32_t* Gp, const int32_t* Gi, int32_t waves,
                                              int32_t flex, int64_t out[16], int32_t* pairs, int64_t cap);

static int check(const char* name, int32_t g, const std::vector<int32_t>& Gp, const std::vector<int32_t>& Gi) {
  const int32_t m = (int32_t)Gp.size() - 1;
  int64_t with[16], without[16];
  std::vector<int32_t> pairs((size_t)4 * 64 * 96 * 3);
  if (plaidhip_debug_pair_flex_probe(g, m, Gp.data(), Gi.data(), 16, 1, with, pairs.data(), (int64_t)pairs.size() / 4) != 0) return 1;
  if (plaidhip_debug_pair_flex_probe(g, m, Gp.data(), Gi.data(), 16, 0, without, nullptr, 0) != 0) return 1;
  printf("%s: g %d m %d z %d slices %" PRId64 " regp %" PRId64 " slots %" PRId64 " (without flex steps %" PRId64
         ") double-booked %" PRId64 " (%" PRId64 ") pairs %" PRId64 " broken %" PRId64 " wrong %" PRId64 "\n",
         name, g, m, Gp[m], with[0], with[5], with[8], without[8], with[3], without[3], with[9], with[10], with[4]);
  int bad = 0;
  if (with[2] != Gp[m] || with[4] != 0 || with[10] != 0) bad = 1;          // once each, right lane and step, relations hold
  if (without[2] != Gp[m] || without[4] != 0 || without[9] != 0) bad = 1;
  if (with[8] > without[8]) bad = 1;                                       // flex steps never add slots
  if (with[5] == 0 && (with[9] != 0 || with[8] != without[8])) bad = 1;    // only register-partial plans get them
  for (int64_t k = 0; k < with[9] && k < (int64_t)pairs.size() / 4; ++k)
    if (pairs[4 * k + 1] < 0 || pairs[4 * k + 1] >= m || pairs[4 * k + 2] >= m || pairs[4 * k + 3] < 0 || pairs[4 * k + 3] >= g) bad = 1;
  if (bad) fprintf(stderr, "%s: the plan's self-check failed\n", name);
  return bad;
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { perror(argv[a]); return 2; }
    int32_t g = 0, m = 0;
    if (fread(&g, 4, 1, f) != 1 || fread(&m, 4, 1, f) != 1) return 2;
    std::vector<int32_t> Gp((size_t)m + 1);
    if (fread(Gp.data(), 4, Gp.size(), f) != Gp.size()) return 2;
    std::vector<int32_t> Gi((size_t)Gp[m]);
    if (!Gi.empty() && fread(Gi.data(), 4, Gi.size(), f) != Gi.size()) return 2;
    fclose(f);
    bad |= check(argv[a], g, Gp, Gi);
  }
  if (argc < 2) {
    // built in: 130 sets of 60 genes, 42 / 18 and 18 / 42 in the two slices of 10,400 genes in turn (half the lanes of a tile
    // long, half hosts; the third tile has two sets and 62 lanes without one), and 300 sets of 5 ... 204 genes over three slices
    uint64_t st = 88172645463325252ull;
    auto rnd = [&st]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    {
      const int32_t g = 10400;
      std::vector<int32_t> Gp{0}, Gi;
      for (int j = 0; j < 130; ++j) {
        const int first = j % 2 == 0 ? 42 : 18;
        for (int k = 0; k < 60; ++k) Gi.push_back((k < first ? 0 : 5200) + j * 39 + (k < first ? k : k - first));   // ascending
        Gp.push_back((int32_t)Gi.size());
      }
      bad |= check("two-slices-42-18", g, Gp, Gi);
    }
    {
      const int32_t g = 20600;
      std::vector<int32_t> Gp{0}, Gi;
      for (int j = 0; j < 300; ++j) {
        const int k = 5 + (int)(rnd() % 200);
        int32_t gene = (int32_t)(rnd() % 50);
        for (int i = 0; i < k && gene < g; ++i) { Gi.push_back(gene); gene += 1 + (int32_t)(rnd() % (2 * g / k)); }
        Gp.push_back((int32_t)Gi.size());
      }
      bad |= check("three-slices-random", g, Gp, Gi);
    }
  }
  if (bad) return 1;
  printf("[host-asan-flex] ok\n");
  return 0;
}
