// plaid.romer: the keys of one (gene, rotation) and the shapes of the set statistic as pinned in include/plaidhip.h
// (plaidhip_romer), once, for the device (kernels_romer.hip) and for the host entries.  The rotated moderated t itself is
// roast.h's (roast_chain_step, roast_moderated_t): one copy of that arithmetic for both tests.
#pragma once

#include <vector>

#include "roast.h"

#define PLAIDHIP_ROMER_STAT_MEAN 0
#define PLAIDHIP_ROMER_STAT_FLOORMEAN 1
#define PLAIDHIP_ROMER_STAT_MEAN50 2

namespace plaidhip {

// the three keys of a rotated t; *nan is raised where t is a NaN (0 / 0), which is keyed as 0.0.  x = t + 0.0, so that no
// -0.0 reaches a ranker; key b exists under floormean only (0.0 otherwise)
PH_CAM_HD inline void romer_keys(double t, int set_statistic, double* a, double* b, double* c, bool* nan) {
#pragma clang fp contract(off)
  *nan = t != t;
  const double x = (*nan ? 0.0 : t) + 0.0;
  const double ax = fabs(x);
  if (set_statistic == PLAIDHIP_ROMER_STAT_FLOORMEAN) {
    const double nx = -x;
    *a = x > 0.0 ? x : 0.0;
    *b = (nx > 0.0 ? nx : 0.0) + 0.0;
    *c = ax > 1.0 ? ax : 1.0;
  } else {
    *a = x;
    *b = 0.0;
    *c = ax;
  }
}

// how many key matrices a statistic ranks (a, c; floormean: a, b, c)
inline int romer_nkeys(int set_statistic) { return set_statistic == PLAIDHIP_ROMER_STAT_FLOORMEAN ? 3 : 2; }

// mean50 on the device: a wave holds the 2 r of one (set, rotation) in LDS.  Class 0: at most 1,024 members (four waves a
// workgroup, 16 KiB); class 1: up to PLAIDHIP_ROAST_MEAN50_MAX (one wave a workgroup, 64 KiB); the sets above it get no
// statistic.  Sets without a member are in class 0.
inline int romer_mean50_class(int32_t members) { return members <= 1024 ? 0 : members <= 16384 ? 1 : 2; }
inline int32_t romer_mean50_class_cap(int cls) { return cls == 0 ? 1024 : 16384; }

// the set numbers of mean50's two size classes, class after class; the sets above the cap are left out
inline void romer_mean50_classes(const int32_t* gp, int32_t m, std::vector<int32_t>& sel, int32_t class_cnt[2]) {
  sel.clear();
  class_cnt[0] = class_cnt[1] = 0;
  for (int cls = 0; cls < 2; ++cls)
    for (int32_t st = 0; st < m; ++st)
      if (romer_mean50_class(gp[(size_t)st + 1] - gp[(size_t)st]) == cls) {
        sel.push_back(st);
        ++class_cnt[cls];
      }
}

}  // namespace plaidhip
