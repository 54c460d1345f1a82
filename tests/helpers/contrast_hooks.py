"""plaid.test.contrasts for the tests: the library's one-device sharding hook
(multi.cpp: plaidhip_debug_plaid_test_contrasts_sharded_on_one_device), and the inputs that the GPU test of the exclusions
and the host test of its references share.

The hook's C signature is plaidhip_plaid_test_contrasts_multi's with (device, nshards, fail_shard) for (devices, ndev), as
for every hook of tests/helpers/sharded_hooks.py; it goes through the package's own marshaller."""
import numpy as np

from plaid_amd import engine
from tests.helpers import exact_stats as xs
from tests.helpers.sharded_hooks import _status, hook

NA = -1


def run(nshards, X, Y, Gp, Gi, gsetX=None, tests=7, metap=0, fail=-1, out=None):
    """(status, sets x 6 x C) of plaid.test.contrasts on `nshards` contexts of one device; the result holds -7 before the
    call unless it is the caller's `out`"""
    Y = np.asarray(Y)
    ncon = 1 if Y.ndim == 1 else Y.shape[1]
    out = np.full((len(Gp) - 1, 6, ncon), -7.0, order="F") if out is None else out
    status, _ = _status(lambda: engine._plaid_test_contrasts(hook("plaid_test_contrasts"), (0, nshards, fail), X, Y, Gp, Gi,
                                                             gsetX, tests, metap, out=out))
    return status, out


def random_contrasts(n, C, rng, na=0.0):
    """n x C labels: 0 / 1 at random (about 40 % ones), a fraction `na` of each column NA"""
    Y = (rng.random((n, C)) < 0.4).astype(np.int32)
    if na > 0:
        Y[rng.random((n, C)) < na] = NA
    return Y


# ---- the exclusion cases: (g, n, m, seed); n > 128 so that one contrast can keep its group 1 inside the first column block
EXCLUSION_CASES = [(300, 263, 24, 5), (257, 129, 12, 6)]


def exclusion_case(g, n, m, seed):
    """X (g x n), Y (n x 3, about 30 % NA per contrast), the sets, and scores S (m x n) for gsetX, all with a real group
    effect per gene / per set and contrast, so that no Welch or t statistic sits on a variance of zero.
      contrast 0: labels at random;   contrast 1: its group 1 lies wholly in the first 128 columns;
      contrast 2: group 1 is ONE sample (p.lm = 1 - 1e-99 for every set)"""
    rng = np.random.default_rng(seed)
    Y = random_contrasts(n, 3, rng, na=0.3)
    Y[:4, 0] = [0, 1, 0, 1]
    Y[Y[:, 1] == 1, 1] = 0
    Y[rng.choice(128, 30, replace=False), 1] = 1
    Y[-4:, 1] = [0, 0, NA, 0]
    Y[Y[:, 2] == 1, 2] = 0
    Y[n // 2, 2] = 1
    X = rng.gamma(2.0, 1.0, size=(g, n))
    S = rng.gamma(2.0, 1.0, size=(m, n)) + 0.25
    for j in range(3):
        X[:, Y[:, j] == 1] += rng.normal(0.0, 0.3, size=(g, 1))
        S[:, Y[:, j] == 1] += 0.3 * rng.normal(size=(m, 1))
    sizes = rng.integers(2, min(200, g - 2) + 1, size=m)
    sizes[0], sizes[-1] = 2, g - 2
    sets = [np.sort(rng.choice(g, size=int(k), replace=False)) for k in sizes]
    Gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return X, Y, Gp, np.concatenate(sets).astype(np.int32), S


def subset(Y, j):
    """(sel, y): the samples of contrast j and their 0 / 1 labels"""
    sel = np.flatnonzero(Y[:, j] != NA)
    return sel, Y[sel, j].astype(np.int32)


def welch_intervals(S_sel, y):
    """per set: (gsetFC of tests = 4 and its bound, the interval of p.lm) from the exact moments of S_sel; the interval is
    None where not separable, and the string "degenerate" where a group has fewer than two samples or the moments are not
    finite (p.lm is then 1 - 1e-99 exactly)"""
    ref = xs.group_moments(S_sel, y)
    n0, n1 = (int(v) for v in ref["n"])
    nk = ref["n"][:, None].astype(np.float64)
    mb = xs.mean_bound(ref["mag"], nk)
    qb = xs.ssd_bound(ref["ssd"], nk, mb)
    with np.errstate(all="ignore"):
        fc = ref["mean"][1] - ref["mean"][0]
        fb = mb[0] + mb[1] + 2 * xs.U * np.abs(fc)
    ivs = []
    for j in range(S_sel.shape[0]):
        if n0 < 2 or n1 < 2 or not (np.isfinite(ref["ssd"][:, j]).all() and np.isfinite(fc[j])):
            ivs.append("degenerate")
            continue
        ivs.append(xs.welch_interval(ref["mean"][0, j], mb[0, j], ref["mean"][1, j], mb[1, j], ref["ssd"][0, j], qb[0, j],
                                     ref["ssd"][1, j], qb[1, j], n0, n1))
    return fc, fb, ivs
