"""plaid.roast's references and its host-only step 6, without a GPU (tests/helpers/roast_ref.py).

  1. The identity the design rests on, at 50 digits: limma's own form -- the effects [beta | Q2'r] of the full QR rotated by
     (r0, R2), and their row sum of squares -- equals the sample-space form beta r0 + r.w with w = Q2 R2, and beta^2 + RSS, to
     10^-40 on every case.
  2. The numpy restatement's deviation from the 50-digit one per quantity is what roast_ref.MEASURED records (re-measured).
  3. In the 50-digit reference of the end-to-end cases no (set, side, rotation) lies within twice the device's allowance of
     the observed statistic (exact structural ties apart), so the counts b are decided and the device must match them.
  4. plaidhip_roast_finish is step 6 exactly: counts -> p, midp and its pmax, BH, Direction ties, m = 0, the mean50 cap.
  5. The mean50 threshold form equals the mean of the h largest (a sort) at 50 digits, ties and one-signed z among them."""
import numpy as np
import pytest

from plaid_amd import engine
from tests.helpers import roast_ref as rr


@pytest.mark.parametrize("nf,p,seed", [(5, 2, 1), (9, 3, 2), (14, 5, 3), (40, 2, 4)])
def test_sample_space_form_is_limmas_form_at_50_digits(nf, p, seed):
    import mpmath as mp
    mp.mp.dps = rr.DPS
    rng = np.random.default_rng(seed)
    D = rr.make_design(nf, p, rng)
    for _ in range(3):
        x = rng.normal(size=nf)
        R = [mp.mpf(float(v)) for v in rng.normal(size=nf - p + 1)]
        nrm = mp.sqrt(mp.fsum(v * v for v in R))
        R = [v / nrm for v in R]
        lB, B, lss, ss = rr.identity_mp(x, D, R)
        assert abs(lB - B) <= mp.mpf(10) ** -40 * max(1, abs(B)), (lB, B)
        assert abs(lss - ss) <= mp.mpf(10) ** -40 * max(1, abs(ss)), (lss, ss)


def test_numpy_restatement_deviates_by_what_measured_records():
    worst = rr.measure_np()
    print("[measure] roast numpy against 50 digits: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():      # (the BLAS at hand may add in another order: half as much again either way, no more)
        assert 0.5 * rr.MEASURED[k] <= v <= 1.5 * rr.MEASURED[k], (k, v)


@pytest.mark.parametrize("stat", rr.STATS)
@pytest.mark.parametrize("name", rr.E2E_CASES)
def test_no_rotation_lies_within_twice_the_allowance_of_the_observed_statistic(name, stat):
    allowance = rr.FACTOR * rr.MEASURED[stat]
    for j, ref in enumerate(rr.e2e_reference(name, stat)):
        print(f"[gap] {name} {stat} contrast {j}: {ref['gap']:.3g} (allowance {allowance:.3g})")
        assert ref["gap"] > 2 * allowance


def test_finish_is_step_6_exactly():
    rng = np.random.default_rng(5)
    m, nrot = 40, 199
    cnt = rng.integers(0, nrot + 1, size=(m, 4))
    cnt[3, :2] = [7, 7]                      # p_up = p_down: Down
    cnt[4, :2] = [8, 7]                      # p_up < p_down: Up
    cnt[:6, 2] = 0                           # several sets at the smallest p: BH ties
    msize = rng.integers(1, 30, size=m).astype(np.float64)
    msize[7] = 0
    msize[9] = engine.ROAST_MEAN50_MAX + 1
    msize[10] = engine.ROAST_MEAN50_MAX
    nd, nu = np.floor(msize * 0.25), np.floor(msize * 0.5)
    for stat in rr.STATS:
        for midp in (True, False):
            got = engine.roast_finish(cnt, msize, nd, nu, nrot, stat, midp)[:, :, 0, 0]
            want = rr.finish_np(cnt, msize, nd, nu, nrot, stat, midp)
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), (stat, midp, np.argwhere(got != want)[:5])
            assert got[3, 3] == -1.0 and got[4, 3] == 1.0
            assert np.isnan(got[7, 1:]).all() and got[7, 0] == 0
            assert np.isnan(got[9, 3:]).all() == (stat == "mean50") and not np.isnan(got[10, 3:]).any()
            ok = ~np.isnan(got[:, 4])
            assert (got[ok, 5] >= got[ok, 4]).all() and (got[ok, 7] >= got[ok, 6]).all()      # FDR >= p, midp's pmax included
            assert got[ok, 4].min() == 1.0 / (nrot + 1)
    # midp lowers the FDR somewhere, and never below p
    a = engine.roast_finish(cnt, msize, nd, nu, nrot, "mean", True)[:, 5, 0, 0]
    b = engine.roast_finish(cnt, msize, nd, nu, nrot, "mean", False)[:, 5, 0, 0]
    assert (a[~np.isnan(a)] <= b[~np.isnan(b)]).all() and (a[~np.isnan(a)] < b[~np.isnan(b)]).any()


def test_finish_for_several_contrasts_and_fits_is_the_single_calls():
    rng = np.random.default_rng(6)
    m, q, nfit, nrot = 9, 2, 3, 49
    cnt = rng.integers(0, nrot + 1, size=(m, 4, q, nfit))
    msize = rng.integers(0, 5, size=(m, nfit)).astype(np.float64)
    nd, nu = rng.integers(0, 2, size=(m, q, nfit)) * (msize[:, None, :] > 0), np.zeros((m, q, nfit))
    got = engine.roast_finish(cnt, msize, nd, nu, nrot, "msq", True)
    for f in range(nfit):
        for j in range(q):
            want = rr.finish_np(cnt[:, :, j, f], msize[:, f], nd[:, j, f], nu[:, j, f], nrot, "msq", True)
            assert np.array_equal(got[:, :, j, f].view(np.int64), want.view(np.int64)), (f, j)


def test_mean50_threshold_form_is_the_mean_of_the_h_largest():
    rng = np.random.default_rng(8)
    cols = []
    for m in (1, 2, 3, 4, 7, 64, 65):
        z = rng.normal(size=(m, 6))
        z[:, 1] = np.round(z[:, 1])                     # many ties, +-0.0 among them
        z[:, 2] = 1.25                                  # all equal
        z[:, 3] = np.abs(z[:, 3])                       # one sign only
        z[:, 4] = np.where(np.arange(m) % 2, 0.0, -0.0)
        if m > 2:
            z[0, 5] = z[m // 2, 5] = np.sort(z[:, 5])[::-1][m // 2]     # two identical values straddling tau
        got = rr.stats_np(z, "mean50")
        want = rr.stats_mp(z.tolist(), "mean50")
        for k in range(6):
            for e in range(4):
                assert abs(got[k, e] - float(want[k][e])) <= 4 * m * rr.U * max(1.0, abs(float(want[k][e]))), (m, k, e)
        assert not np.signbit(got[4]).any()
        cols.append(got)
