"""The references of tests/test_gpu_plaid_test_contrasts.py::test_contrasts_with_excluded_samples_against_the_subset, from
the reference alone (host only): with gsetX given, no set of any contrast may be "not separable" -- so the GPU test, which
counts them, checks every set -- and the cases are what that test says they are."""
import numpy as np
import pytest

from tests.helpers import contrast_hooks as ch
from tests.helpers import exact_stats as xs

mpmath = pytest.importorskip("mpmath")


@pytest.mark.parametrize("case", ch.EXCLUSION_CASES)
def test_every_set_of_every_contrast_is_separable(case):
    X, Y, Gp, Gi, S = ch.exclusion_case(*case)
    n = X.shape[1]
    assert Y.shape == (n, 3) and set(np.unique(Y)) == {ch.NA, 0, 1}
    assert np.all(np.abs((Y == ch.NA).mean(axis=0) - 0.3) < 0.1)              # about 30 % NA per contrast
    assert (Y[:128, 1] == 1).sum() >= 2 and not (Y[128:, 1] == 1).any()       # group 1 inside the first column block
    assert (Y[:, 2] == 1).sum() == 1                                          # a group of one
    for j in range(3):
        sel, y = ch.subset(Y, j)
        assert len(sel) < n and (y == 0).sum() >= 2
        for k, (one, two) in enumerate(xs.crossprod_intervals(X[:, sel], y, Gp, Gi)):
            assert one is not None and two is not None, (case, j, k)
            assert one[0] <= one[1] and two[0] <= two[1]
        fc, fb, wiv = ch.welch_intervals(S[:, sel], y)
        assert np.isfinite(fc).all() and np.isfinite(fb).all()
        for k, iv in enumerate(wiv):
            assert iv is not None, (case, j, k)
            if j == 2:
                assert iv == "degenerate"                                     # p.lm = 1 - 1e-99: a variance of 0 / 0
            else:
                assert not isinstance(iv, str) and iv[0] <= iv[1] < 1.0, (case, j, k, iv)


def test_subset_of_a_contrast():
    Y = np.array([[0, ch.NA], [1, 1], [ch.NA, 0], [0, ch.NA]], dtype=np.int32)
    sel, y = ch.subset(Y, 0)
    assert sel.tolist() == [0, 1, 3] and y.tolist() == [0, 1, 0]
    sel, y = ch.subset(Y, 1)
    assert sel.tolist() == [1, 2] and y.tolist() == [1, 0]
