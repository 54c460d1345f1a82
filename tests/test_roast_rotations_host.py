"""plaid.roast's rotations (plaidhip_roast_rotations; include/plaidhip.h: plaidhip_roast, step 2), without a GPU.

  1. Every rotation is a unit vector: |r0^2 + |w|^2 - 1| <= 4 x 2^-53, the sum taken exactly (rationals).  The sum under
     the root is kept in double-double (fp64 operations only, pinned in the header), so s is its rounded root; each entry then carries one rounding of its division: 2u from the
     squares, u from s^2, and the rest is second order.
  2. w is orthogonal to the design within a derived bound.  With a = Q1'nu and wt = nu - Q1 a in floating point,
       |Q1'wt|_k <= |(I - Q1'Q1) a|_k + gamma_n sum_c |Q1_ck| |nu_c| + gamma_{p+1} sum_c |Q1_ck| (|nu_c| + sum_j |Q1_cj| |a_j|):
     the loss of orthogonality of Q1 itself (measured from the Q1 that plaidhip_limma_design returns), the chain of a_k, and
     the p products and p additions of the projection.  nu is recovered as wt + Q1 a up to the same terms, so the bound is
     taken on s w with |nu_c| <= |s w_c| + sum_j |Q1_cj| |a_j| and doubled.
  3. Exact 0.0 on the samples the fit leaves out.
  4. A draw is a function of (seed, fit, k, i) alone: the first rotations of a longer call are those of a shorter one, bit
     for bit; another seed or fit number gives other bits.
  5. The first 10^5 standard normals (the library's hook) have mean and variance within 5 sigma of 0 and 1."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from plaid_amd import _lib, engine
from tests.helpers import roast_ref as rr

U = 2.0 ** -53
CASES = [(5, 2, False), (14, 3, True), (131, 5, True), (260, 2, False)]


def case(n, p, masked):
    rng = np.random.default_rng(n + p)
    D = rr.make_design(n, p, rng)
    use = None
    if masked:
        use = np.ones(n, dtype=np.int8)
        use[rng.choice(np.arange(p + 2, n), size=max(1, n // 5), replace=False)] = 0
    return D, use


@pytest.mark.parametrize("n,p,masked", CASES)
def test_rotations_are_unit_vectors_orthogonal_to_the_design(n, p, masked):
    D, use = case(n, p, masked)
    nrot = 65
    W = engine.roast_rotations(D, use, fit=0, nrot=nrot, seed=3)
    assert W.shape == (n + 1, nrot) and np.isfinite(W).all()
    worst = 0.0
    for k in range(nrot):
        ss = sum(Fraction(float(v)) ** 2 for v in W[:, k])
        worst = max(worst, abs(float(ss - 1)))
    print(f"[rotations] n={n} p={p}: worst |r0^2 + |w|^2 - 1| = {worst:.3g}")
    assert worst <= 4 * U
    if use is not None:
        assert (W[1:][use == 0] == 0.0).all() and not np.signbit(W[1:][use == 0]).any()
        assert (W[1:][use != 0] != 0.0).all()
    Q = engine.limma_design(D, use, fit=1)["Q"]                  # n x p, zero on the samples left out
    E = np.abs(np.eye(p) - Q.T @ Q) + n * U                      # (the product above is itself rounded)
    gam = lambda k: k * U / (1 - k * U)
    aQ = np.abs(Q)
    for k in range(nrot):
        w = W[1:, k]
        a_hi = aQ.T @ np.abs(w) + p * np.abs(aQ.T @ aQ).max() * np.abs(w).max()      # |a| / s, generously
        nu = np.abs(w) + aQ @ a_hi
        bound = E @ a_hi + gam(n) * (aQ.T @ nu) + gam(p + 1) * (aQ.T @ (nu + aQ @ a_hi))
        got = np.abs(Q.T @ w)
        assert (got <= 2 * bound + n * U * (aQ.T @ np.abs(w))).all(), (k, got, bound)


def test_a_draw_depends_on_seed_fit_rotation_and_index_alone():
    D, use = case(14, 3, True)
    full = engine.roast_rotations(D, use, fit=2, nrot=130, seed=9)
    for part in (1, 63, 64, 65):
        assert np.array_equal(engine.roast_rotations(D, use, fit=2, nrot=part, seed=9).view(np.int64),
                              full[:, :part].view(np.int64)), part
    assert not np.array_equal(engine.roast_rotations(D, use, fit=2, nrot=130, seed=10), full)
    assert not np.array_equal(engine.roast_rotations(D, use, fit=1, nrot=130, seed=9), full)
    # the mask changes which samples are drawn for, not what is drawn: a rotation's nu_0 / |.| ratio aside, signs agree
    other = engine.roast_rotations(D, None, fit=2, nrot=130, seed=9)
    assert (np.sign(other[0]) == np.sign(full[0])).all()


def test_the_normals_are_standard():
    fn = _lib.load().plaidhip_debug_roast_normals
    fn.argtypes, fn.restype = [C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p], None
    x = np.empty(100000)
    fn(1, 0, 0, 0, len(x), x.ctypes.data)
    n = len(x)
    assert np.isfinite(x).all()
    assert abs(x.mean()) <= 5 / np.sqrt(n)
    assert abs(x.var() - 1) <= 5 * np.sqrt(2 / n)
    y = np.empty(1000)
    fn(1, 0, 1, 0, len(y), y.ctypes.data)                      # the next rotation: other draws
    assert not np.array_equal(x[:1000], y)
    assert abs(np.corrcoef(x[:1000], y)[0, 1]) <= 5 / np.sqrt(1000)


def test_the_entry_checks_its_arguments():
    lib = _lib.load()
    D = np.asfortranarray(np.column_stack([np.ones(4), np.arange(4.0)]))
    W = np.zeros((5, 3))
    ptr = lambda a: a.ctypes.data
    err = lambda: lib.plaidhip_last_error_string().decode()
    assert lib.plaidhip_roast_rotations(ptr(D), 4, 2, None, 0, 0, 1, ptr(W)) == _lib.EINVAL and "nrot = 0" in err()
    assert lib.plaidhip_roast_rotations(ptr(D), 4, 0, None, 0, 3, 1, ptr(W)) == _lib.EINVAL and "coefficients" in err()
    assert lib.plaidhip_roast_rotations(ptr(D), 4, 2, None, 0, 3, 1, None) == _lib.EINVAL and "null W" in err()
    assert lib.plaidhip_roast_rotations(ptr(D), 2, 2, None, 0, 3, 1, ptr(W)) == _lib.EINVAL and "fit 1 has 2 samples" in err()
    assert lib.plaidhip_roast_rotations(ptr(D), 4, 2, None, 0, 3, 1, ptr(W)) == _lib.OK
