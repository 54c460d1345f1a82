"""replaid.plage on the device (plaidhip_plage, kernels_plage.hip), certified without trusting any SVD.

With Z_s recomputed in extended precision and v the device row: mu = |Z_s v|^2 / |v|^2, rho = |Z_s'Z_s v - mu v|;
trace(C) = k (n - 1) exactly and C is positive semi-definite, so lambda_2 <= trace - mu and sin angle(v, v_1) <= rho /
(2 mu - trace).  rho must lie within tol lambda plus the rounding terms of plage_ref.plage_rounding (the Gram sums, the
projection, the standardization: DESIGN.md section 22).  numpy's oriented svd row is certified the same way and the device
row must lie within the sum of the two certified angles of it.  The inputs carry one planted factor (loadings in [0.85,
0.97], a quarter negative); that 2 mu - trace >= trace / 4 is asserted on the host, from the reference alone, before the
device is touched; no set is skipped.

g = 600 genes and n = 2, 3, 65, 130, 257 samples (the remainders of the 16-sample trip of the Gram loop and of the
projection's 256-sample blocks); the effective sizes of plage_ref.SIZES, whose edges are named there, plus 0; the special
sets of plage_ref.build_case; the exactly orthogonal pair; one case at g = 20,480.  dgCMatrix input, every sharding through
the hook, a repeated call: the same bits."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from plaid_amd import engine
from tests.helpers import plage_hooks
from tests.helpers import plage_ref as ref

pytestmark = pytest.mark.gpu

SAMPLES = (2, 3, 65, 130, 257)
TOL = ref.TOL
LD = ref.LD


def same(a, b, what=""):
    assert a.shape == b.shape
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}"


@functools.lru_cache(maxsize=None)
def case(n, g=600):
    c = ref.build_case(n, ref.SEEDS[n]) if g == 600 else ref.build_case(n, 1, g=g, sizes=(17, 65, 129), extras=False)
    sep = ref.separated(c)
    for nm, r in sep.items():     # on the host, from the reference alone, before the device is touched; none is skipped
        assert r["ok"], (n, nm, float(r["cert"]["gap"]), float(r["cert"]["trace"]))
    return c, sep


@functools.lru_cache(maxsize=None)
def ctx():
    return engine.Context(0)


def check(c, sep):
    X, Gp, Gi, names = c["X"], c["Gp"], c["Gi"], c["names"]
    n = X.shape[1]
    S, info, L = ctx().plage(X, Gp, Gi, loadings=True)
    _, _, flag = ref.moments(X)
    for s, nm in enumerate(names):
        rows, pos, bad = ref.members(Gp, Gi, flag, s)
        k = len(rows)
        assert info[s, 0] == k, nm
        seg = L[Gp[s]:Gp[s + 1]]
        dropped = np.setdiff1d(np.arange(Gp[s + 1] - Gp[s]), pos)
        assert (seg[dropped] == 0).all(), nm                       # a dropped constant member
        if bad or k == 0:
            assert np.isnan(S[s]).all() and np.isnan(info[s, [1, 2, 4]]).all() and (info[s, [3, 5]] == 0).all(), nm
            assert np.isnan(seg[pos]).all(), nm
            continue
        r = sep[nm]
        lam, expl, its, res, conv = info[s, 1:]
        assert conv == 1 and res <= TOL and 1 <= its <= 1000, (nm, info[s])
        v, u = S[s], seg[pos]
        assert np.isfinite(v).all() and np.isfinite(u).all()
        R, dv, dC = ref.plage_rounding(X, rows, lam)
        cd, cn = ref.certify(r["Zl"], v), r["cert"]
        trace = float(cd["trace"])
        # the certificate
        assert float(cd["rho"]) <= TOL * lam + 1.01 * R, (nm, float(cd["rho"]), TOL * lam, R)
        assert cd["gap"] >= cd["trace"] / 4 * (1 - 1e-9), nm
        # against numpy's oriented row: within the sum of the two certified angles (chord <= angle)
        angle = np.arcsin(float(cd["sin"])) + np.arcsin(float(cn["sin"]))
        dist = float(np.sqrt(((cd["w"] - cn["w"]) ** 2).sum()))
        assert dist <= angle + 8 * ref.U, (nm, dist, angle)
        # |v| = 1: v = Z'u / sqrt(u'Cu) has norm 1 for any unit u; what is left is rounding
        unit = 1.01 * ((k + 4) * ref.U + (3 * k * ref.U * trace + dC) / lam + dv)
        assert abs(float(cd["norm"]) - 1) <= unit, (nm, float(cd["norm"]) - 1, unit)
        # lambda = u'Cu and mu differ by r^2 / lambda <= tol^2 lambda in exact arithmetic
        dl = TOL * TOL * lam + 1.01 * R
        assert abs(lam - float(cd["mu"])) <= dl, (nm, lam - float(cd["mu"]), dl)
        de = dl / trace + 1.01 * (lam / trace) * (dC + (k + 1) * ref.U * trace) / trace
        assert abs(expl - float(cd["mu"]) / trace) <= de, (nm, expl, de)
        # the loadings: Z v / sqrt(lambda) = C u / lambda = u + (residual) / lambda
        zv = (r["Zl"] @ v.astype(LD)) / np.sqrt(LD(lam))
        dl_u = TOL + 1.01 * (R / lam + dv * np.sqrt(trace / lam))
        assert float(np.sqrt(((zv - u.astype(LD)) ** 2).sum())) <= dl_u, (nm, dl_u)
        assert abs(float(np.sqrt((u.astype(LD) ** 2).sum())) - 1) <= 1.01 * (k + 4) * ref.U
        # the orientation rule itself
        assert ref.orient(u) == 1.0, nm
        print(f"plage n={n} {nm}: k={k} iterations={int(its)} residual={res:.2e} rho={float(cd['rho']):.2e} "
              f"allowed={TOL * lam + 1.01 * R:.2e} sin={float(cd['sin']):.2e} dist={dist:.2e} angle={angle:.2e}")
    return S, info, L


@pytest.mark.parametrize("n", SAMPLES)
def test_rows_are_certified_and_meet_numpy_within_the_certified_angles(n):
    c, sep = case(n)
    S, info, L = check(c, sep)
    nm, Gp = c["names"], c["Gp"]
    for k in ref.SIZES:
        assert info[nm.index(f"k{k}"), 0] == k
    assert info[nm.index("empty"), 0] == 0 and info[nm.index("constants"), 0] == 0
    assert info[nm.index("one_constant"), 0] == 16 and info[nm.index("identical"), 0] == 6
    one = nm.index("k1")
    assert L[Gp[one]] == 1.0 and info[one, 3] == 1 and info[one, 4] == 0.0      # u = (1), one step, no residual
    # a mixed-sign set with sum u far from 0 comes out with sum u > 0; the negative pair with member 0 positive
    a = c["loadings"]
    big = nm.index("k65")
    u = L[Gp[big]:Gp[big + 1]]
    planted = a[c["Gi"][Gp[big]:Gp[big + 1]]]
    assert (planted < 0).any() and u.sum() > 0
    if n > 3:   # (with 2 or 3 samples the sample correlations need not carry the planted signs)
        assert (np.sign(u) == np.sign(planted)).all() and u.sum() > 0.2 * np.abs(u).sum()
    neg = nm.index("negative_pair")
    u = L[Gp[neg]:Gp[neg + 1]]
    if u[0] * u[1] < 0 and abs(u.sum()) <= 2.0 ** -20 * np.abs(u).sum():
        assert u[0] > 0 > u[1]
    if n > 3:
        assert u[0] > 0 > u[1] and abs(abs(u[0]) - abs(u[1])) < 1e-9


def test_rows_past_16_bits():
    c, sep = case(65, 20480)
    assert len(c["names"]) == 3 and int(c["Gi"].max()) >= 16384 and c["X"].shape == (20480, 65)
    check(c, sep)


def test_orthogonal_pair():
    """lambda_1 = lambda_2: only a unit v, a zero residual and the iteration's own deterministic answer (the start, column 0)"""
    X = np.asfortranarray(np.random.default_rng(4).normal(size=(600, 4)))
    X[0] = [1.0, -1.0, 1.0, -1.0]
    X[1] = [1.0, 1.0, -1.0, -1.0]
    Gp, Gi = np.array([0, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    S, info, L = ctx().plage(X, Gp, Gi, loadings=True)
    assert info[0, 0] == 2 and info[0, 4] == 0.0 and info[0, 5] == 1 and info[0, 3] == 1, info
    assert L.tolist() == [1.0, 0.0]
    assert abs(np.linalg.norm(S[0]) - 1) <= 8 * ref.U
    z = ref.standardize(X[:2])[0]
    np.testing.assert_allclose(S[0], z[0] / np.sqrt(info[0, 1]), rtol=4 * ref.U, atol=0)
    assert abs(info[0, 2] - 0.5) <= 8 * ref.U


def test_the_mfma_gram_kernel_meets_the_same_certificates():
    """the v_mfma_f64_16x16x4_f64 form of plage_gram_kernel (behind the test hook; not what the product launches): the
    bounds hold whether products fuse or not, the remainders of its 16-sample trip at n = 65 and n = 130 included.  On the
    orthogonal pair it leaves a rounding residue in C_01 where the product's kernel leaves an exact zero, which is why the
    product does not launch it."""
    X = np.asfortranarray(np.random.default_rng(4).normal(size=(600, 4)))
    X[0] = [1.0, -1.0, 1.0, -1.0]
    X[1] = [1.0, 1.0, -1.0, -1.0]
    plage_hooks.gram_mode(1)
    try:
        for n in (65, 130):
            check(*case(n))
        _, info = ctx().plage(X, np.array([0, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32))
    finally:
        plage_hooks.gram_mode(0)
    print("orthogonal pair on the MFMA form:", info.tolist())
    assert info[0, 5] == 1 and info[0, 4] <= 4 * ref.U and abs(info[0, 2] - 0.5) <= 8 * ref.U


def sparse_case():
    c, _ = case(65)
    rng = np.random.default_rng(11)
    X = np.asfortranarray(np.where(rng.random(c["X"].shape) < 0.6, 0.0, np.nan_to_num(c["X"], nan=1.5, posinf=2.5)))
    X[-3, 7] = np.nan
    return X, c["Gp"], c["Gi"]


def test_bits_dgcmatrix_shards_and_repeats():
    X, Gp, Gi = sparse_case()
    first = ctx().plage(X, Gp, Gi, loadings=True)
    for what, other in (("a second call", ctx().plage(X, Gp, Gi, loadings=True)),
                        ("dgCMatrix", ctx().plage(sp.csc_matrix(X), Gp, Gi, loadings=True)),
                        ("plage_multi", engine.plage_multi(sp.csc_matrix(X), Gp, Gi, loadings=True, devices=1))):
        for a, b in zip(first, other):
            same(a, b, what)
    assert np.isnan(first[0]).any() and np.isfinite(first[0]).any()
    same(first[0], ctx().plage(X, Gp, Gi)[0], "without the loadings")
    for c in (case(65)[0], case(3)[0]):
        base = plage_hooks.plage(1, c["X"], c["Gp"], c["Gi"], loadings=True)
        for a, b in zip(base, ctx().plage(c["X"], c["Gp"], c["Gi"], loadings=True)):
            same(a, b, "hook against context")
        for shards in (2, 3, 7):           # (7 > 3: more shards than columns)
            for a, b in zip(base, plage_hooks.plage(shards, c["X"], c["Gp"], c["Gi"], loadings=True)):
                same(a, b, f"{shards} shards")


def test_one_step_reports_what_it_reached():
    c, _ = case(65)
    S, info = ctx().plage(c["X"], c["Gp"], c["Gi"], maxit=1)
    _, _, flag = ref.moments(c["X"])
    for s, nm in enumerate(c["names"]):
        rows, _, bad = ref.members(c["Gp"], c["Gi"], flag, s)
        if bad or len(rows) == 0:
            continue
        assert np.isfinite(S[s]).all() and info[s, 3] == 1, nm
        assert info[s, 5] == (1.0 if info[s, 4] <= TOL else 0.0), nm      # converged only where one step suffices
    assert info[c["names"].index("k257"), 5] == 0 and info[c["names"].index("k1"), 5] == 1


def test_a_failing_shard_fails_the_call():
    c, _ = case(3)
    with pytest.raises(Exception, match="injected failure"):
        plage_hooks.plage(3, c["X"], c["Gp"], c["Gi"], fail=1)


def test_replaid_plage_and_replaid_zscore_by_name():
    """the R-style entries: genes aligned by name, sets outside [minSize, maxSize] dropped, dense or sparse X, the bits of the
    engine call on the aligned operands"""
    import plaid_amd
    c, _ = case(65)
    g = c["X"].shape[0]
    genes = [f"g{i}" for i in range(g)]
    samples = [f"s{j}" for j in range(65)]
    M = np.zeros((g, len(c["names"])))
    for s in range(len(c["names"])):
        M[c["Gi"][c["Gp"][s]:c["Gp"][s + 1]], s] = 1.0
    order = np.random.default_rng(2).permutation(g)                      # matG's rows in another order than X's
    G = plaid_amd.NamedMatrix(sp.csc_matrix(M[order]), [genes[i] for i in order], list(c["names"]))
    X = plaid_amd.NamedMatrix(c["X"], genes, samples)
    S, info, load = plaid_amd.replaid_plage(X, G, minSize=2, maxSize=256, loadings=True, ctx=ctx())
    kept = [nm for s, nm in enumerate(c["names"]) if 2 <= c["Gp"][s + 1] - c["Gp"][s] <= 256]
    assert S.rownames == kept and S.colnames == samples and info.rownames == kept
    assert list(info.colnames) == list(engine.PLAGE_COLUMNS) and "k257" not in kept and "k1" not in kept and "empty" not in kept
    # the aligned pattern lists a set's members in another order: the same set, so both rows lie within the certified
    # angle of v_1, rho <= tol lambda + 1.01 R over a gap of at least trace / 4, and within the bound on | |v| - 1 | of unit
    base, binfo = ctx().plage(c["X"], c["Gp"], c["Gi"])
    _, _, flag = ref.moments(c["X"])
    for q, nm in enumerate(kept):
        s = c["names"].index(nm)
        assert info.values[q, 0] == binfo[s, 0]
        if np.isnan(base[s]).all():
            assert np.isnan(S.values[q]).all()
            continue
        rows, _, _ = ref.members(c["Gp"], c["Gi"], flag, s)
        k, lam, trace = len(rows), binfo[s, 1], len(rows) * 64.0
        R, dv, dC = ref.plage_rounding(c["X"], rows, lam)
        allow = 2 * np.arcsin((TOL * lam + 1.01 * R) / (trace / 4)) + 2 * 1.01 * ((k + 4) * ref.U + (3 * k * ref.U * trace + dC) / lam + dv)
        d = np.linalg.norm(S.values[q] - base[s])
        if nm == "negative_pair":     # sum u ~ 0: the first member in the order GIVEN is made positive, and the orders differ
            d = min(d, np.linalg.norm(S.values[q] + base[s]))
        assert d <= allow, (nm, d, allow)
        names, u = load[nm]
        assert len(names) == c["Gp"][s + 1] - c["Gp"][s] and set(names) == {genes[i] for i in c["Gi"][c["Gp"][s]:c["Gp"][s + 1]]}
        assert abs(np.linalg.norm(u) - 1) < 1e-12 and ref.orient(u[u != 0]) == 1.0
    Ss, infos = plaid_amd.replaid_plage(plaid_amd.NamedMatrix(sp.csc_matrix(np.nan_to_num(c["X"], posinf=9.0)), genes, samples), G,
                                        minSize=2, maxSize=256, ctx=ctx())
    Sd, infod = plaid_amd.replaid_plage(plaid_amd.NamedMatrix(np.nan_to_num(c["X"], posinf=9.0), genes, samples), G, minSize=2,
                                        maxSize=256, ctx=ctx())
    same(Ss.values, Sd.values, "sparse X")
    same(infos.values, infod.values, "sparse X")
    Z = plaid_amd.replaid_zscore(X, G, ctx=ctx())
    assert Z.rownames == list(c["names"]) and Z.colnames == samples
    zb, _ = ctx().zscore(c["X"], c["Gp"], c["Gi"])
    assert np.array_equal(np.isnan(Z.values), np.isnan(zb))
    for s, nm in enumerate(c["names"]):      # the members summed in another order: twice the forward bound apart at the most
        rows, _, bad = ref.members(c["Gp"], c["Gi"], flag, s)
        if not bad and len(rows):
            bound = ref.zscore_bound(c["X"], rows, int(c["Gp"][s + 1] - c["Gp"][s]), zb[s])
            assert (np.abs(Z.values[s] - zb[s]) <= 2 * bound).all(), nm
    with pytest.raises(ValueError, match="a set of 257 members|maxSize"):
        plaid_amd.replaid_plage(X, G, maxSize=5000, ctx=ctx())
