"""plaid.limma on the device -- `pytest -m gpu`.

  1. plaidhip_dev_row_design_effects against the exact dot products of the same doubles (integers), with the Q of
     plaidhip_limma_design, at the summation bound derived in DESIGN.md section 20;
  2. plaidhip_dev_row_design_rss against the exact value of its own pinned expression at the effects the device returned, at
     the bound derived there;
  3. `use`: NaN and +-Inf in excluded samples change no bit, and a fit that uses every sample has, inside a multi-fit call,
     the bits of that fit called alone;
  4. plaid_limma and plaid_limma_contrasts end to end against limma_np on the five branch cases, at a MEASURED tolerance;
  5. plaidhip_limma_multi's engine with 1 / 2 / 3 / 5 / 9 shards: the one-device bits; a failing shard's message;
  6. the hallmark sets on the 50-cell fixture: replaid_gsva_exact -> plaid_limma_contrasts, and plaid_limma_contrasts on the
     genes -> plaid_sig -> plaid_fisher.

The shapes are the smallest at which the kernels can go wrong: rows 515 (odd: a second 512-row workgroup, the 8-byte loads) and
514 (the 16-byte loads), one case with ld = rows + 3; n = 131 (a full 128-column block and a tail of 3, no multiple of the
8-deep unroll) and 300 (three blocks); (p, nfit) with W = nfit (p + 1) = 3, 12, 9, 20, 33 weight columns: a lone partial tile,
fits that straddle a tile boundary, a last tile of one column, and every register count of the RSS kernel (p <= 4, 8, 16, 32).
The exact checks 1 and 2 take every combination; their device results and references are computed once and shared."""
import os

import numpy as np
import pytest

from plaid_amd import _lib, engine
from tests.helpers import exact_ref as er
from tests.helpers import limma_ref as lr

pytestmark = pytest.mark.gpu

# end to end against limma_np: the worst relative deviation measured on an MI355X in the first run (the constant rows' t and
# logFC, whose reference is 0, relative to the size of the terms that cancel: limma_ref.dev_t), and what is asserted: 8 times it, and never looser than 1e-9
MEASURED = {"t": 6.5e-13, "p": 1.3e-13, "logFC": 2.3e-13, "df_prior": 4.0e-16, "s2_prior": 1.9e-15}
FACTOR = 8
BOUND = {k: FACTOR * v for k, v in MEASURED.items()}
assert all(b <= 1e-9 for b in BOUND.values())

# rows, n, p, nfit, pad (ld = rows + pad)
EXACT_CASES = [(rows, n, p, nfit, 0) for rows in (515, 514) for n in (131, 300)
               for p, nfit in ((2, 1), (3, 3), (8, 1), (9, 2), (32, 1))] + [(514, 131, 3, 3, 3)]
BIT_CASES = [(515, 131, 3, 3, 0), (514, 300, 9, 2, 0), (514, 131, 2, 2, 1)]


def make_fits(n, p, nfit, rng, masked_single=False):
    """nfit designs [1, group, covariates ...] (n x p; p = 1: the intercept alone) and use (n x nfit int8, or None): fit 0 uses
    every sample, the others leave about 30 % out; a single fit leaves a third out when `masked_single`"""
    D = np.empty((n, p, nfit), order="F")
    for f in range(nfit):
        D[:, 0, f] = 1.0
        if p > 1:
            D[:, 1, f] = rng.permutation(np.arange(n) % 2)
        if p > 2:
            D[:, 2:, f] = rng.normal(size=(n, p - 2))
    if nfit == 1 and not masked_single:
        return D, None
    use = np.ones((n, nfit), dtype=np.int8, order="F")
    for f in range(0 if nfit == 1 else 1, nfit):
        use[rng.random(n) < 0.3, f] = 0
        use[:p + 2, f] = 1
    return D, use


def fit_Q(D, use):
    """(Q n x p x nfit, n_f) of the library's own decomposition"""
    n, p, nfit = D.shape
    Q = np.empty((n, p, nfit), order="F")
    nf = []
    for f in range(nfit):
        d = engine.limma_design(D[:, :, f], None if use is None else use[:, f], fit=f + 1)
        Q[:, :, f] = d["Q"]
        nf.append(d["nf"])
    return Q, np.array(nf, dtype=np.int64)


def device_passes(ctx, A, ld, Q, use, nf, seedE=None, seedR=None):
    """(E [W][rows], rss [nfit][rows]) of the two device entries on A (rows x n) held with leading dimension ld; the buffers
    carry sentinels that are checked"""
    import torch
    dev = torch.device("cuda", 0)
    rows, n = A.shape
    _, p, nfit = Q.shape
    W = nfit * (p + 1)
    Ad = torch.full((n, ld), 777.0, dtype=torch.float64, device=dev)
    Ad[:, :rows] = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)
    Qd = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).to(dev)       # [nfit][p][n] = n x p x nfit column-major
    Ud = None if use is None else torch.from_numpy(np.ascontiguousarray(use.T)).to(dev)
    inv = torch.from_numpy(1.0 / nf.astype(np.float64)).to(dev)
    E = torch.full((W * rows + 5,), -7.0, dtype=torch.float64, device=dev)
    R = torch.full((nfit * rows + 5,), -7.0, dtype=torch.float64, device=dev)
    sE = None if seedE is None else torch.from_numpy(np.ascontiguousarray(seedE)).to(dev)
    sR = None if seedR is None else torch.from_numpy(np.ascontiguousarray(seedR)).to(dev)
    torch.cuda.synchronize()
    uptr = None if Ud is None else Ud.data_ptr()
    ctx.dev_row_design_effects(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, inv.data_ptr(), p, nfit,
                               None if sE is None else sE.data_ptr(), E.data_ptr())
    ctx.dev_row_design_rss(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, p, nfit, E.data_ptr(),
                           None if sR is None else sR.data_ptr(), R.data_ptr())
    ctx.synchronize()
    e, r = E.cpu().numpy(), R.cpu().numpy()
    assert np.all(e[W * rows:] == -7.0) and np.all(r[nfit * rows:] == -7.0)
    assert np.all(Ad.cpu().numpy()[:, rows:] == 777.0)
    return e[:W * rows].reshape(W, rows), r[:nfit * rows].reshape(nfit, rows)


_CACHE = {}


def exact_case(ctx, case):
    """the inputs, the device results and nothing else of an EXACT_CASES entry, computed once for checks 1 and 2"""
    if case not in _CACHE:
        rows, n, p, nfit, pad = case
        rng = np.random.default_rng(list(case))
        D, use = make_fits(n, p, nfit, rng, masked_single=(p == 2))
        Q, nf = fit_Q(D, use)
        A = rng.normal(size=(rows, n)) * np.exp(rng.normal(size=(rows, 1))) + rng.normal(size=(rows, 1))
        E, rss = device_passes(ctx, A, rows + pad, Q, use, nf)
        _CACHE[case] = dict(A=A, Q=Q, use=use, nf=nf, E=E, rss=rss)
    return _CACHE[case]


@pytest.mark.parametrize("case", EXACT_CASES, ids=[f"rows{c[0]}-n{c[1]}-p{c[2]}-nfit{c[3]}-pad{c[4]}" for c in EXACT_CASES])
def test_effects_against_exact_dot_products(hip_ctx, case):
    c = exact_case(hip_ctx, case)
    rows, n, p, nfit, _ = case
    for f in range(nfit):
        used = np.ones(n, dtype=bool) if c["use"] is None else c["use"][:, f] != 0
        Wm = np.column_stack([c["Q"][:, :, f], np.full(n, 1.0 / c["nf"][f])]) * used[:, None]
        ref, mag = lr.exact_effects(c["A"], Wm)
        got = c["E"][f * (p + 1):(f + 1) * (p + 1)].T
        bound = lr.effects_bound(mag, int(c["nf"][f]))
        worst = float(np.max(np.abs(got - ref) / bound))
        print(f"[measure] effects {case} fit {f + 1}: worst error / bound {worst:.3g}")
        er.assert_within(got, ref, bound, f"effects {case} fit {f + 1}")


@pytest.mark.parametrize("case", EXACT_CASES, ids=[f"rows{c[0]}-n{c[1]}-p{c[2]}-nfit{c[3]}-pad{c[4]}" for c in EXACT_CASES])
def test_rss_against_its_exact_expression(hip_ctx, case):
    c = exact_case(hip_ctx, case)
    rows, n, p, nfit, _ = case
    for f in range(nfit):
        used = np.ones(n, dtype=bool) if c["use"] is None else c["use"][:, f] != 0
        Ef = c["E"][f * (p + 1):f * (p + 1) + p].T
        ref, r, rho = lr.exact_rss(c["A"], c["Q"][:, :, f], used, Ef)
        bound = lr.rss_bound(r, rho, ref, int(c["nf"][f]), p)
        worst = float(np.max(np.abs(c["rss"][f] - ref) / bound))
        print(f"[measure] rss {case} fit {f + 1}: worst error / bound {worst:.3g}")
        er.assert_within(c["rss"][f], ref, bound, f"rss {case} fit {f + 1}")
        # and it is a residual sum of squares: near the projection's, which is far below sum x^2 for these rows
        proj = ((c["A"][:, used] - Ef @ c["Q"][used, :, f].T) ** 2).sum(axis=1)
        np.testing.assert_allclose(c["rss"][f], proj, rtol=1e-9)


@pytest.mark.parametrize("case", BIT_CASES, ids=[f"rows{c[0]}-n{c[1]}-p{c[2]}-nfit{c[3]}-pad{c[4]}" for c in BIT_CASES])
def test_use_masks_and_seeds_change_no_bit(hip_ctx, case):
    rows, n, p, nfit, pad = case
    rng = np.random.default_rng(17 + rows + n)
    D, use = make_fits(n, p, nfit, rng)
    Q, nf = fit_Q(D, use)
    A = rng.normal(size=(rows, n)) + 3.0
    E0, R0 = device_passes(hip_ctx, A, rows + pad, Q, use, nf)
    assert np.isfinite(E0).all() and np.isfinite(R0).all() and (R0 > 0).all()
    for f in range(1, nfit):                 # a fit's excluded samples hold NaN and +-Inf instead: its own results keep their bits
        out = np.flatnonzero(use[:, f] == 0)
        assert len(out) >= 3
        Az = A.copy()
        Az[:, out] = 0.0
        Ez, Rz = device_passes(hip_ctx, Az, rows + pad, Q, use, nf)
        An = A.copy()
        An[:, out] = rng.choice([np.nan, np.inf, -np.inf], size=(rows, len(out)))
        En, Rn = device_passes(hip_ctx, An, rows + pad, Q, use, nf)
        sl = slice(f * (p + 1), (f + 1) * (p + 1))
        er.assert_same_bits(En[sl], Ez[sl], f"effects of fit {f + 1}, NaN / Inf in its excluded samples")
        er.assert_same_bits(Rn[f], Rz[f], f"rss of fit {f + 1}")
        er.assert_same_bits(Ez[sl], E0[sl], "the excluded samples' own values do not matter")
        er.assert_same_bits(Rz[f], R0[f])
        assert not np.isfinite(En[:p + 1]).any() and np.isnan(Rn[0]).all()   # fit 1 uses them: nothing of it is finite
    # fit 1 uses every sample: inside the multi-fit call it has the bits of the fit called alone (use = NULL)
    E1, R1 = device_passes(hip_ctx, A, rows + pad, Q[:, :, :1].copy(order="F"), None, nf[:1])
    er.assert_same_bits(E0[:p + 1], E1, "fit 1 alone")
    er.assert_same_bits(R0[0], R1[0], "fit 1 alone, rss")
    # a seed is what the blocks are added to, in order: two halves cut at a block boundary chain to the whole
    cut = 128
    Ea, _ = device_passes(hip_ctx, A[:, :cut], rows + pad, Q[:cut].copy(order="F"), use[:cut].copy(order="F"), nf)
    Eb, _ = device_passes(hip_ctx, A[:, cut:], rows + pad, Q[cut:].copy(order="F"), use[cut:].copy(order="F"), nf, seedE=Ea)
    er.assert_same_bits(Eb, E0, "effects chained over two column shards")


def _tables_against_np(tables, hyper, X, Y, B, worst):
    for j, (nm, tab) in enumerate(tables.items()):
        D, use = lr.contrast_design(Y, B, j)
        ref = lr.limma_np(X, D, use, [0.0, 1.0] + [0.0] * B.shape[1])
        h = hyper[nm]
        assert h["n.ok"] == ref["nok"] and h["df.residual"] == ref["df_residual"]
        assert np.isinf(h["df.prior"]) == np.isinf(ref["df_prior"]) and (h["df.prior"] == 0) == (ref["df_prior"] == 0)
        worst["df_prior"] = max(worst["df_prior"], lr.dev_rel(h["df.prior"], ref["df_prior"]))
        worst["s2_prior"] = max(worst["s2_prior"], lr.dev_rel(h["s2.prior"], ref["s2_prior"]))
        v = tab.values
        flat = lr.flat_rows(X, use)                       # constant rows: held to the size of the terms that cancel
        scale = np.abs(X[:, np.flatnonzero(use)[0]]) * ref["w1"][0]
        worst["logFC"] = max(worst["logFC"], lr.dev_t(v[:, 0], ref["logFC"][:, 0], flat, scale))
        with np.errstate(all="ignore"):
            worst["t"] = max(worst["t"], lr.dev_t(v[:, 2], ref["t"][:, 0], flat, scale / ref["se"][:, 0]))
        worst["p"] = max(worst["p"], lr.dev_p(v[:, 3], ref["p"][:, 0]))
        np.testing.assert_allclose(v[:, 1], ref["AveExpr"], rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(v[:, 5], ref["s2"], rtol=1e-9, atol=1e-24)
        np.testing.assert_array_equal(v[:, 4], lr.bh(v[:, 3]))


@pytest.mark.parametrize("name", lr.BRANCH_CASES)
def test_end_to_end_against_limma_np(hip_ctx, name):
    import plaid_amd
    X, Y, B = lr.branch_case(name)
    rows, n = X.shape
    S = plaid_amd.NamedMatrix(X, [f"set{r}" for r in range(rows)], [f"cell{c}" for c in range(n)])
    Yn = plaid_amd.NamedMatrix(Y, S.colnames, ["all", "some"])
    worst = dict.fromkeys(MEASURED, 0.0)
    tables, hyper = plaid_amd.plaid_limma_contrasts(S, Yn, B=B, ctx=hip_ctx)
    assert list(tables) == ["all", "some"] and tables["all"].rownames == S.rownames
    assert tables["all"].colnames == ["logFC", "AveExpr", "t", "P.Value", "adj.P.Val", "sigma2"]
    _tables_against_np(tables, hyper, X, Y, B, worst)
    # plaid_limma: the second contrast's design, its use, and a contrast matrix of two columns
    D, use = lr.contrast_design(Y, B, 1)
    K = plaid_amd.NamedMatrix(np.array([[0.0, 0.0], [1.0, 1.0], [0.0, -2.0]]), ["Intercept", "y", "b"], ["y", "y-2b"])
    t2, h2 = plaid_amd.plaid_limma(S, plaid_amd.NamedMatrix(D, S.colnames, ["Intercept", "y", "b"]), K, use=use, ctx=hip_ctx)
    assert list(t2) == ["y", "y-2b"]
    er.assert_same_bits(t2["y"].values, tables["some"].values, "plaid_limma and plaid_limma_contrasts, one fit")
    ref = lr.limma_np(X, D, use, K.values)
    flat = lr.flat_rows(X, use)
    scale = np.abs(X[:, np.flatnonzero(use)[0]]) * ref["w1"][1]
    with np.errstate(all="ignore"):
        worst["t"] = max(worst["t"], lr.dev_t(t2["y-2b"].values[:, 2], ref["t"][:, 1], flat, scale / ref["se"][:, 1]))
    worst["p"] = max(worst["p"], lr.dev_p(t2["y-2b"].values[:, 3], ref["p"][:, 1]))
    np.testing.assert_equal(h2, hyper["some"])          # (NaN equal to NaN: s2.prior with one ok row)
    print(f"[measure] end to end {name}: " + ", ".join(f"{k} {x:.3g}" for k, x in worst.items()))
    for k, x in worst.items():
        assert x <= BOUND[k], (k, x)
    # sort_by orders the rows; NaN rows last
    by_p = plaid_amd.plaid_limma_contrasts(S, Yn, B=B, sort_by="P.Value", ctx=hip_ctx)[0]["all"]
    pv = by_p.values[:, 3]
    k = int((~np.isnan(pv)).sum())
    assert np.all(np.diff(pv[:k]) >= 0) and np.isnan(pv[k:]).all() and sorted(by_p.rownames) == sorted(S.rownames)


@pytest.mark.parametrize("case", [(515, 300, 3, 3), (514, 131, 9, 2), (40, 7, 2, 1)])
def test_every_sharding_has_the_one_device_bits(hip_ctx, case):
    rows, n, p, nfit = case
    rng = np.random.default_rng(23 + n)
    D, use = make_fits(n, p, nfit, rng)
    A = rng.normal(size=(rows, n)) + rng.normal(size=(rows, 1))
    A[3, 1] = np.nan                                       # a row that is not ok
    K = rng.normal(size=(p, 2))
    out1, hyper1 = hip_ctx.limma(A, D, use, K)
    assert np.isnan(out1[3]).all() and np.isfinite(out1[:3]).all() and np.isfinite(hyper1[:, [0, 2, 3]]).all()
    for nshards in (1, 2, 3, 5, 9):                        # (n = 7: more shards than samples)
        status, out, hyper = lr.run_sharded(nshards, A, D, use, K)
        assert status == _lib.OK
        er.assert_same_bits(out, out1, f"{nshards} shards")
        er.assert_same_bits(hyper, hyper1, f"{nshards} shards, hyper")


def test_a_failing_shard_reports_and_writes_nothing(hip_ctx):
    rng = np.random.default_rng(29)
    D, use = make_fits(300, 3, 2, rng)
    A = rng.normal(size=(64, 300))
    status, out, hyper = lr.run_sharded(3, A, D, use, None, fail=1)
    text = _lib.load().plaidhip_last_error_string().decode()
    assert status == _lib.EHIP and "injected failure" in text, (status, text)
    assert (out == -7).all() and (hyper == -7).all()


def test_the_hallmark_pipelines_on_the_fixture(hip_ctx, pbmc, golden_dir):
    import scipy.sparse as sp

    import plaid_amd
    d, _ = pbmc
    X = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"]))
    Xn = plaid_amd.NamedMatrix(np.asfortranarray(X.toarray()), d["rownames"], d["colnames"])
    matG = plaid_amd.gmt2mat(plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt")))
    types, counts = np.unique(d["celltype"], return_counts=True)
    top = types[np.argsort(-counts)][:2]
    Y = np.full((50, 2), np.nan)
    Y[:, 0] = d["celltype"] == top[0]
    Y[d["celltype"] == top[0], 1], Y[d["celltype"] == top[1], 1] = 1.0, 0.0      # the rest take no part
    Yn = plaid_amd.NamedMatrix(Y, d["colnames"], [f"{top[0]}_vs_rest", f"{top[0]}_vs_{top[1]}"])
    cols = ["logFC", "AveExpr", "t", "P.Value", "adj.P.Val", "sigma2"]
    # the scores of the sets, tested
    S = plaid_amd.replaid_gsva_exact(Xn, matG, ctx=hip_ctx)
    tabs, hyper = plaid_amd.plaid_limma_contrasts(S, Yn, sort_by="P.Value", ctx=hip_ctx)
    assert list(tabs) == Yn.colnames == list(hyper)
    for nm, tab in tabs.items():
        assert tab.shape == (50, 6) and tab.colnames == cols and sorted(tab.rownames) == sorted(matG.colnames)
        assert np.isfinite(tab.values).all() and np.all(np.diff(tab.values[:, 3]) >= 0)
        assert set(hyper[nm]) == {"df.residual", "df.prior", "s2.prior", "n.ok"} and hyper[nm]["n.ok"] == 50
    assert hyper[Yn.colnames[0]]["df.residual"] == 48
    assert hyper[Yn.colnames[1]]["df.residual"] == int((~np.isnan(Y[:, 1])).sum()) - 2
    # the genes, tested; their logFC and P.Value go straight into plaid_sig and plaid_fisher
    gt, gh = plaid_amd.plaid_limma_contrasts(Xn, Yn, ctx=hip_ctx)
    g = gt[Yn.colnames[0]]
    assert g.shape == (X.shape[0], 6) and g.rownames == Xn.rownames
    fc = plaid_amd.NamedMatrix(np.column_stack([t.values[:, 0] for t in gt.values()]), Xn.rownames, list(gt))
    pv = plaid_amd.NamedMatrix(np.column_stack([t.values[:, 3] for t in gt.values()]), Xn.rownames, list(gt))
    sig = plaid_amd.plaid_sig(fc, pv, lfc=0.2, pcut=0.05)
    assert sig.shape == (X.shape[0], 2) and (sig.values != 0).any()
    res = plaid_amd.plaid_fisher(sig, matG, ctx=hip_ctx)
    assert list(res) == Yn.colnames
    for tab in res.values():
        assert tab.shape[1] == 12 and tab.shape[0] > 0 and tab.colnames[:3] == ["size", "ovUp", "ovDn"]
