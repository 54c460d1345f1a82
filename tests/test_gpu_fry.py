"""plaid.fry on the device (kernels_fry.hip, shard_limma.cpp: limma_worker with kFry, fry_tail) -- `pytest -m gpu`.

What is checked, and against what (DESIGN.md section 26 has the derivations and the host measurements):
  1. Z' of plaidhip_dev_fry_residuals is equal bit for bit to plaidhip_fry_residual_row (the same inline functions, on the
     host) on the device's own effects and on the divisors plaidhip_fry_divisors makes of the device's own RSS: rows 7 (odd,
     the 8-byte path) and 8 (the 16-byte path); n = 5, 131, 260 (the tail of the unroll, one and two column-block crossings);
     a `use` mask; p = 2 and 5; all three `standardize` values.  Shapes past these: p = 9 and 16, 17 and 32 (both ends of
     the 16- and 32-register instances) at n = 40 and 70, and rows 515 and 514 (a second workgroup of 512 rows), each on
     both load paths.
  2. The residual effects rho = Q2'z' at n_f = 131, p = 4 (d + 1 = 128: the cap, across a column block) against exact
     rationals on the device's own Z' within gamma_{128 + nblk} sum |q||z|: a block's chain of at most 128 fma carries
     gamma_128, the nblk block additions the rest.
  3. fry_gram_kernel bit for bit against fry_ref.gram_np: sets of 0, 1, 2, d, d + 1, d + 2 and 300 members, two identical
     genes, a gene outside the universe (zero rows), q = 1 and 3 at d = 9 and q = 2 at d = 127 (the widest staging array
     and the most entries per thread); tr M and |M|_F^2 likewise.
  4. fry_eigen_kernel: |lambda - exact| <= max(4 x EIG_DEV, D 2^-53) lambda_1 against the 50-digit spectrum of the matrix the
     device was given (EIG_DEV: numpy.linalg.eigvalsh's own worst deviation over the same matrices, host-measured); D = 2,
     3, 8, 33, 128 (the committed 50-digit pair), rank-deficient, a repeated top eigenvalue, a diagonal matrix; converged.
  5. End to end against fry_ref.fry_mp on the conditioned cases: 4 x fry_np's host-measured deviation; PValue held to the t
     tail's asserted accuracy at the device's own t and d; Direction; m = 1; a fit above the cap; BH restated.
  6. 1, 2 and 3 shards on the hook -- among them a case whose fits under the cap use samples on every side of columns 128
     and 256, so that rho is chained across shards that all hold data --, a failing shard, and plaid_fry_contrasts against
     the single calls: bit for bit."""
from fractions import Fraction

import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers import camera_ref as cr
from tests.helpers import exact_stats as xs
from tests.helpers import fry_ref as fr
from tests.helpers import limma_ref as lr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BOUND = {k: fr.FACTOR * v for k, v in fr.MEASURED.items()}

# rows, n, p, nfit (nfit = 2: the second fit leaves samples out)
RES_CASES = [(7, 5, 2, 1), (8, 5, 2, 1), (8, 131, 5, 2), (7, 260, 2, 2), (8, 260, 5, 1), (7, 131, 4, 1)]
# (appended only: test_residual_effects_against_exact_rationals takes RES_CASES[5]) the 16- and 32-register instances of the
# residual kernel at both ends (p = 9, 16, 17, 32), and a second workgroup of 512 rows holding three rows and two, each on
# both load paths
RES_CASES += [(8, 40, 9, 1), (7, 70, 16, 2), (8, 70, 17, 1), (7, 70, 32, 1), (515, 131, 5, 2), (514, 131, 2, 1)]
RES_IDS = ["x".join(str(v) for v in c) for c in RES_CASES]


def res_case(rows, n, p, nfit):
    rng = np.random.default_rng(100 * rows + n + p)
    X = cr.int_matrix(rows, n, rng)
    D = np.asfortranarray(np.stack([cr.make_design(n, p, rng) for _ in range(nfit)], axis=2))
    use = None
    if nfit > 1:
        use = np.ones((n, nfit), dtype=np.int8, order="F")
        use[rng.random(n) < 0.3, 1] = 0
        use[:p + 4, 1] = 1
        X[1, np.flatnonzero(use[:, 1] == 0)[0]] = np.nan      # a NaN where fit 1 does not look
    if n > 5:
        X[rows - 1, 0] = np.nan                                # a gene outside the universe of every fit
        X[2, :] = 3.0                                          # a constant gene: s2 = 0
    return X, D, use


def device_residuals(ctx, X, D, use, std):
    """E, rss, cg (host entry on the device's rss), Z' per fit, Q, nf -- and, for the last fit, rho with Q2"""
    import torch
    dev = torch.device("cuda", 0)
    rows, n = X.shape
    p, nfit = D.shape[1], D.shape[2]
    W = nfit * (p + 1)
    ld = rows + (rows & 1)
    Q = np.empty((n, p, nfit), order="F")
    nf = []
    for f in range(nfit):
        des = engine.limma_design(D[:, :, f], None if use is None else use[:, f], fit=f + 1)
        Q[:, :, f] = des["Q"]
        nf.append(des["nf"])
    nf = np.array(nf, dtype=np.int64)
    Ad = torch.full((n, ld), 777.0, dtype=torch.float64, device=dev)
    Ad[:, :rows] = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    Qd = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).to(dev)
    Ud = None if use is None else torch.from_numpy(np.ascontiguousarray(use.T)).to(dev)
    inv = torch.from_numpy(1.0 / nf.astype(np.float64)).to(dev)
    E = torch.full((W * rows,), -7.0, dtype=torch.float64, device=dev)
    R = torch.full((nfit * rows,), -7.0, dtype=torch.float64, device=dev)
    Zd = torch.full((n, ld), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    uptr = None if Ud is None else Ud.data_ptr()
    ctx.dev_row_design_effects(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, inv.data_ptr(), p, nfit, None, E.data_ptr())
    ctx.dev_row_design_rss(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, p, nfit, E.data_ptr(), None, R.data_ptr())
    ctx.synchronize()
    Eh, Rh = E.cpu().numpy().reshape(W, rows), R.cpu().numpy().reshape(nfit, rows)
    cg = engine.fry_divisors(Rh, nf, p, std)
    cgd = torch.from_numpy(cg).to(dev)
    Zs = []
    out = {"E": Eh, "rss": Rh, "cg": cg, "Q": Q, "nf": nf}
    for f in range(nfit):
        ctx.dev_fry_residuals(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, p, nfit, f, E.data_ptr(), cgd.data_ptr(),
                              Zd.data_ptr(), ld)
        ctx.synchronize()
        Zall = Zd.cpu().numpy()
        assert (Zall[:, rows:] == -7.0).all()                   # the padding of Z is not written
        Zs.append(np.ascontiguousarray(Zall[:, :rows].T))
    out["Z"] = Zs
    d = int(nf[-1] - p)
    if d + 1 <= engine.FRY_MIXED_MAX:
        uf = None if use is None else use[:, nfit - 1]
        Q2 = engine.fry_q2(D[:, :, nfit - 1], uf)
        Q2d = torch.from_numpy(np.ascontiguousarray(Q2.T)).to(dev)
        ud = None if uf is None else torch.from_numpy(np.ascontiguousarray(uf)).to(dev)
        rho = torch.full(((d + 1) * rows + 3,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.dev_fry_residual_effects(Zd.data_ptr(), ld, rows, n, Q2d.data_ptr(), None if ud is None else ud.data_ptr(), d, None,
                                     rho.data_ptr())
        ctx.synchronize()
        rh = rho.cpu().numpy()
        assert (rh[(d + 1) * rows:] == -7.0).all()
        out["rho"], out["Q2"] = rh[:d * rows].reshape(d, rows), Q2
    return out


@pytest.mark.parametrize("std", fr.STD)
@pytest.mark.parametrize("case", RES_CASES, ids=RES_IDS)
def test_z_is_the_host_entry_bit_for_bit(hip_ctx, case, std):
    X, D, use = res_case(*case)
    rows, n, p, nfit = case
    dv = device_residuals(hip_ctx, X, D, use, std)
    for f in range(nfit):
        uf = None if use is None else use[:, f]
        want = np.stack([engine.fry_residual_row(X[r], dv["Q"][:, :, f], uf, dv["E"][f * (p + 1):f * (p + 1) + p, r],
                                                 dv["cg"][f, r]) for r in range(rows)])
        got = dv["Z"][f]
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (f, np.argwhere(got != want)[:5])
        out = np.isnan(dv["cg"][f])
        assert (got[out] == 0.0).all() and not np.signbit(got[out]).any() and np.isfinite(got).all()
        if uf is not None:
            assert (got[:, uf == 0] == 0.0).all()
        if n > 5:
            assert out[rows - 1]                                             # the NaN gene
            zero = dv["rss"][f, 2] == 0.0                                    # the constant gene: s2 = 0 where no rounding
            assert out[2] == (std == "residual.sd" and zero)                 # a zero divisor leaves, the others keep it
        # the divisor is what the header says of the device's own RSS
        s2 = dv["rss"][f] / float(dv["nf"][f] - p)
        if std == "residual.sd":
            keep = ~out
            assert np.array_equal(dv["cg"][f][keep], np.sqrt(s2[keep]))
        if std == "none":
            assert (dv["cg"][f][~out] == 1.0).all()


def test_residual_effects_against_exact_rationals(hip_ctx):
    case = RES_CASES[5]                                        # n_f = 131, p = 4: d + 1 = 128
    X, D, use = res_case(*case)
    rows, n, p, nfit = case
    dv = device_residuals(hip_ctx, X, D, use, "posterior.sd")
    Z, Q2, rho = dv["Z"][0], dv["Q2"], dv["rho"]
    d = n - p
    assert d + 1 == engine.FRY_MIXED_MAX and rho.shape == (d, rows)
    nblk = (n + 127) // 128
    k = 128 + nblk
    gam = k * U / (1 - k * U)
    worst = 0.0
    for r in range(rows):
        zf = [Fraction(float(v)) for v in Z[r]]
        for c in range(d):
            exact = sum((z * Fraction(float(w)) for z, w in zip(zf, Q2[:, c])), Fraction(0))
            mag = float(np.abs(Z[r]) @ np.abs(Q2[:, c]))
            err = abs(float(Fraction(float(rho[c, r])) - exact))
            assert err <= gam * mag, (r, c, err, gam * mag)
            worst = max(worst, err / (gam * mag) if mag > 0 else 0.0)
    assert (rho[:, rows - 1] == 0.0).all()                    # the gene outside the universe
    print(f"[measure] residual effects: worst error / bound {worst:.3g}")


# ---- Gram --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,d", [(1, 9), (3, 9), (2, 127)], ids=["q1-d9", "q3-d9", "q2-d127"])
def test_gram_is_the_numpy_order_bit_for_bit(hip_ctx, q, d):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17 + q + d)
    rows = 400
    rho = rng.normal(size=(rows, d))
    e = rng.normal(size=(rows, q))
    rho[11] = rho[10]                                          # two identical genes
    e[11] = e[10]
    rho[20], e[20] = 0.0, 0.0                                  # a gene outside the universe (a NaN in a used sample)
    sets = cr.make_sets(rows, (0, 1, 2, d, d + 1, d + 2, 300), rng) + [[10, 11, 5], [20, 3, 4, 7]]
    sets = [list(rng.permutation(s)) for s in sets]            # (the order is the set's own: not sorted)
    Gp, Gi = cr.pattern(sets)
    m = len(sets)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rd, ed, gp, gi = t(rho), t(e), t(Gp), t(Gi if len(Gi) else np.zeros(1, np.int32))
    Cd = torch.full((m * d * d + 2,), -7.0, dtype=torch.float64, device=dev)
    bd = torch.full((m * q * d + 2,), -7.0, dtype=torch.float64, device=dev)
    ad, trd, frd = (torch.full((m * q + 2,), -7.0, dtype=torch.float64, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    hip_ctx.dev_fry_gram(rd.data_ptr(), ed.data_ptr(), rows, d, q, gp.data_ptr(), gi.data_ptr(), m, Cd.data_ptr(), bd.data_ptr(),
                         ad.data_ptr(), trd.data_ptr(), frd.data_ptr())
    hip_ctx.synchronize()
    C, b, a, tr, fro = (v.cpu().numpy() for v in (Cd, bd, ad, trd, frd))
    for v, k in ((C, m * d * d), (b, m * q * d), (a, m * q), (tr, m * q), (fro, m * q)):
        assert (v[k:] == -7.0).all()
    want = fr.gram_np(rho, e, sets)
    same = lambda x, y: np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64))
    for s, w in enumerate(want):
        assert same(C[s * d * d:(s + 1) * d * d].reshape(d, d), w["C"]), s
        assert same(b[s * q * d:(s + 1) * q * d].reshape(q, d), w["b"]), s
        assert same(a[s * q:(s + 1) * q], w["a"]) and same(tr[s * q:(s + 1) * q], w["tr"]), s
        assert same(fro[s * q:(s + 1) * q], w["fro"]), s
    assert (C[:d * d] == 0.0).all() and tr[0] == 0.0                        # the empty set


# ---- eigen -----------------------------------------------------------------------------------------------------------------------
def device_eigen(ctx, M, Dn):
    import torch
    dev = torch.device("cuda", 0)
    dim = M.shape[0]
    Md = torch.from_numpy(np.ascontiguousarray(M)).to(dev)
    Dk = torch.tensor([Dn], dtype=torch.int32, device=dev)
    l1, lD = (torch.full((2,), -7.0, dtype=torch.float64, device=dev) for _ in range(2))
    sw, cv = (torch.full((2,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    ctx.dev_fry_eigen(Md.data_ptr(), dim, 1, Dk.data_ptr(), l1.data_ptr(), lD.data_ptr(), sw.data_ptr(), cv.data_ptr())
    ctx.synchronize()
    assert l1[1].item() == -7.0 and lD[1].item() == -7.0 and sw[1].item() == -7
    return l1[0].item(), lD[0].item(), sw[0].item(), cv[0].item()


@pytest.mark.parametrize("name", sorted(fr.eigen_cases()))
def test_eigenvalues_hold_the_certificate(hip_ctx, name):
    import mpmath as mp
    M, Dn = fr.eigen_cases()[name]
    l1, lD, sweeps, conv = device_eigen(hip_ctx, M, Dn)
    e1, eD = fr.eigen_exact(name)
    a = fr.eig_allowance(Dn)
    with mp.workdps(fr.DPS + 20):
        dev1, devD = float(abs(mp.mpf(l1) - e1) / e1), float(abs(mp.mpf(lD) - eD) / e1)
    print(f"[measure] eigen {name}: lambda_1 {dev1:.3g}, lambda_D {devD:.3g} (allowed {a:.3g}), {sweeps} sweeps")
    assert conv == 1 and 0 <= sweeps <= 30
    assert dev1 <= a and devD <= a, (name, dev1, devD, a)
    if name == "rank5of12":
        assert lD > 1e-3 * l1                                  # the fifth eigenvalue, not the noise about 0 past it


def test_eigenvalues_at_the_cap(hip_ctx):
    import mpmath as mp
    gold = np.load("tests/golden/fry_eig128.npz")
    assert int(gold["seed"]) == fr.EIG128_SEED
    M = fr.eig128_matrix()
    l1, lD, sweeps, conv = device_eigen(hip_ctx, M, 128)
    a = fr.eig_allowance(128)
    with mp.workdps(fr.DPS + 20):
        e1, eD = mp.mpf(str(gold["lam1"][0])), mp.mpf(str(gold["lam128"][0]))
        dev1, devD = float(abs(mp.mpf(l1) - e1) / e1), float(abs(mp.mpf(lD) - eD) / e1)
    print(f"[measure] eigen D128: lambda_1 {dev1:.3g}, lambda_128 {devD:.3g} (allowed {a:.3g}), {sweeps} sweeps")
    assert conv == 1
    assert dev1 <= a and devD <= a, (dev1, devD, a)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("std", fr.STD)
@pytest.mark.parametrize("name", fr.E2E_CASES)
def test_end_to_end_against_the_words_at_50_digits(hip_ctx, name, std):
    """fry_np against fry_mp over these cases, measured on the host: t 1.22e-13, PValue 9.27e-15, PValue.Mixed 1.47e-14;
    asserted: 4 x that"""
    X, D, use, K, sets = fr.e2e_case(name)
    Gp, Gi = cr.pattern(sets)
    out, hyper = hip_ctx.fry(X, D, Gp, Gi, use, K, std)
    ref = fr.e2e_reference(name, std)
    worst = {k: 0.0 for k in BOUND}
    acc = xs.ASSERTED_ACC["pt"]
    for f, fit in enumerate(ref):
        d = fit["d"]
        assert hyper[f, 0] == d and hyper[f, 5] == d + 1 and hyper[f, 6] == 1.0
        assert hyper[f, 4] == fit["inuni"].sum()
        for j, rows in enumerate(fit["tables"]):
            got = out[:, :, j, f]
            want = fr.table_float(rows)
            keep = np.array([fr.conditioned(r) for r in rows])
            dev = fr.deviation(got[:, [0, 2, 3, 5]], want, keep)
            for k in worst:
                worst[k] = max(worst[k], dev[k])
            for s in range(len(sets)):
                if np.isnan(got[s, 2]):
                    assert got[s, 0] == 0 and np.isnan(got[s, 1:]).all()
                    continue
                assert got[s, 1] == (-1.0 if got[s, 2] < 0 else 1.0)
                pt = float(xs.two_pt(got[s, 2], d))
                assert abs(got[s, 3] - pt) <= acc * pt, (f, j, s)
                if got[s, 0] == 1:
                    assert got[s, 5] == got[s, 3]
            assert np.allclose(got[:, 4], lr.bh(got[:, 3]), rtol=4 * U, atol=0, equal_nan=True)
            assert np.allclose(got[:, 6], lr.bh(got[:, 5]), rtol=4 * U, atol=0, equal_nan=True)
    print(f"[measure] end to end {name} {std}: " + ", ".join(f"{k} {v:.3g} (bound {BOUND[k]:.3g})" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= BOUND[k], (k, v, BOUND[k])


def cap_case():
    """140 samples, p = 2: d + 1 = 139 effects, above the cap; a second fit of 60 samples under it"""
    rng = np.random.default_rng(8)
    g, n = 60, 140
    X = cr.int_matrix(g, n, rng)
    D = np.asfortranarray(np.stack([cr.make_design(n, 2, rng) for _ in range(2)], axis=2))
    use = np.ones((n, 2), dtype=np.int8, order="F")
    use[60:, 1] = 0
    sets = cr.make_sets(g, (0, 1, 2, 7, 30, g), rng)
    return X, D, use, sets


def test_a_fit_above_the_cap_has_no_mixed_test_and_says_so(hip_ctx):
    X, D, use, sets = cap_case()
    Gp, Gi = cr.pattern(sets)
    out, hyper = hip_ctx.fry(X, D, Gp, Gi, use, np.array([0.0, 1.0]))
    assert hyper[0, 5] == 139 and hyper[0, 6] == 0.0 and hyper[1, 5] == 59 and hyper[1, 6] == 1.0
    assert np.isnan(out[:, 5:7, 0, 0]).all()
    assert not np.isnan(out[1:, 0:5, 0, 0]).any() and not np.isnan(out[1:, :, 0, 1]).any()
    acc = xs.ASSERTED_ACC["pt"]
    for s in range(1, len(sets)):
        pt = float(xs.two_pt(out[s, 2, 0, 0], 138))
        assert abs(out[s, 3, 0, 0] - pt) <= acc * pt
    ref = fr.fry_np(X, D[:, :, 0], None, np.array([0.0, 1.0]), sets)
    assert np.allclose(out[1:, 2, 0, 0], ref[1:, 1, 0], rtol=1e-9, atol=0)      # (a sanity check of the large-n path, not a bound)


# ---- sharding ---------------------------------------------------------------------------------------------------------------------
def spread_case():
    """260 samples (two column blocks and a tail), two fits under the cap whose used samples lie on every side of columns
    128 and 256: 100 and 70 samples spread over all columns, p = 2, two contrasts -- so that with 2 and 3 shards every
    shard holds rows of Q2 and of Z' that count, and rho is chained across them"""
    rng = np.random.default_rng(21)
    g, n = 50, 260
    X = cr.int_matrix(g, n, rng)
    D = np.asfortranarray(np.stack([cr.make_design(n, 2, rng) for _ in range(2)], axis=2))
    use = np.zeros((n, 2), dtype=np.int8, order="F")
    use[np.sort(rng.choice(n, size=100, replace=False)), 0] = 1
    use[np.sort(rng.choice(n, size=70, replace=False)), 1] = 1
    for f in range(2):
        for lo, hi in ((0, 128), (128, 256), (256, 260)):
            assert use[lo:hi, f].sum() >= 1, "every column block holds used samples of every fit"
    X[7, np.flatnonzero(use[:, 0] == 0)[0]] = np.nan          # a NaN where fit 0 does not look
    sets = cr.make_sets(g, (0, 1, 2, 7, 25, g), rng)
    K = np.array([[0.0, 1.0], [1.0, -0.5]])
    return X, D, use, K, sets


@pytest.mark.parametrize("which", ["small", "cap", "spread"])
def test_every_sharding_has_the_one_device_bits(hip_ctx, which):
    if which == "small":
        X, D, use, K, sets = fr.e2e_case("small")
    elif which == "spread":
        X, D, use, K, sets = spread_case()
    else:
        X, D, use, sets = cap_case()
        K = np.array([0.0, 1.0])
    Gp, Gi = cr.pattern(sets)
    out, hyper = hip_ctx.fry(X, D, Gp, Gi, use, K)
    if which == "spread":
        assert (hyper[:, 6] == 1.0).all() and list(hyper[:, 5]) == [99.0, 69.0]
        assert not np.isnan(out[1:, :, :, :]).any()             # every set with members has its mixed columns
        ref = [fr.fry_np(X, D[:, :, f], use[:, f], K, sets) for f in range(2)]
        for f in range(2):                                      # (a sanity check that the chained rho is the right one, not a bound)
            assert np.allclose(out[1:, 5, :, f], ref[f][1:, 3, :], rtol=1e-8, atol=0)
    for nshards in (1, 2, 3):
        status, o2, h2 = fr.run_sharded(nshards, X, D, Gp, Gi, use, K)
        assert status == _lib.OK
        assert np.array_equal(o2.view(np.int64), out.view(np.int64)), nshards
        assert np.array_equal(h2.view(np.int64), hyper.view(np.int64)), nshards


def test_a_failing_shard_reports_and_writes_nothing(hip_ctx):
    X, D, use, sets = cap_case()
    Gp, Gi = cr.pattern(sets)
    status, out, hyper = fr.run_sharded(3, X, D, Gp, Gi, use, np.array([0.0, 1.0]), fail=1)
    assert status == _lib.EHIP
    assert "injected failure" in _lib.load().plaidhip_last_error_string().decode()
    assert (out == -7.0).all() and (hyper == -7.0).all()


def test_contrasts_column_is_the_single_call_bit_for_bit(hip_ctx):
    rng = np.random.default_rng(78)
    g, n = 120, 40
    genes = [f"g{i}" for i in range(g)]
    X = plaid_amd.NamedMatrix(cr.int_matrix(g, n, rng), genes, [f"s{i}" for i in range(n)])
    Y = np.column_stack([rng.permutation(np.arange(n) % 2).astype(np.float64) for _ in range(3)])
    Y[rng.choice(n, size=6, replace=False), 1] = np.nan
    Y[rng.choice(n, size=9, replace=False), 2] = np.nan
    Yn = plaid_amd.NamedMatrix(Y, X.colnames, ["a", "b", "c"])
    B = rng.normal(size=(n, 1))
    G = {f"set{k}": [genes[i] for i in rng.choice(g, size=sz, replace=False)] for k, sz in enumerate((1, 2, 7, 30, 64, 65))}
    tabs, hyp = plaid_amd.plaid_fry_contrasts(X, Yn, G, B=B, sort_by="none", ctx=hip_ctx)
    by_mixed, _ = plaid_amd.plaid_fry_contrasts(X, Yn, G, B=B, sort_by="mixed", ctx=hip_ctx)
    for j, nm in enumerate(["a", "b", "c"]):
        Dj, uj = lr.contrast_design(Y, B, j)
        one, h1 = plaid_amd.plaid_fry(X, Dj, G, contrasts=np.array([0.0, 1.0, 0.0]), use=uj, sort_by="none", ctx=hip_ctx)
        assert tabs[nm].rownames == one["1"].rownames and tabs[nm].colnames == list(engine.FRY_COLUMNS)
        assert np.array_equal(tabs[nm].values.view(np.int64), one["1"].values.view(np.int64)), nm
        assert hyp[nm] == h1 and h1["mixed"] == 1.0
        assert (np.diff(by_mixed[nm].values[:, 5]) >= 0).all()
