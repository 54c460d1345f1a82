"""The pair crossprod's flex steps (`pytest -m gpu`, through the C ABI).

A register-partial pair plan (more than 10,224 genes, at most 6,144 sets) is planned with FLEX STEPS (geneset.cpp,
plan_tile_flex): step 7 of every index chunk adds into an accumulator pair of its own, and in a HOST lane -- one whose
list in the slice is short -- those cells gather the overflow of one long lane (the OWNER) of the same tile, which pulls
the sum across the wavefront at the tile end.  Every case holds the kernel to the C oracle at the tolerance of
test_gpu_pair_regpartials.py (oracle/fullsize.py RTOL / ATOL) and to the pinned scratch form
(PLAIDHIP_OPT_SPMM_DENSE_KERNEL = 4), which walks the same plan, bit for bit, flag words included.

Shape: 10,400 genes (two slices of 5,200), 130 sets (two full tiles and one of two lanes), 5 sample columns (the last pair
has no column B).  The sets are disjoint, so a gene belongs to one set only and a NaN in a gene that a host lane reads
for its owner may show in the owner's score alone.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G2 = 10400     # two slices of 5,200 genes
M = 130
N = 5


def _tol():
    from oracle.fullsize import ATOL, RTOL
    return RTOL, ATOL


def _probe(g, Gp, Gi, flex=1):
    """plaidhip_debug_pair_flex_probe: (padded slots per pair, double-booked reads, pairs[k] = (slice, owner set, host
    set or -1, a gene the host lane reads for the owner)); the plan's self-check must be clean"""
    from plaid_amd import _lib
    fn = _lib.load().plaidhip_debug_pair_flex_probe
    fn.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_void_p,
                   C.c_int64]
    fn.restype = C.c_int
    out = (C.c_int64 * 16)()
    cap = 64 * 96 * 3
    pairs = np.full((cap, 4), -9, dtype=np.int32)
    Gp = np.ascontiguousarray(Gp, dtype=np.int32)
    Gi = np.ascontiguousarray(Gi, dtype=np.int32)
    assert fn(g, len(Gp) - 1, Gp.ctypes.data, Gi.ctypes.data, 16, flex, out, pairs.ctypes.data, cap) == 0
    assert out[2] == int(Gp[-1]) and out[4] == 0 and out[10] == 0 and out[5] == 1
    return int(out[8]), int(out[3]), pairs[:out[9]].copy()


def _split_sets(g, shares, sizes, nsl=2, seed=3):
    """disjoint sets: set j has round(share * size) of its genes in the first slice and the rest in the last one (a
    middle slice, if there is one, gets a fixed 5 genes more), drawn without replacement"""
    rng = np.random.default_rng(seed)
    width = (g + nsl - 1) // nsl
    width += width & 1
    pools = [list(rng.permutation(np.arange(s * width, min(g, (s + 1) * width)))) for s in range(nsl)]
    Gi, Gp = [], [0]
    for share, k in zip(shares, sizes):
        a = int(round(share * k))
        take = [(0, a), (nsl - 1, k - a)] + [(s, 5) for s in range(1, nsl - 1)]
        genes = []
        for s, cnt in take:
            genes += [pools[s].pop() for _ in range(cnt)]
        Gi.append(np.sort(np.array(genes, dtype=np.int32)))
        Gp.append(Gp[-1] + len(genes))
    return np.array(Gp, dtype=np.int32), np.concatenate(Gi).astype(np.int32)


def _x(g, n, seed=1):
    return np.asfortranarray(np.random.default_rng(seed).normal(8.0, 2.0, size=(g, n)))


def _both_forms(pin, g, Gp, Gi, X, stat="mean", ldx=None, lds=None, csc=False):
    """scores (m x n) and flag words of the default form and of the pinned scratch form, on one geneset"""
    import torch
    dev = torch.device("cuda", 0)
    n = X.shape[1]
    m = len(Gp) - 1
    ldx = g if ldx is None else ldx
    lds = m if lds is None else lds
    res = []
    ctx = pin()
    gs = ctx.geneset(g, Gp, Gi)
    try:
        if csc:
            import scipy.sparse as sp
            Xs = sp.csc_matrix(X)
            dXp = torch.from_numpy(Xs.indptr.astype(np.int32)).to(dev)
            dXi = torch.from_numpy(Xs.indices.astype(np.int32)).to(dev)
            dXx = torch.from_numpy(Xs.data.astype(np.float64)).to(dev)
        else:
            Xh = np.full((n, ldx), -77.0)          # rows of this array are the columns of X, ldx apart
            Xh[:, :g] = X.T
            dX = torch.from_numpy(Xh).to(dev)
        for mode in ("auto", "pair_scratch"):
            ctx = pin(spmm_dense_kernel=mode, spmm_sparse_kernel="gather")
            S = torch.full((n, lds), -55.0, dtype=torch.float64, device=dev)
            flags = torch.zeros(4, dtype=torch.int32, device=dev)
            if csc:
                ctx.dev_spmm_csc(gs, dXp.data_ptr(), dXi.data_ptr(), dXx.data_ptr(), n, S.data_ptr(), lds, stat, 1.0, 0.0,
                                 flags.data_ptr(), nnz=int(Xs.nnz))
            else:
                ctx.dev_spmm_dense(gs, dX.data_ptr(), ldx, n, S.data_ptr(), lds, stat, 1.0, 0.0, flags.data_ptr())
            torch.cuda.synchronize()
            Sh = S.cpu().numpy()
            assert np.all(Sh[:, m:] == -55.0)      # nothing written between the columns of S
            res.append((np.ascontiguousarray(Sh[:, :m].T), flags.cpu().numpy()[:3].copy()))
    finally:
        gs.close()
    return res


def _check(pin, g, Gp, Gi, X, stat="mean", **kw):
    from oracle import c_oracle
    (Sa, fa), (Sb, fb) = _both_forms(pin, g, Gp, Gi, X, stat=stat, **kw)
    assert np.array_equal(Sa.view(np.int64), Sb.view(np.int64)), "register-partial and scratch forms differ in bits"
    assert np.array_equal(fa, fb)
    rtol, atol = _tol()
    ref = c_oracle.crossprod_dense(X, Gp, Gi, stat, threads=8)
    np.testing.assert_allclose(Sa, ref, rtol=rtol, atol=atol, equal_nan=True)
    return Sa, fa


def _sets_70_30(g=G2, m=M, nsl=2):
    """60 genes per set, 42 / 18 and 18 / 42 in the first / last slice in turn: in either slice half the lanes of a tile
    are long and half can host.  Sets 128 and 129 sit alone in the third tile, whose other 62 lanes have no set."""
    return _split_sets(g, [0.7 if j % 2 == 0 else 0.3 for j in range(m)], [60] * m, nsl=nsl)


@pytest.fixture(scope="module")
def c7030():
    Gp, Gi = _sets_70_30()
    slots, booked, pairs = _probe(G2, Gp, Gi)
    return Gp, Gi, slots, booked, pairs


def test_hosts_in_both_slices_and_a_host_without_a_set(pinned_ctx, c7030):
    Gp, Gi, slots, _, pairs = c7030
    for s in (0, 1):
        assert np.sum(pairs[:, 0] == s) >= 8
    assert np.any(pairs[:, 2] < 0), "no owner is hosted by a lane without a set (the third tile's empty lanes)"
    assert np.all(pairs[:, 3] >= 0)
    slots0, _, none = _probe(G2, Gp, Gi, flex=0)
    assert len(none) == 0 and slots < slots0
    _check(pinned_ctx, G2, Gp, Gi, _x(G2, N))


def test_no_long_lane_anywhere_plans_as_without_flex_steps(pinned_ctx):
    """30 / 30: every lane of a tile is as long as the next, nobody can host; the two sets of the third tile have 4 / 4
    genes, one chunk either way"""
    Gp, Gi = _split_sets(G2, [0.5] * M, [60] * 128 + [8, 8])
    slots, booked, pairs = _probe(G2, Gp, Gi)
    slots0, booked0, _ = _probe(G2, Gp, Gi, flex=0)
    assert len(pairs) == 0 and slots == slots0 and booked == booked0
    _check(pinned_ctx, G2, Gp, Gi, _x(G2, N))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_guest_value_stays_out_of_the_host_score(pinned_ctx, c7030, bad):
    """NaN / +Inf in one gene that a host lane reads for its owner, for eight owners (four per slice): exactly the owner's
    score of that column is NaN / Inf, every other score -- the host's among them -- has the bits of the clean run"""
    Gp, Gi, _, _, pairs = c7030
    pick, owners, hosts = [], set(), set()
    for s in (0, 1):           # (a set that hosts in one slice is an owner in the other: no picked host may be a picked owner)
        for row in pairs[pairs[:, 0] == s]:
            if sum(1 for r in pick if r[0] == s) < 4 and int(row[1]) not in hosts and int(row[2]) not in owners:
                pick.append(row)
                owners.add(int(row[1]))
                hosts.add(int(row[2]))
    pick = np.array(pick)
    assert len(pick) == 8
    X = _x(G2, N)
    clean, _ = _check(pinned_ctx, G2, Gp, Gi, X)
    Xb = X.copy()
    col = 3
    for _, owner, host, gene in pick:
        assert gene in Gi[Gp[owner]:Gp[owner + 1]] and np.sum(Gi == gene) == 1     # the owner's, and of this set only
        Xb[gene, col] = bad
    S, f = _check(pinned_ctx, G2, Gp, Gi, Xb)
    hit = np.zeros(S.shape, dtype=bool)
    hit[pick[:, 1], col] = True
    assert np.all(np.isnan(S[hit]) if np.isnan(bad) else np.isposinf(S[hit]))
    assert np.array_equal(S[~hit].view(np.int64), clean[~hit].view(np.int64))
    hosts = pick[:, 2][pick[:, 2] >= 0]
    assert np.all(np.isfinite(S[hosts, col]))
    assert f[2] == (1 if np.isnan(bad) else 0)


def test_nan_zero_column_and_negatives_with_flags(pinned_ctx, c7030):
    Gp, Gi = c7030[0], c7030[1]
    X = _x(G2, N) - 8.0         # negative values
    X[:, 2] = 0.0               # a zero column: exact zero scores
    X[Gi[Gp[7]], 3] = np.nan    # one NaN, member of set 7
    S, f = _check(pinned_ctx, G2, Gp, Gi, X)
    assert list(f) == [1, 1, 1]                       # has_neg, has_zero, has_nan
    assert np.isnan(S[7, 3]) and np.sum(np.isnan(S)) == 1 and np.all(S[:, 2] == 0.0)


def test_stat_sum(pinned_ctx, c7030):
    _check(pinned_ctx, G2, c7030[0], c7030[1], _x(G2, N), stat="sum")


def test_leading_dimensions(pinned_ctx, c7030):
    """S with a leading dimension above m, X with an odd one above g (every other column 8 bytes off 16-byte alignment)"""
    _check(pinned_ctx, G2, c7030[0], c7030[1], _x(G2, N), ldx=G2 + 7, lds=M + 5)


def test_csc_x_through_the_pair_kernel(pinned_ctx, c7030):
    X = _x(G2, N)
    X[np.random.default_rng(4).random(X.shape) < 0.6] = 0.0
    _check(pinned_ctx, G2, c7030[0], c7030[1], X, csc=True)


def test_three_slices(pinned_ctx):
    g = 20600
    Gp, Gi = _sets_70_30(g=g, nsl=3)
    _, _, pairs = _probe(g, Gp, Gi)
    assert np.sum(pairs[:, 0] == 0) >= 8 and np.sum(pairs[:, 0] == 2) >= 8
    _check(pinned_ctx, g, Gp, Gi, _x(g, N))


def test_rank_input_has_the_bits_of_the_rank_route(pinned_ctx, c7030):
    """power-1 ranks: every sum is an integer below 2^53, exact in any order -- dev_spmm_ranks (u16 staging) and
    dev_spmm_dense (the flex form) agree in every bit"""
    import torch
    Gp, Gi = c7030[0], c7030[1]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    R = np.stack([rng.permutation(G2) + 1.0 for _ in range(N)])      # rows = columns of the rank matrix
    dR = torch.from_numpy(R).to(dev)
    ctx = pinned_ctx()
    gs = ctx.geneset(G2, Gp, Gi)
    try:
        out = []
        for fn in (ctx.dev_spmm_ranks, ctx.dev_spmm_dense):
            S = torch.zeros((N, M), dtype=torch.float64, device=dev)
            fn(gs, dR.data_ptr(), G2, N, S.data_ptr(), M, "mean", 1.0, 0.0, None)
            torch.cuda.synchronize()
            out.append(S.cpu().numpy())
    finally:
        gs.close()
    assert np.array_equal(out[0].view(np.int64), out[1].view(np.int64))
    exact = np.stack([[R[c, Gi[Gp[j]:Gp[j + 1]]].sum() / (1e-8 + (Gp[j + 1] - Gp[j])) for j in range(M)] for c in range(N)])
    np.testing.assert_allclose(out[1], exact, rtol=1e-14, atol=0)     # (the sum is exact; two roundings in the weight)
