"""The pair crossprod's tile ends and staging stores (`pytest -m gpu`, through the C ABI).

A tile end of the register-partial form keeps the tile's partial sums in ONE register vector indexed by the tile's ordinal
within its wavefront (put and get are register-indexed moves), and the staging of a slice writes a lane's two LDS
entries in an order that depends on the lane (kernels_spmm.hip, PLAIDHIP_RSLOT_PUT / _GET and PLAIDHIP_ST_ONE).  Neither
changes a sum or its order, so every case here is held to EXACT results: X holds integers (permuted ranks) and the
statistic is "sum", so every score is an integer below 2^53 that numpy computes without rounding, and the kernel's score
must equal it.  The pinned scratch form (`spmm_dense_kernel = "pair_scratch"`) shares the tile end and the staging, so it
must agree bit for bit, flag words included -- but only the exact reference catches an error common to both.

Shapes are the smallest that reach each path: 10,400 genes = two slices of 5,200, 20,600 = three; 1,536 sets = 24 tiles
(two per wavefront of the 768-thread form), 6,144 sets = 96 tiles (eight per wavefront: every slot).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G2 = 10400     # two slices of 5,200 genes
G3 = 20600     # three slices


def _probe(g, Gp, Gi):
    """plaidhip_debug_pair_flex_probe: its sixteen words (the plan's self-check must be clean and the plan must be a
    register-partial one) and the owner <-> host pairs"""
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
    assert fn(g, len(Gp) - 1, Gp.ctypes.data, Gi.ctypes.data, 16, 1, out, pairs.ctypes.data, cap) == 0
    assert out[2] == int(Gp[-1]) and out[4] == 0 and out[10] == 0 and out[5] == 1
    return [int(v) for v in out], pairs[:out[9]].copy()


def _sets_by_slice(g, m, counts, nsl, seed=3):
    """m sets; set j draws counts(j)[s] distinct genes from slice s (sets may share genes)"""
    rng = np.random.default_rng(seed)
    width = (g + nsl - 1) // nsl
    width += width & 1
    Gi, Gp = [], [0]
    for j in range(m):
        genes = [s * width + rng.choice(min(g, (s + 1) * width) - s * width, size=c, replace=False) for s, c in enumerate(counts(j))]
        Gi.append(np.sort(np.concatenate(genes)).astype(np.int32))
        Gp.append(Gp[-1] + len(Gi[-1]))
    return np.array(Gp, dtype=np.int32), np.concatenate(Gi).astype(np.int32)


def _sets_70_30(g, m, nsl):
    """the 70 / 30 collection of test_gpu_pair_flex.py for any number of sets: 60 genes, 42 / 18 and 18 / 42 in the first /
    last slice in turn (5 more in a middle slice): in either slice half the lanes of a tile are long and half can host"""
    def counts(j):
        a = 42 if j % 2 == 0 else 18
        return [a] + [5] * (nsl - 2) + [60 - a]
    return _sets_by_slice(g, m, counts, nsl)


def _ranks(g, n, seed=1):
    """n columns of permuted ranks 1..g (integers: every sum of them is exact)"""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.stack([rng.permutation(g) + 1.0 for _ in range(n)], axis=1))


def _exact_sums(Gp, Gi, X):
    return np.add.reduceat(X[Gi], Gp[:-1].astype(np.int64), axis=0)      # (no empty set anywhere in this file)


def _check_exact(pin, g, Gp, Gi, X, ldx=None):
    """stat "sum" by the default form and by the pinned scratch form: equal bits and flag words, and equal to numpy's sums"""
    import torch
    dev = torch.device("cuda", 0)
    n, m = X.shape[1], len(Gp) - 1
    ldx = g if ldx is None else ldx
    Xh = np.full((n, ldx), -77.0)          # rows of this array are the columns of X, ldx apart
    Xh[:, :g] = X.T
    dX = torch.from_numpy(Xh).to(dev)
    res = []
    ctx = pin()
    gs = ctx.geneset(g, Gp, Gi)
    try:
        for mode in ("auto", "pair_scratch"):
            ctx = pin(spmm_dense_kernel=mode)
            S = torch.full((n, m), -55.0, dtype=torch.float64, device=dev)
            flags = torch.zeros(4, dtype=torch.int32, device=dev)
            ctx.dev_spmm_dense(gs, dX.data_ptr(), ldx, n, S.data_ptr(), m, "sum", 1.0, 0.0, flags.data_ptr())
            torch.cuda.synchronize()
            res.append((np.ascontiguousarray(S.cpu().numpy().T), flags.cpu().numpy()[:3].copy()))
    finally:
        gs.close()
    (Sa, fa), (Sb, fb) = res
    ref = _exact_sums(Gp, Gi, X)
    assert np.all(ref < 2.0 ** 53)
    bad = np.argwhere(Sa != ref)
    assert len(bad) == 0, f"{len(bad)} scores differ from the exact sums, first (set, column) {bad[0]}: {Sa[tuple(bad[0])]} != {ref[tuple(bad[0])]}"
    assert np.array_equal(Sa.view(np.int64), Sb.view(np.int64)), "default and scratch forms differ in bits"
    assert np.array_equal(fa, fb) and list(fa) == [0, 0, 0]
    return Sa


def test_back_to_back_one_chunk_tiles(pinned_ctx):
    """1,536 sets of 3 + 3 genes: 24 tiles of one chunk per slice, so a wavefront with two tiles ends one in each of two
    consecutive steps; 5 columns: the last pair has no column B"""
    Gp, Gi = _sets_by_slice(G2, 1536, lambda j: [3, 3], 2)
    out, _ = _probe(G2, Gp, Gi)
    assert out[0] == 2 and out[1] == 2 * 24, "not one chunk per tile and slice"
    assert out[6] >= 2, "no wavefront with two tiles"
    _check_exact(pinned_ctx, G2, Gp, Gi, _ranks(G2, 5))


def test_owners_at_consecutive_tile_ends(pinned_ctx):
    """70 / 30 at 1,536 sets: a wavefront whose every tile has an owner in either slice pulls at consecutive tile ends and
    at its last tile end of a slice"""
    Gp, Gi = _sets_70_30(G2, 1536, 2)
    out, pairs = _probe(G2, Gp, Gi)
    for s in (0, 1):
        assert np.sum(pairs[:, 0] == s) >= 24
    assert out[13] >= 1, "no wavefront with owners on all of its (two or more) tiles in both slices"
    _check_exact(pinned_ctx, G2, Gp, Gi, _ranks(G2, 5))


def test_all_eight_slots_three_slices(pinned_ctx):
    """6,144 sets = 96 tiles, eight on every wavefront; three slices: the middle one gets AND puts every slot at its tile
    ends"""
    Gp, Gi = _sets_70_30(G3, 6144, 3)
    out, pairs = _probe(G3, Gp, Gi)
    assert out[0] == 3 and out[6] == 8 and out[7] == 12
    assert np.sum(pairs[:, 0] == 0) >= 8 and np.sum(pairs[:, 0] == 2) >= 8
    _check_exact(pinned_ctx, G3, Gp, Gi, _ranks(G3, 3))


def test_second_pair_of_a_workgroup(pinned_ctx):
    """2 x (compute units) + 3 columns: more pairs than workgroups, so a workgroup walks a second pair with the slots (and
    whatever a tile end leaves behind) of its first"""
    import torch
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    Gp, Gi = _sets_70_30(G2, 130, 2)
    out, pairs = _probe(G2, Gp, Gi)
    assert len(pairs) >= 16
    _check_exact(pinned_ctx, G2, Gp, Gi, _ranks(G2, n))


@pytest.mark.parametrize("m", [10400, 6144])
def test_every_staged_entry_is_read_back(pinned_ctx, m):
    """singleton sets {gene i}: a score IS one staged entry.  10,400 sets (every gene; 163 tiles: the 1,024-thread form);
    6,144 sets (96 tiles: the register-partial form) spread over both slices and every entry position modulo 8.  Distinct
    integers, and an odd leading dimension: every other column starts 8 bytes off 16-byte alignment."""
    if m == G2:
        genes = np.arange(G2, dtype=np.int32)
    else:
        half = (np.arange(m // 2, dtype=np.int64) * 5200) // (m // 2)     # 3,072 distinct positions of a 5,200-gene slice
        assert len(np.unique(half)) == m // 2 and set(half % 8) == set(range(8)) and half.max() >= 5192
        genes = np.concatenate([half, 5200 + half]).astype(np.int32)
    Gp = np.arange(m + 1, dtype=np.int32)
    X = _ranks(G2, 3, seed=5)
    X[:, 1] += G2
    X[:, 2] += 2 * G2
    S = _check_exact(pinned_ctx, G2, Gp, genes, X, ldx=G2 + 7)
    assert np.array_equal(S, X[genes])
