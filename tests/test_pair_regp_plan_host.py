"""Host checks of the pair plan's 12-wavefront form (geneset.cpp; no GPU): a collection with more than one gene slice
and at most 12 x 8 tiles is dealt to 12 wavefronts, no more than 8 tiles each, so that the kernel can keep a lane's partial
sums in 8 register pairs; the plan's self-check (every membership scheduled exactly once, in its slice, for its set, in
the stream of the wavefront that owns its tile) covers that form."""
import ctypes as C
import os

import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, synth


def _check(g, Gp, Gi):
    fn = _lib.load().plaidhip_debug_pair_plan_check
    fn.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    fn.restype = C.c_int
    Gp = np.ascontiguousarray(Gp, dtype=np.int32)
    Gi = np.ascontiguousarray(Gi, dtype=np.int32)
    out = (C.c_int64 * 8)()
    assert fn(g, len(Gp) - 1, Gp.ctypes.data, Gi.ctypes.data, 16, out) == 0
    return dict(slices=out[0], chunks=out[1], found=out[2], conflicts=out[3], wrong=out[4], regp=out[5], most=out[6],
                waves=out[7])


def _assert_regp(r, z):
    assert r["found"] == z and r["wrong"] == 0
    assert r["regp"] == 1 and r["waves"] == 12 and 1 <= r["most"] <= 8
    assert r["conflicts"] <= 0.25 * r["chunks"] * 8


def test_synthetic_5000_sets_get_the_12_wavefront_plan():
    g, m = 20000, 5000
    Gp, Gi = synth.geneset_csc(g, m)
    r = _check(g, Gp, Gi)
    assert r["slices"] == 2
    _assert_regp(r, int(Gp[-1]))
    assert r["most"] >= 7            # 79 tiles on 12 wavefronts: some wavefront holds at least 7


def test_hallmarks_over_a_whole_transcriptome(golden_dir):
    """the bundled hallmark collection (50 sets over 4,386 genes) against a 21,930-gene matrix, its genes on every fifth
    row: three gene slices, one tile"""
    M = plaid_amd.gmt2mat(plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt")))
    G = M.values.tocsc()
    G.sort_indices()
    g = 5 * G.shape[0]
    r = _check(g, G.indptr, G.indices * 5)
    assert r["slices"] == 3
    _assert_regp(r, int(G.nnz))
    assert r["most"] == 1


@pytest.mark.parametrize("g,m,regp", [(10224, 700, 0), (10225, 6144, 1), (10225, 6145, 0), (30001, 768, 1)])
def test_eligibility_bounds(g, m, regp):
    Gp, Gi = synth.geneset_csc(g, m, kmin=5, kmax=40)
    r = _check(g, Gp, Gi)
    assert r["found"] == int(Gp[-1]) and r["wrong"] == 0 and r["regp"] == regp
    if regp:
        assert r["waves"] == 12 and r["most"] <= 8
    else:
        assert r["waves"] == 16


def test_cap_binds_when_one_tile_is_far_longer():
    g, m = 20000, 6100
    rng = np.random.default_rng(9)
    sizes = np.full(m, 15)
    sizes[0] = 2000
    Gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    Gi = np.concatenate([np.sort(rng.choice(g, size=k, replace=False)) for k in sizes]).astype(np.int32)
    r = _check(g, Gp, Gi)
    _assert_regp(r, int(Gp[-1]))
    assert r["most"] == 8
