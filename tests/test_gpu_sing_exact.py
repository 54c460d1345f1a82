"""replaid.sing.exact on the GPU (include/plaidhip.h: plaidhip_sing_exact, _multi, plaidhip_dev_sing_mad_f64;
kernels_sing.hip: sing_score_kernel, sing_mad_kernel).

Every result is integer work closed by two divisions and at most two subtractions (score) or one product (dispersion), so
the device must return the bits of the pinned form in numpy (tests/helpers/sing_mad.py) in every case.  The dispersion
kernel has ONE route for every set size; its seams are the 64 lanes of a wavefront, the 64 bits of a map word and the
4,096 positions of a run of 64 words.  A dgCMatrix scores as its dense form; sharding, the mixed precision mode and the
Python alignment must not change a bit.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import exact_ref as er
from tests.helpers import sing_mad as sm
from tests.helpers import sharded_hooks
from tests.test_gpu_ssgsea_exact import SHAPES, _sets, _sparse, _tied
from tests.test_sing_exact_ref import pbmc_case

pytestmark = pytest.mark.gpu


def same_all(got, exp, what=""):
    assert sorted(got) == sorted(exp), f"{what}: outputs {sorted(got)} expected {sorted(exp)}"
    for name in exp:
        er.assert_same_bits(got[name], exp[name], f"{what} {name}")


def _sized_sets(g, sizes, seed=17, extra=()):
    rng = np.random.default_rng(seed)
    Gi, Gp = [], [0]
    for k in sizes:
        Gi.extend(sorted(rng.choice(g, size=k, replace=False)))
        Gp.append(len(Gi))
    for rows in extra:
        Gi.extend(rows)
        Gp.append(len(Gi))
    return np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)


def _down(g, m, seed=29):
    """m down sets, the first one empty"""
    rng = np.random.default_rng(seed)
    sizes = [0] + [int(rng.integers(1, max(2, min(g, 200)) + 1)) for _ in range(m - 1)]
    return _sized_sets(g, [min(k, g) for k in sizes], seed=seed + 1)


# --------------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("g,n", SHAPES)
def test_shapes_equal_the_pinned_form(hip_ctx, g, n):
    X = _tied(g, n)
    Gp, Gi = _sets(g, 24)
    Dp, Di = _down(g, 24)
    for center in (True, False):
        same_all(hip_ctx.sing_exact(X, Gp, Gi, Dp, Di, center, True), sm.pinned(X, Gp, Gi, Dp, Di, center),
                 f"g={g} n={n} center={center}")
    up = hip_ctx.sing_exact(X, Gp, Gi, None, None, True, True)
    same_all(up, sm.pinned(X, Gp, Gi, None, None, True), f"g={g} n={n} up only")


def test_hand_case(hip_ctx):
    X = np.asfortranarray([[5.0], [1.0], [3.0], [3.0], [2.0]])
    Gp = np.array([0, 3, 5], dtype=np.int32)
    Gi = np.array([0, 2, 3, 0, 1], dtype=np.int32)
    c = hip_ctx.sing_exact(X, Gp, Gi)
    u = hip_ctx.sing_exact(X, Gp, Gi, center=False)
    assert u["UpScore"][:, 0].tolist() == [(11.0 / 3.0 - 2.0) / 2.0, 0.5]
    assert c["UpScore"][:, 0].tolist() == [(11.0 / 3.0 - 2.0) / 2.0 - 0.5, 0.0]
    assert c["UpDispersion"][:, 0].tolist() == [0.0, 1.4826 * 2.0]


# --------------------------------------------------------------------------------------------------- 2. the kernel's seams
@pytest.mark.parametrize("g", [64, 65, 4096, 4097, 8192, 8193])
def test_set_sizes_and_column_lengths_at_the_kernel_seams(hip_ctx, g):
    """sets of 1, 2, 63 / 64 / 65, 4,095 / 4,096 / 4,097, N - 1, N and 0 members where g allows, in columns whose map ends
    at, and one past, a word and a run of 64 words; a member list given out of order; tied and tie-free columns"""
    n = 9
    X = _tied(g, n)
    X[:, 2] = np.random.default_rng(4).permutation(g)                       # tie-free
    sizes = [k for k in (1, 2, 3, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, g - 2, g - 1) if 0 < k < g] + [0, g]
    shuffled = [int(v) for v in np.random.default_rng(8).permutation(g)[:min(g, 70)]]
    Gp, Gi = _sized_sets(g, sizes, extra=(shuffled,))
    Dp, Di = _sized_sets(g, sizes[::-1], seed=31, extra=(shuffled[::-1],))
    got = hip_ctx.sing_exact(X, Gp, Gi, Dp, Di, True, True)
    same_all(got, sm.pinned(X, Gp, Gi, Dp, Di, True), f"g={g}")
    j0, jN = len(sizes) - 2, len(sizes) - 1
    assert np.isnan(got["UpScore"][[j0, jN]]).all() and np.isnan(got["UpDispersion"][j0]).all()
    assert np.isfinite(got["UpDispersion"][jN]).all()
    assert np.isnan(got["TotalScore"][1]).all()                             # its down column is the empty one


def test_one_tie_group_and_a_median_between_two_tie_groups(hip_ctx):
    g = 1000
    X = np.zeros((g, 3), order="F")
    X[:, 0] = 7.0                                                           # one tie group: every rank 1
    X[: g // 2, 1] = 1.0                                                    # two tie groups, ranks 501 and 1
    X[:, 2] = np.repeat(np.arange(g // 4), 4)                               # groups of four
    Gp, Gi = _sized_sets(g, [1, 2, 10, 11, 500, 999, g], extra=(list(range(495, 505)), list(range(490, 500)) + list(range(500, 510))))
    got = hip_ctx.sing_exact(X, Gp, Gi, Gp, Gi, False, True)
    exp = sm.pinned(X, Gp, Gi, Gp, Gi, False)
    same_all(got, exp, "tie groups")
    assert (got["UpDispersion"][:, 0] == 0.0).all()
    assert got["UpDispersion"][-1, 1] == 1.4826 * 250.0                     # ten and ten: the median lies between the groups
    er.assert_same_bits(got["DownDispersion"], got["UpDispersion"], "reflection")


def test_the_gene_bound_and_one_above(hip_ctx):
    from plaid_amd._lib import EUNSUPPORTED, PlaidHipError
    g, n = 131072, 3
    X = np.asfortranarray(np.round(np.random.default_rng(2).normal(0, 50, size=(g, n)), 0))
    Gp, Gi = _sized_sets(g, [1, 64, 5000, 65537, g - 1, g])
    same_all(hip_ctx.sing_exact(X, Gp, Gi), sm.pinned(X, Gp, Gi), f"g={g}")
    X1 = np.asfortranarray(np.vstack([X, np.ones((1, n))]))
    with pytest.raises(PlaidHipError) as e:
        hip_ctx.sing_exact(X1, Gp, Gi)
    assert e.value.code == EUNSUPPORTED
    off = hip_ctx.sing_exact(X1, Gp, Gi, dispersion=False)                  # the score has no such bound
    er.assert_same_bits(off["UpScore"], sm.pinned(X1, Gp, Gi)["UpScore"], "g + 1, scores only")


def test_nan_column_gives_nan_everywhere(hip_ctx):
    g, n = 3001, 9
    X = np.asfortranarray(np.round(np.random.default_rng(9).normal(0, 2, size=(g, n)), 0))
    X[100, 4] = np.nan
    Gp, Gi = _sets(g, 12)
    Dp, Di = _down(g, 12)
    got = hip_ctx.sing_exact(X, Gp, Gi, Dp, Di)
    for name in sm.NAMES:
        assert np.isnan(got[name][:, 4]).all(), name
    same_all(got, sm.pinned(X, Gp, Gi, Dp, Di), "NaN column")
    Xs = sp.csc_matrix(np.where(np.isnan(X), 0.0, X))
    Xs.data[5] = np.nan
    same_all(hip_ctx.sing_exact(Xs, Gp, Gi, Dp, Di), sm.pinned(Xs.toarray(), Gp, Gi, Dp, Di), "NaN among the stored values")


# --------------------------------------------------------------------------------------------------- 3. arguments
def test_dispersion_off_gives_the_same_scores(hip_ctx):
    g, n = 3001, 37
    X = _tied(g, n)
    Gp, Gi = _sets(g, 24)
    Dp, Di = _down(g, 24)
    on = hip_ctx.sing_exact(X, Gp, Gi, Dp, Di, True, True)
    off = hip_ctx.sing_exact(X, Gp, Gi, Dp, Di, True, False)
    assert sorted(off) == ["DownScore", "TotalScore", "UpScore"]
    for name in off:
        er.assert_same_bits(off[name], on[name], name)
    assert sorted(hip_ctx.sing_exact(X, Gp, Gi, dispersion=False)) == ["UpScore"]


# --------------------------------------------------------------------------------------------------- 4. dgCMatrix
@pytest.mark.parametrize("density", [0.0, 0.05, 0.6])
def test_dgcmatrix_equals_the_dense_form(hip_ctx, density):
    for g, n in ((3001, 64), (20000, 64)):
        Xs = _sparse(g, n, density, 31)
        Gp, Gi = _sets(g, 24)
        Dp, Di = _down(g, 24)
        dense = hip_ctx.sing_exact(Xs.toarray(), Gp, Gi, Dp, Di)
        same_all(hip_ctx.sing_exact(Xs, Gp, Gi, Dp, Di), dense, f"g={g} density={density}")
        same_all(dense, sm.pinned(Xs.toarray(), Gp, Gi, Dp, Di), "dense form vs the pinned form")


# --------------------------------------------------------------------------------------------------- 5. sharding, modes
def _run_hook(nshards, X, Gp, Gi, Dp, Di, center=True, fail=-1):
    return sharded_hooks.sing_exact(nshards, X, Gp, Gi, Dp, Di, center, fail=fail)


@pytest.mark.parametrize("kind", ["dense", "csc"])
def test_sharded_engine_is_bit_identical(hip_ctx, kind):
    """1, 2, 3 and 7 shards; 5 columns over 7 shards leave empty shards"""
    g = 3001
    Gp, Gi = _sets(g, 24)
    Dp, Di = _down(g, 24)
    for n in (513, 5):
        X = _tied(g, n) if kind == "dense" else _sparse(g, n, 0.05, 41)
        exp = hip_ctx.sing_exact(X, Gp, Gi, Dp, Di)
        for nshards in (1, 2, 3, 7):
            rc, S = _run_hook(nshards, X, Gp, Gi, Dp, Di)
            assert rc == 0
            same_all(S, exp, f"{kind} n={n} nshards={nshards}")


def test_injected_shard_failure_returns_an_error(hip_ctx):
    from plaid_amd._lib import load
    g, n = 500, 300
    X = _tied(g, n)
    Gp, Gi = _sets(g, 10)
    Dp, Di = _down(g, 10)
    rc, _ = _run_hook(3, X, Gp, Gi, Dp, Di, fail=1)
    assert rc != 0 and b"injected failure" in load().plaidhip_last_error_string()


def test_multi_on_one_device_equals_the_context_call(hip_ctx):
    import plaid_amd
    g, n = 3001, 23
    Gp, Gi = _sets(g, 24)
    Dp, Di = _down(g, 24)
    for X in (_tied(g, n), _sparse(g, n, 0.05, 43)):
        same_all(plaid_amd.sing_exact_multi(X, Gp, Gi, Dp, Di, True, True, devices=1), hip_ctx.sing_exact(X, Gp, Gi, Dp, Di),
                 "multi")
        same_all(plaid_amd.sing_exact_multi(X, Gp, Gi, center=False, dispersion=False, devices=1),
                 hip_ctx.sing_exact(X, Gp, Gi, center=False, dispersion=False), "multi, up scores only")


def test_mixed_mode_does_not_change_a_bit(hip_ctx):
    g, n = 3001, 33
    X = _tied(g, n)
    Gp, Gi = _sets(g, 24)
    Dp, Di = _down(g, 24)
    exp = hip_ctx.sing_exact(X, Gp, Gi, Dp, Di)
    hip_ctx.set_precision("mixed")
    try:
        got = hip_ctx.sing_exact(X, Gp, Gi, Dp, Di)
    finally:
        hip_ctx.set_precision("f64")
    same_all(got, exp, "mixed mode")


# --------------------------------------------------------------------------------------------------- 6. alignment
def test_python_wrapper_on_the_pbmc_fixture(hip_ctx, golden_dir):
    import plaid_amd
    Xn, matG, matD = pbmc_case(golden_dir)
    exp = dict(np.load(os.path.join(golden_dir, "sing_exact_pbmc3k50.npz"), allow_pickle=False))
    for Xin in (Xn, plaid_amd.NamedMatrix(Xn.values.toarray(), Xn.rownames, Xn.colnames)):
        got = plaid_amd.replaid_sing_exact(Xin, matG, matD, ctx=hip_ctx)
        same_all({k: v.values for k, v in got.items()}, exp, "pbmc3k-50")
        assert list(got["TotalScore"].rownames) == list(matG.colnames)
        assert list(got["TotalScore"].colnames) == list(Xn.colnames)
    up = plaid_amd.replaid_sing_exact(Xn, matG, dispersion=False, ctx=hip_ctx)
    assert sorted(up) == ["UpScore"]
    er.assert_same_bits(up["UpScore"].values, exp["UpScore"], "up only, scores only")
    with pytest.raises(ValueError):
        plaid_amd.replaid_sing_exact(Xn, matG, plaid_amd.NamedMatrix(matD.values[:, :3], matD.rownames, matD.colnames[:3]),
                                     ctx=hip_ctx)


# --------------------------------------------------------------------------------------------------- the device entry
def test_dev_entry_equals_the_host_entry(hip_ctx):
    import torch
    dev = torch.device("cuda", 0)
    g, n = 3001, 19
    X = _tied(g, n)
    X[7, 2] = np.nan
    Gp, Gi = _sets(g, 24)
    m = len(Gp) - 1
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    dGp, dGi = torch.from_numpy(Gp).to(dev), torch.from_numpy(Gi).to(dev)
    R = torch.empty((n, g), dtype=torch.float64, device=dev)
    Q = torch.empty((n, g), dtype=torch.float64, device=dev)
    colnan = torch.empty((n,), dtype=torch.int32, device=dev)
    scratch = torch.empty(2 * g * n, dtype=torch.float64, device=dev)
    hip_ctx.dev_colranks_dense(dX.data_ptr(), g, g, n, R.data_ptr(), g, ties="min")
    hip_ctx.dev_ssgsea_exact_operands(dX.data_ptr(), g, g, n, 0.0, Q.data_ptr(), g, scratch.data_ptr(), colnan.data_ptr())
    S = torch.full((n, m + 3), -7.0, dtype=torch.float64, device=dev)
    hip_ctx.dev_sing_mad(R.data_ptr(), Q.data_ptr(), g, colnan.data_ptr(), g, n, dGp.data_ptr(), dGi.data_ptr(), m, S.data_ptr(),
                         m + 3)
    torch.cuda.synchronize()
    out = S.cpu().numpy().T
    er.assert_same_bits(out[:m], hip_ctx.sing_exact(X, Gp, Gi)["UpDispersion"], "dev entry")
    assert (out[m:] == -7.0).all()
