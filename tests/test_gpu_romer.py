"""plaid.romer on the device (kernels_romer.hip, shard_romer.cpp) -- `pytest -m gpu`.

What is checked, and against what:
  1. romer_key_kernel and 2 x the average ranks of the rank kernels (plaidhip_dev_colranks_dense_f64), bit for bit against romer_ref.keys_np and 2 x scipy's rankdata
     ("average"): t given in roast's tile layout over rows with holes (a universe index list); U = 1, 2, 63, 64, 65, 1,030
     and 12,300 (past the rankers' 12,288-key switch, three rotations); nrot = 1, 63, 64, 65, 130 with the chunk forced to 64
     (a second and a third launch); columns that are all equal, +-0.0 mixed (must tie), of one sign only (floormean's mass tie
     at 0 and at 1), with +-Inf; the input's tile padding is NaN and must not be read into a key; the tail of every column
     and what follows the matrices are not written.  A NaN t is keyed as 0.0 and raises the flag.
  2. The sides (the rank crossprod and romer_count_kernel; romer_mean50_kernel), int64 equality with romer_ref.sides_np on
     given average ranks: sets of 0, 1, 2, 3, 63, 64, 65, 300 members,
     the whole universe, one at the mean50 cap and one above it; keys with many ties (duplicates straddle the h-th key); 70
     rotations (a full and a partial tile), all at once and in chunks of 64.  The counts against numpy's on the device's own
     sides, exactly; the observed column through the same kernel on a one-column matrix.
  3. End to end against the 50-digit reference, whose cases are decidable (tests/test_romer_ref.py): the tables follow bit
     for bit from the reference's counts (plaidhip_romer_finish's form), for the three statistics, shrink.resid TRUE and FALSE
     and supplied factors; the empty set, a set whose only gene is outside the universe, an all-zero gene and a duplicated gene.
  4. Generated against supplied rotations; 1, 2 and 3 shards on the hook with 300 rotations (five tiles) and 64 (one tile:
     shards without work) bit for bit the one-device call; the counts of two half calls add up to the whole's; a failing shard
     writes nothing; plaid_romer_contrasts against the single calls; and rotation (r0 = 1, w = 0) reproduces the observed
     sides (p = 1 on every side), which ties the rotated chain to the observed one."""
import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers import limma_ref as lr
from tests.helpers import romer_ref as mr

pytestmark = pytest.mark.gpu

STAT_ID = engine.ROMER_STATISTIC
SENT = -7.0


def _dev():
    import torch
    return torch.device("cuda", 0)


def column(kind, rows, rng):
    """one rotation's t over all rows"""
    t = np.round(rng.normal(size=rows) * 4) / 4                          # many ties
    if kind == 1:
        t[:] = 1.75                                                      # all equal
    elif kind == 2:
        t[rng.random(rows) < 0.6] = 0.0
        t[rng.random(rows) < 0.3] = -0.0                                 # +-0.0 mixed: one tie
    elif kind == 3:
        t = np.abs(t) * 0.3 + 0.125                                      # positive, mostly under floormean's floor of 1
    elif kind == 4:
        t = -np.abs(t) - 0.5                                             # negative only
    elif kind == 5:
        t[rng.random(rows) < 0.2] = np.inf
        t[rng.random(rows) < 0.2] = -np.inf
    return t


def tiles(t):
    """rows x nrot -> roast's layout [tile][rows][64], the padding NaN"""
    rows, nrot = t.shape
    ntile = (nrot + 63) // 64
    Z = np.full((ntile, rows, 64), np.nan)
    for k in range(nrot):
        Z[k // 64, :, k % 64] = t[:, k]
    return Z


def device_keys_ranks(ctx, t, uidx, stat, chunk):
    """(keys a, b, c as U x nrot or None, 2 x the rank kernels' average ranks of them likewise, flag) of the device; asserts
    that nothing beside them was written"""
    import torch
    dev = _dev()
    rows, nrot = t.shape
    nuniv = len(uidx)
    ldu = nuniv + (nuniv & 1) + 2
    Zd = torch.from_numpy(tiles(t)).to(dev)
    ud = torch.from_numpy(np.ascontiguousarray(uidx, dtype=np.int32)).to(dev)
    floor = stat == "floormean"
    K = [torch.full((nrot * ldu + 5,), SENT, dtype=torch.float64, device=dev) for _ in range(3)]
    R = [torch.full((nrot * ldu + 5,), -7.0, dtype=torch.float64, device=dev) for _ in range(3)]
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.dev_romer_keys(Zd.data_ptr(), rows, ud.data_ptr(), nuniv, ldu, STAT_ID[stat], nrot, chunk, K[0].data_ptr(),
                       K[1].data_ptr() if floor else None, K[2].data_ptr(), flag.data_ptr())
    keys, ranks = [], []
    for e in range(3):
        if e == 1 and not floor:
            keys.append(None)
            ranks.append(None)
            continue
        ctx.dev_colranks_dense(K[e].data_ptr(), ldu, nuniv, nrot, R[e].data_ptr(), ldu)      # ties average, power 1
        ctx.synchronize()
        Kh, Rh = K[e].cpu().numpy(), R[e].cpu().numpy()
        assert (Kh[nrot * ldu:] == SENT).all() and (Rh[nrot * ldu:] == -7).all()
        Kh, Rh = Kh[:nrot * ldu].reshape(nrot, ldu), Rh[:nrot * ldu].reshape(nrot, ldu)
        assert (Kh[:, nuniv:] == SENT).all() and (Rh[:, nuniv:] == -7).all()      # the tail of every column
        keys.append(Kh[:, :nuniv].T.copy())
        twice = 2.0 * Rh[:, :nuniv].T
        assert (twice == np.rint(twice)).all()
        ranks.append(twice.astype(np.int64))
    ctx.synchronize()
    return keys, ranks, int(flag.cpu().numpy()[0])


KEY_CASES = [(1, 1), (2, 63), (63, 64), (64, 65), (65, 130), (1030, 130), (12300, 3)]


@pytest.mark.parametrize("stat", ["mean", "floormean"])
@pytest.mark.parametrize("case", KEY_CASES, ids=[f"{u}x{k}" for u, k in KEY_CASES])
def test_keys_and_ranks_bit_for_bit(hip_ctx, case, stat):
    nuniv, nrot = case
    rng = np.random.default_rng(1000 * nuniv + nrot)
    rows = nuniv + nuniv // 3 + 2
    uidx = np.sort(rng.choice(rows, size=nuniv, replace=False))
    t = np.column_stack([column(k % 6, rows, rng) for k in range(nrot)])
    hole = np.setdiff1d(np.arange(rows), uidx)
    t[hole] = 1e300                                                      # rows outside the universe: never keyed
    chunk = 64 if nrot > 64 else 0
    keys, ranks, flag = device_keys_ranks(hip_ctx, t, uidx, stat, chunk)
    assert flag == 0
    want = mr.keys_np(t[uidx], stat)
    for e in range(3):
        if want[e] is None:
            assert keys[e] is None
            continue
        assert np.array_equal(keys[e].view(np.int64), np.ascontiguousarray(want[e]).view(np.int64)), ("key", e)
        assert not (np.signbit(keys[e]) & (keys[e] == 0.0)).any()        # no -0.0 reaches a ranker
        assert np.array_equal(ranks[e], mr.rank2_np(want[e])), ("rank", e)
    if chunk:                                                            # the chunking changes no bit
        k2, r2, _ = device_keys_ranks(hip_ctx, t, uidx, stat, 0)
        for e in range(3):
            if keys[e] is not None:
                assert np.array_equal(k2[e].view(np.int64), keys[e].view(np.int64)) and np.array_equal(r2[e], ranks[e])


def test_a_nan_t_is_keyed_as_zero_and_flagged(hip_ctx):
    rng = np.random.default_rng(5)
    t = rng.normal(size=(9, 3))
    t[4, 1] = np.nan
    uidx = np.array([0, 2, 4, 5, 8])
    keys, ranks, flag = device_keys_ranks(hip_ctx, t, uidx, "mean", 0)
    assert flag == 1 and keys[0][2, 1] == 0.0 and keys[2][2, 1] == 0.0
    want = mr.keys_np(t[uidx], "mean")
    assert np.array_equal(ranks[0], mr.rank2_np(want[0])) and np.array_equal(ranks[2], mr.rank2_np(want[2]))


# ---- the sides -------------------------------------------------------------------------------------------------------------------
NU_SIDES = 16400
SIDE_SIZES = (0, 1, 2, 3, 63, 64, 65, 300, NU_SIDES, engine.ROAST_MEAN50_MAX, engine.ROAST_MEAN50_MAX + 1)
_SIDES = {}


def sides_case():
    """2 rank matrices (U x 70) of tied keys, the sets and numpy's sides per statistic: made once"""
    if not _SIDES:
        rng = np.random.default_rng(77)
        nrot = 70
        t = np.round(rng.normal(size=(NU_SIDES, nrot)) * 8) / 8
        sets = [np.sort(rng.choice(NU_SIDES, size=k, replace=False)).astype(np.int32) for k in SIDE_SIZES]
        _SIDES["sets"], _SIDES["nrot"] = sets, nrot
        for stat in mr.STATS:
            a, b, c = mr.keys_np(t, stat)
            Ra, Rc = mr.rank2_np(a), mr.rank2_np(c)
            Rb = mr.rank2_np(b) if b is not None else None
            want = [mr.sides_np(Ra, Rb, Rc, s, stat, NU_SIDES) if len(s) else None for s in sets]
            _SIDES[stat] = (Ra, Rb, Rc, want)
    return _SIDES


def device_sides(ctx, Ra, Rb, Rc, sets, stat, chunk, obs=None):
    """(stat m x nrot x 3 int64 with the sentinel where nothing was written, cnt m x 3 or None)"""
    import torch
    dev = _dev()
    nuniv, nrot = Ra.shape
    ldu = nuniv + (nuniv & 1) + 2
    def up(Rm):
        if Rm is None:
            return None
        P = np.full((nrot, ldu), 0.0)
        P[:, :nuniv] = Rm.T / 2.0                                        # the average ranks, as the rank kernels write them
        return torch.from_numpy(P).to(dev)
    A, B, Cc = up(Ra), up(Rb), up(Rc)
    Gp, Gi = mr.pattern([list(s) for s in sets])
    Gpd, Gid = torch.from_numpy(Gp).to(dev), torch.from_numpy(np.concatenate([Gi, [0]]).astype(np.int32)).to(dev)
    m = len(sets)
    S = torch.full((m * nrot * 3 + 4,), -9, dtype=torch.int64, device=dev)
    od = cd = None
    if obs is not None:
        od = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.int64)).to(dev)
        cd = torch.zeros((m * 3 + 2,), dtype=torch.int32, device=dev)
        cd[m * 3:] = -7
    torch.cuda.synchronize()
    ctx.dev_romer_sides(A.data_ptr(), None if B is None else B.data_ptr(), Cc.data_ptr(), ldu, nuniv, Gpd.data_ptr(), Gid.data_ptr(),
                        m, STAT_ID[stat], nrot, chunk, S.data_ptr(), None if od is None else od.data_ptr(),
                        None if cd is None else cd.data_ptr())
    ctx.synchronize()
    Sh = S.cpu().numpy()
    assert (Sh[m * nrot * 3:] == -9).all()
    cnt = None
    if cd is not None:
        ch = cd.cpu().numpy()
        assert (ch[m * 3:] == -7).all()
        cnt = ch[:m * 3].reshape(m, 3)
    return Sh[:m * nrot * 3].reshape(m, nrot, 3), cnt


@pytest.mark.parametrize("stat", mr.STATS)
def test_sides_and_counts_exactly(hip_ctx, stat):
    case = sides_case()
    sets, nrot = case["sets"], case["nrot"]
    Ra, Rb, Rc, want = case[stat]
    got, _ = device_sides(hip_ctx, Ra, Rb, Rc, sets, stat, 0)
    capped = [stat == "mean50" and len(s) > engine.ROAST_MEAN50_MAX for s in sets]
    for s, w in enumerate(want):
        if w is None or capped[s]:
            assert (got[s] == -9).all(), s                               # no member, or above the cap: not written
        else:
            assert np.array_equal(got[s], w), (s, len(sets[s]))
    assert sum(capped) == (2 if stat == "mean50" else 0)
    # the observed column through the same kernel: rotation 3 as a one-column matrix
    pick = lambda Rm: None if Rm is None else Rm[:, 3:4]
    obs, _ = device_sides(hip_ctx, pick(Ra), pick(Rb), pick(Rc), sets, stat, 0)
    assert np.array_equal(obs[:, 0], got[:, 3])
    # the counts on the device's own sides, in chunks of 64 (a second launch) and all at once
    obs3 = np.where(obs[:, 0] == -9, 0, obs[:, 0])
    for chunk in (64, 0):
        again, cnt = device_sides(hip_ctx, Ra, Rb, Rc, sets, stat, chunk, obs=obs3)
        assert np.array_equal(again, got)
        live = np.array([w is not None and not c for w, c in zip(want, capped)])
        assert np.array_equal(cnt[live], (got[live] >= obs3[live][:, None, :]).sum(axis=1))
        assert (cnt[~live] == 0).all()
        assert (cnt[live] >= 1).all()                                    # (rotation 3 is among them)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
E2E = [("a", "mean", "shrunk"), ("a", "floormean", "shrunk"), ("a", "mean50", "shrunk"), ("a", "mean", "plain"),
       ("b", "floormean", "plain"), ("b", "mean50", "given"), ("wide", "mean", "shrunk"), ("wide", "mean50", "plain")]


def run_case(ctx, name, stat, mode, **kw):
    X, D, use, K, sets, W, _ = mr.e2e_case(name)
    Gp, Gi = mr.pattern(sets)
    shrink = mr.given_shrink(name) if mode == "given" else None
    return ctx.romer(X, D, Gp, Gi, use, K, stat, shrink_resid=mode == "shrunk", shrink=shrink, rotations=W, **kw)


@pytest.mark.parametrize("case", E2E, ids=["-".join(c) for c in E2E])
def test_end_to_end_against_the_50_digit_reference(hip_ctx, case):
    name, stat, mode = case
    ref = mr.e2e_reference(name, stat, mode)[0]
    nrot = mr.e2e_case(name)[5].shape[1]
    out, hyper = run_case(hip_ctx, name, stat, mode)
    want = mr.finish_np(ref["cnt"], ref["msize"], nrot, stat)
    got = out[:, :, 0, 0]
    b = np.rint(got[:, 1:4] * (nrot + 1) - 1)
    live = ref["msize"] >= 1
    print(f"[romer e2e] {case}: counts differ in {int((b[live] != ref['cnt'][live]).sum())} places")
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert np.isnan(got[5, 1:]).all() and got[5, 0] == 0 and np.isnan(got[6, 1:]).all() and got[6, 0] == 0
    assert hyper[0, 4] == ref["U"] and hyper[0, 5] == nrot and hyper[0, 6] == 0 and hyper[0, 7] == 0
    if mode == "shrunk":
        assert abs(hyper[0, 8] - ref["pi"]) <= 1e-9 and hyper[0, 8] > 0
    else:
        assert hyper[0, 8] == 0.0


# ---- wrappers and sharding -----------------------------------------------------------------------------------------------------------
def counts_of(out, nrot):
    return np.rint(out[:, 1:4] * (nrot + 1) - 1)


def big_case(nrot):
    X, D, use, K, sets, _, _ = mr.e2e_case("b")
    Gp, Gi = mr.pattern(sets)
    return X, D, use, K, Gp, Gi, engine.roast_rotations(D, use, 0, nrot, seed=2)


@pytest.mark.parametrize("nrot", [300, 64])
@pytest.mark.parametrize("stat", ["mean", "mean50"])
def test_shards_have_the_one_device_bits(hip_ctx, nrot, stat):
    X, D, use, K, Gp, Gi, W = big_case(nrot)
    out, hyper = hip_ctx.romer(X, D, Gp, Gi, use, K, stat, nrot=nrot, seed=2)
    given, h2 = hip_ctx.romer(X, D, Gp, Gi, use, K, stat, rotations=W)              # generated against supplied rotations
    assert np.array_equal(given.view(np.int64), out.view(np.int64)) and np.array_equal(h2.view(np.int64), hyper.view(np.int64))
    for nshards in (1, 2, 3):
        status, o2, hy = mr.run_sharded(nshards, X, D, Gp, Gi, use, K, set_statistic=stat, nrot=nrot, seed=2)
        assert status == _lib.OK
        assert np.array_equal(o2.view(np.int64), out.view(np.int64)), nshards
        assert np.array_equal(hy.view(np.int64), hyper.view(np.int64)), nshards
    if nrot == 300:                                                                # two half calls add up to the whole
        o_a, _ = hip_ctx.romer(X, D, Gp, Gi, use, K, stat, rotations=W[:, :128])
        o_b, _ = hip_ctx.romer(X, D, Gp, Gi, use, K, stat, rotations=W[:, 128:])
        live = out[:, 0, 0, 0] >= 1
        whole = counts_of(out[:, :, 0, 0], 300)[live]
        assert np.array_equal(whole, counts_of(o_a[:, :, 0, 0], 128)[live] + counts_of(o_b[:, :, 0, 0], 172)[live])


def test_a_failing_shard_writes_nothing(hip_ctx):
    X, D, use, K, Gp, Gi, _ = big_case(130)
    status, out, hyper = mr.run_sharded(3, X, D, Gp, Gi, use, K, fail=1, set_statistic="mean", nrot=130, seed=2)
    assert status != _lib.OK and (out == -7.0).all() and (hyper == -7.0).all()


def test_the_unit_rotation_reproduces_the_observed_sides(hip_ctx):
    X, D, use, K, sets, _, _ = mr.e2e_case("a")
    Gp, Gi = mr.pattern(sets)
    W = np.zeros((X.shape[1] + 1, 1))
    W[0, 0] = 1.0
    out, _ = hip_ctx.romer(X, D, Gp, Gi, use, K, "mean", shrink_resid=False, rotations=W)
    live = out[:, 0, 0, 0] >= 1
    assert live.sum() == len(sets) - 2
    assert (out[live, 1:4, 0, 0] == 1.0).all()                          # b = 1 of 1 on every side: the sides are the observed ones


def test_contrasts_wrapper_equals_the_single_calls(hip_ctx):
    rng = np.random.default_rng(12)
    g, n = 30, 14
    Xv = np.round(rng.normal(size=(g, n)) * 64) / 64
    X = plaid_amd.NamedMatrix(Xv, [f"g{i}" for i in range(g)], [f"s{i}" for i in range(n)])
    Y = np.zeros((n, 2))
    Y[::2, 0] = 1.0
    Y[:7, 1] = 1.0
    Y[12:, 1] = np.nan
    Yn = plaid_amd.NamedMatrix(Y, X.colnames, ["a", "b"])
    G = {"s1": ["g1", "g2", "g3", "g9"], "s2": [f"g{i}" for i in range(10, 25)], "s3": ["g0", "g29"]}
    Bz = np.zeros((n, 0))
    Ws = [engine.roast_rotations(*lr.contrast_design(Y, Bz, j), j, 99, 4) for j in range(2)]
    tabs, hyp = plaid_amd.plaid_romer_contrasts(X, Yn, G, nrot=99, seed=4, ctx=hip_ctx)
    for j, nm in enumerate(["a", "b"]):
        Dj, uj = lr.contrast_design(Y, Bz, j)
        one, h1 = plaid_amd.plaid_romer(X, Dj, G, contrasts=np.array([0.0, 1.0]), use=uj, rotations=Ws[j], ctx=hip_ctx)
        assert tabs[nm].rownames == one["1"].rownames and tabs[nm].colnames == list(engine.ROMER_COLUMNS)
        assert np.array_equal(tabs[nm].values.view(np.int64), one["1"].values.view(np.int64)), nm
        assert hyp[nm]["n.genes"] == h1["n.genes"] and hyp[nm]["proportion"][nm] == h1["proportion"]["1"]
    by_up, _ = plaid_amd.plaid_romer_contrasts(X, Yn, G, nrot=99, seed=4, sort_by="up", ctx=hip_ctx)
    assert (np.diff(by_up["a"].values[:, 1]) >= 0).all()
