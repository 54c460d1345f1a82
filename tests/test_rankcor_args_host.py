"""The argument checks of plaid.rankcor (multi.cpp: check_rankcor_call) through plaidhip_rankcor, plaidhip_rankcor_multi and
the sharded test hook, without a GPU: every fault returns its status and text before any device is touched (there is none
here), and the checks run in the order include/plaidhip.h states -- two faults at once report the earlier one."""
import numpy as np
import pytest

from plaid_amd import _lib, engine
from tests.helpers.sharded_hooks import hook

G_ROWS, LISTS = 10, 3
GP = np.array([0, 3, 5], dtype=np.int32)
GI = np.array([0, 1, 2, 8, 9], dtype=np.int32)


def entries():
    lib = _lib.load()
    return {"rankcor": (lib.plaidhip_rankcor, (None,)),                      # (a null context: the checks come first)
            "rankcor_multi": (lib.plaidhip_rankcor_multi, (None, 2)),
            "hook": (hook("rankcor"), (0, 3, -1))}


def ptr(a):
    return None if a is None else a.ctypes.data


def call(which, stat, g, c, Gp, Gi, m, use_rank, ties, out, tot):
    fn, head = entries()[which]
    rc = fn(*head, ptr(stat), g, c, ptr(Gp), ptr(Gi), m, use_rank, ties, ptr(out), ptr(tot))
    return rc, _lib.load().plaidhip_last_error_string().decode()


def good():
    """a valid call's arguments, the outputs holding -7"""
    rng = np.random.default_rng(3)
    stat = np.asfortranarray(rng.normal(size=(G_ROWS, LISTS)))
    stat[2, 1] = np.nan
    return dict(stat=stat, g=G_ROWS, c=LISTS, Gp=GP, Gi=GI, m=2, use_rank=1, ties=0, out=np.full((2, 5, LISTS), -7.0, order="F"),
                tot=np.full(LISTS, -7.0))


FAULTS = [   # name, what to change, status, a word of the text -- in the order of the checks
    ("lists", dict(c=0), _lib.EINVAL, "0 lists"),
    ("dims", dict(g=0), _lib.EINVAL, "bad dims"),
    ("sets", dict(m=-1), _lib.EINVAL, "bad dims"),
    ("null Gp", dict(Gp=None), _lib.EINVAL, "null Gp"),
    ("null stat", dict(stat=None), _lib.EINVAL, "null stat / out / tot_out"),
    ("null out", dict(out=None), _lib.EINVAL, "null stat / out / tot_out"),
    ("null tot", dict(tot=None), _lib.EINVAL, "null stat / out / tot_out"),
    ("use_rank", dict(use_rank=2), _lib.EINVAL, "use_rank = 2"),
    ("ties first", dict(ties=3), _lib.EINVAL, "ties = 3"),
    ("ties random", dict(ties=6), _lib.EINVAL, "ties = 6"),
    ("ties low", dict(ties=-1), _lib.EINVAL, "ties = -1"),
    ("genes", dict(g=131073), _lib.EUNSUPPORTED, "131073 genes (at most 131072)"),
    ("Gp start", dict(Gp=np.array([1, 3, 5], dtype=np.int32)), _lib.EINVAL, "Gp[0] = 1"),
    ("Gp order", dict(Gp=np.array([0, 4, 3], dtype=np.int32)), _lib.EINVAL, "Gp[2] = 3 after 4"),
    ("set size", dict(g=2, Gi=np.array([0, 1, 0, 1, 1], dtype=np.int32)), _lib.EINVAL, "set 1 has 3 members"),
    ("null Gi", dict(Gi=None), _lib.EINVAL, "null Gi"),
    ("Gi high", dict(Gi=np.array([0, 1, 2, 8, 10], dtype=np.int32)), _lib.EINVAL, "Gi[4] = 10 (rows are 0..9)"),
    ("Gi low", dict(Gi=np.array([0, -1, 2, 8, 9], dtype=np.int32)), _lib.EINVAL, "Gi[1] = -1"),
]
RANK = {name: q for q, (name, _, _, _) in enumerate(FAULTS)}


def apply(a, change):
    return {**a, **change}


@pytest.mark.parametrize("which", ["rankcor", "rankcor_multi", "hook"])
@pytest.mark.parametrize("name,change,status,word", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_fault_is_refused_before_any_device(which, name, change, status, word):
    a = apply(good(), change)
    rc, text = call(which, **a)
    assert rc == status and word in text, (rc, text)
    for o in ("out", "tot"):
        if a[o] is not None:
            assert (a[o] == -7).all(), o


PAIRS = [("lists", "null stat"), ("null Gp", "null out"), ("null tot", "use_rank"), ("use_rank", "ties first"),
         ("ties random", "genes"), ("genes", "Gi high"), ("Gp order", "Gi high"), ("null stat", "Gi low"), ("dims", "ties low"),
         ("Gp start", "null Gi")]


@pytest.mark.parametrize("which", ["rankcor", "rankcor_multi", "hook"])
@pytest.mark.parametrize("first,second", PAIRS)
def test_two_faults_report_the_earlier_check(which, first, second):
    assert RANK[first] < RANK[second]
    _, ch1, status, word = FAULTS[RANK[first]]
    _, ch2, _, _ = FAULTS[RANK[second]]
    a = apply(apply(good(), ch2), ch1)
    rc, text = call(which, **a)
    assert rc == status and word in text, (rc, text)


def test_a_valid_call_passes_the_checks_and_then_wants_a_context():
    for use_rank in (0, 1):
        for ties in (0, 1, 2):
            rc, text = call("rankcor", **{**good(), "use_rank": use_rank, "ties": ties})
            assert rc == _lib.EINVAL and "null plaidhip_ctx" in text


def test_the_device_list_and_shard_count_come_first():
    a = good()
    fn = _lib.load().plaidhip_rankcor_multi
    args = (ptr(a["stat"]), 10, 0, ptr(GP), ptr(GI), 2, 1, 0, ptr(a["out"]), ptr(a["tot"]))
    assert fn(None, 0, *args) == _lib.EINVAL and "ndev = 0" in _lib.load().plaidhip_last_error_string().decode()
    assert hook("rankcor")(0, 0, -1, *args) == _lib.EINVAL
    assert "nshards = 0" in _lib.load().plaidhip_last_error_string().decode()


def test_no_sets_is_the_empty_result():
    """m = 0 returns PLAIDHIP_OK with nothing written, on every entry and without a device, as the other entries do; the
    other arguments are still checked"""
    a = good()
    empty = dict(Gp=np.array([0], dtype=np.int32), Gi=None, m=0, out=None)
    for which in ("rankcor_multi", "hook"):
        rc, text = call(which, **{**a, **empty})
        assert rc == _lib.OK, text
        assert (a["tot"] == -7).all()
        rc, text = call(which, **{**a, **empty, "ties": 5})
        assert rc == _lib.EINVAL and "ties = 5" in text


def test_check_rankcor_args_in_python():
    """engine.check_rankcor_args: the same order on what Python can see"""
    s, use_rank, ties = engine.check_rankcor_args([1.0, np.nan, -2.0])
    assert s.shape == (3, 1) and s.dtype == np.float64 and s.flags.f_contiguous and (use_rank, ties) == (1, 0)
    assert engine.check_rankcor_args(np.zeros((4, 2)), use_rank=False, ties="max")[1:] == (0, 2)
    assert engine.check_rankcor_args(np.zeros((4, 2)), ties=1)[2] == 1
    with pytest.raises(ValueError, match="0 lists"):
        engine.check_rankcor_args(np.zeros((4, 0)))
    with pytest.raises(ValueError, match="ties must be one of"):
        engine.check_rankcor_args(np.zeros(4), ties="random")
    with pytest.raises(ValueError, match="genes x lists"):
        engine.check_rankcor_args(np.zeros((2, 2, 2)))
    with pytest.raises(_lib.PlaidHipError, match="131073 genes"):
        engine.check_rankcor_args(np.zeros((131073, 1)))
