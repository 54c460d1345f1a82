"""The argument checks of plaid.fisher (multi.cpp: check_fisher_call) through plaidhip_fisher, plaidhip_fisher_multi and the
sharded test hook, without a GPU: every fault returns its status and text before any device is touched (there is none
here), and the checks run in the order include/plaidhip.h states -- two faults at once report the earlier one."""
import ctypes as C

import numpy as np
import pytest

from plaid_amd import _lib, engine
from tests.helpers.sharded_hooks import hook

G_ROWS, LISTS = 10, 3
GP = np.array([0, 3, 5], dtype=np.int32)
GI = np.array([0, 1, 2, 8, 9], dtype=np.int32)


def entries():
    lib = _lib.load()
    return {"fisher": (lib.plaidhip_fisher, (None,)),                      # (a null context: the checks come first)
            "fisher_multi": (lib.plaidhip_fisher_multi, (None, 2)),
            "hook": (hook("fisher"), (0, 3, -1))}


def ptr(a):
    return None if a is None else a.ctypes.data


def call(which, sig, g, c, Gp, Gi, m, out, tot, ov_len, ov_idx):
    fn, head = entries()[which]
    rc = fn(*head, ptr(sig), g, c, ptr(Gp), ptr(Gi), m, ptr(out), ptr(tot), ptr(ov_len), ptr(ov_idx))
    return rc, _lib.load().plaidhip_last_error_string().decode()


def good():
    """a valid call's arguments, the outputs holding -7"""
    rng = np.random.default_rng(3)
    sig = np.asfortranarray(rng.integers(-1, 2, size=(G_ROWS, LISTS)).astype(np.int8))
    return dict(sig=sig, g=G_ROWS, c=LISTS, Gp=GP, Gi=GI, m=2, out=np.full((2, 12, LISTS), -7.0, order="F"),
                tot=np.full((2, LISTS), -7.0, order="F"), ov_len=np.full((2, LISTS), -7, dtype=np.int32, order="F"),
                ov_idx=np.full((5, LISTS), -7, dtype=np.int32, order="F"))


def bad_sig(a):
    s = a["sig"].copy(order="F")
    s[4, 1] = 2
    return s


FAULTS = [   # name, what to change, status, a word of the text -- in the order of the checks
    ("lists", dict(c=0), _lib.EINVAL, "0 lists"),
    ("dims", dict(g=0), _lib.EINVAL, "bad dims"),
    ("null Gp", dict(Gp=None), _lib.EINVAL, "null Gp"),
    ("null sig", dict(sig=None), _lib.EINVAL, "null sig / out / tot_out"),
    ("null out", dict(out=None), _lib.EINVAL, "null sig / out / tot_out"),
    ("null tot", dict(tot=None), _lib.EINVAL, "null sig / out / tot_out"),
    ("only ov_len", dict(ov_idx=None), _lib.EINVAL, "both or neither"),
    ("only ov_idx", dict(ov_len=None), _lib.EINVAL, "both or neither"),
    ("genes", dict(g=(1 << 26) + 1), _lib.EUNSUPPORTED, "67108865 genes (at most 67108864)"),
    ("Gp start", dict(Gp=np.array([1, 3, 5], dtype=np.int32)), _lib.EINVAL, "Gp[0] = 1"),
    ("Gp order", dict(Gp=np.array([0, 4, 3], dtype=np.int32)), _lib.EINVAL, "Gp[2] = 3 after 4"),
    ("null Gi", dict(Gi=None), _lib.EINVAL, "null Gi"),
    ("Gi high", dict(Gi=np.array([0, 1, 2, 8, 10], dtype=np.int32)), _lib.EINVAL, "Gi[4] = 10 (rows are 0..9)"),
    ("Gi low", dict(Gi=np.array([0, -1, 2, 8, 9], dtype=np.int32)), _lib.EINVAL, "Gi[1] = -1"),
    ("sig value", dict(sig=bad_sig), _lib.EINVAL, "sig[14] = 2"),
]
RANK = {name: q for q, (name, _, _, _) in enumerate(FAULTS)}


def apply(a, change):
    return {**a, **{k: (v(a) if callable(v) else v) for k, v in change.items()}}


@pytest.mark.parametrize("which", ["fisher", "fisher_multi", "hook"])
@pytest.mark.parametrize("name,change,status,word", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_fault_is_refused_before_any_device(which, name, change, status, word):
    a = apply(good(), change)
    rc, text = call(which, **a)
    assert rc == status and word in text, (rc, text)
    for o in ("out", "tot", "ov_len", "ov_idx"):
        if a[o] is not None:
            assert (a[o] == -7).all(), o


PAIRS = [("lists", "null sig"), ("null Gp", "null out"), ("null tot", "only ov_len"), ("only ov_idx", "genes"),
         ("genes", "Gi high"), ("Gp order", "Gi high"), ("Gi low", "sig value"), ("null sig", "Gi high"), ("genes", "sig value")]


@pytest.mark.parametrize("which", ["fisher", "fisher_multi", "hook"])
@pytest.mark.parametrize("first,second", PAIRS)
def test_two_faults_report_the_earlier_check(which, first, second):
    assert RANK[first] < RANK[second]
    _, ch1, status, word = FAULTS[RANK[first]]
    _, ch2, _, _ = FAULTS[RANK[second]]
    a = apply(apply(good(), ch2), ch1)
    rc, text = call(which, **a)
    assert rc == status and word in text, (rc, text)


def test_a_valid_call_passes_the_checks_and_then_wants_a_context():
    rc, text = call("fisher", **good())
    assert rc == _lib.EINVAL and "null plaidhip_ctx" in text
    a = good()
    rc, text = call("fisher", **{**a, "ov_len": None, "ov_idx": None})
    assert rc == _lib.EINVAL and "null plaidhip_ctx" in text


def test_the_device_list_and_shard_count_come_first():
    a = good()
    fn = _lib.load().plaidhip_fisher_multi
    args = (ptr(a["sig"]), 10, 0, ptr(GP), ptr(GI), 2, ptr(a["out"]), ptr(a["tot"]), None, None)
    assert fn(None, 0, *args) == _lib.EINVAL and "ndev = 0" in _lib.load().plaidhip_last_error_string().decode()
    assert hook("fisher")(0, 0, -1, *args) == _lib.EINVAL
    assert "nshards = 0" in _lib.load().plaidhip_last_error_string().decode()


def test_no_sets_is_the_empty_result():
    """m = 0 returns PLAIDHIP_OK with nothing written, on every entry and without a device, as the other entries do; the
    sig values are still checked"""
    a = good()
    empty = dict(Gp=np.array([0], dtype=np.int32), Gi=None, m=0, out=None, ov_len=None, ov_idx=None)
    for which in ("fisher_multi", "hook"):
        rc, text = call(which, **{**a, **empty})
        assert rc == _lib.OK, text
        assert (a["tot"] == -7).all()
        rc, text = call(which, **{**a, **empty, "sig": bad_sig(a)})
        assert rc == _lib.EINVAL and "sig[14] = 2" in text


def test_check_fisher_args_in_python():
    """engine.check_fisher_args: the same order on what Python can see, and values an int8 cannot hold"""
    assert engine.check_fisher_args([1, 0, -1]).shape == (3, 1)
    s = engine.check_fisher_args(np.array([[1.0, 0.0], [-1.0, 1.0]]))
    assert s.dtype == np.int8 and s.flags.f_contiguous and s.tolist() == [[1, 0], [-1, 1]]
    with pytest.raises(ValueError, match="0 lists"):
        engine.check_fisher_args(np.zeros((4, 0)))
    with pytest.raises(ValueError, match=r"sig\[3\] = 2"):
        engine.check_fisher_args(np.array([[0, 0], [0, 2]]))
    with pytest.raises(ValueError, match=r"sig\[1\] = nan"):
        engine.check_fisher_args(np.array([0.0, np.nan]))
    with pytest.raises(ValueError, match=r"sig\[0\] = 0.5"):
        engine.check_fisher_args(np.array([0.5, 1.0]))
    with pytest.raises(ValueError, match="genes x lists"):
        engine.check_fisher_args(np.zeros((2, 2, 2)))
