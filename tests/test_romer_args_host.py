"""The argument checks of plaid.romer through plaidhip_romer, plaidhip_romer_multi, the sharded test hook and the Python
entries, without a GPU: every fault returns its status and its text before any device is touched (there is none here), in
the order include/plaidhip.h states -- plaid.limma's checks under the name "romer:", then the membership's as plaid.camera
makes them, then the set statistic, nrot < 1, nrot above the maximum and more genes than PLAIDHIP_ROMER_MAX_GENES; two faults
at once report the earlier one."""
import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers.sharded_hooks import hook
from tests.test_camera_args_host import SET_FAULTS, faulty, gp
from tests.test_limma_args_host import FAULTS as LIMMA_FAULTS
from tests.test_limma_args_host import apply, good, ptr

M = 3


def entries():
    lib = _lib.load()
    return {"romer": (lib.plaidhip_romer, (None,)),                        # (a null context: the checks come first)
            "romer_multi": (lib.plaidhip_romer_multi, (None, 2)),
            "hook": (hook("romer"), (0, 3, -1))}


def good_romer():
    a = good()
    a["Gp"] = np.array([0, 2, 2, 5], dtype=np.int32)
    a["Gi"] = np.array([0, 3, 1, 2, 4], dtype=np.int32)
    a["m"] = M
    a["stat"], a["nrot"] = 0, 99
    a["out"] = np.full((M, 7, a["q"], a["nfit"]), -7.0, order="F")
    a["hyper"] = np.full((a["nfit"], 8 + a["q"]), -7.0)
    return a


def call(which, a):
    fn, head = entries()[which]
    rc = fn(*head, ptr(a["A"]), a["rows"], a["n"], ptr(a["design"]), a["p"], a["nfit"], ptr(a["use"]), ptr(a["K"]), a["q"],
            ptr(a["Gp"]), ptr(a["Gi"]), a["m"], int(a["stat"]), int(a["nrot"]), 1, 1, None, None, ptr(a["out"]), ptr(a["hyper"]))
    return rc, _lib.load().plaidhip_last_error_string().decode()


OWN_FAULTS = [
    ("set_statistic 3", dict(stat=3), _lib.EINVAL, "set_statistic = 3"),
    ("set_statistic -1", dict(stat=-1), _lib.EINVAL, "set_statistic = -1"),
    ("nrot 0", dict(nrot=0), _lib.EINVAL, "nrot = 0 rotations (at least 1)"),
    ("nrot max", dict(nrot=(1 << 20) + 1), _lib.EINVAL, "nrot = 1048577 rotations (at most 1048576)"),
]
FAULTS = ([("m", dict(m=-1), _lib.EINVAL, "bad dims m=-1")] + list(LIMMA_FAULTS) +
          [f for f in SET_FAULTS if not f[0].startswith("rho")] + OWN_FAULTS)
WHICH = ["romer", "romer_multi", "hook"]


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name,change,status,word", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_fault_is_refused_with_its_text(which, name, change, status, word):
    a = faulty(good_romer(), change)
    rc, msg = call(which, a)
    assert rc == status, (rc, msg)
    assert word in msg, msg
    assert msg.startswith("romer:"), msg
    out, hyper = good_romer()["out"], good_romer()["hyper"]
    assert a["out"] is None or (a["out"] == out).all()
    assert a["hyper"] is None or (a["hyper"] == hyper).all()


def test_the_order_of_the_checks():
    for i, (name, change, status, word) in enumerate(FAULTS):
        for later, lchange, _, _ in FAULTS[i + 1:]:
            a0 = good_romer()
            first, second = (change(a0) if callable(change) and not isinstance(change, dict) else change,
                             lchange(a0) if callable(lchange) and not isinstance(lchange, dict) else lchange)
            if set(first) & set(second):
                continue
            a = apply(apply(a0, second), first)
            rc, msg = call("romer", a)
            assert rc == status and word in msg, (name, later, msg)


def test_a_valid_call_passes_the_checks_and_stops_at_the_context():
    for stat in range(3):
        a = good_romer()
        a["stat"] = stat
        rc, msg = call("romer", a)
        assert rc == _lib.EINVAL and "null plaidhip_ctx" in msg, msg


def test_empty_calls_write_nothing():
    for change in (dict(rows=0, Gp=gp([0, 0, 0, 0])), dict(nfit=0), dict(q=0, K=np.zeros((3, 0), order="F")),
                   dict(m=0, Gp=gp([0]))):
        a = apply(good_romer(), change)
        rc, msg = call("romer_multi", a)
        assert rc == _lib.OK, msg
        assert (a["out"] == -7.0).all() and (a["hyper"] == -7.0).all()


def test_the_host_entries_check_their_arguments():
    lib = _lib.load()
    one = np.ones(8)
    cnt = np.zeros(8, dtype=np.int32)

    def err():
        return lib.plaidhip_last_error_string().decode()
    assert lib.plaidhip_romer_finish(2, 1, 1, 9, 3, ptr(cnt), ptr(one), ptr(one)) == _lib.EINVAL
    assert "set_statistic = 3" in err()
    assert lib.plaidhip_romer_finish(2, 1, 1, 0, 0, ptr(cnt), ptr(one), ptr(one)) == _lib.EINVAL
    assert "nrot = 0" in err()
    assert lib.plaidhip_romer_finish(2, 1, 1, 9, 0, None, ptr(one), ptr(one)) == _lib.EINVAL
    assert "null argument" in err()
    assert lib.plaidhip_romer_finish(-1, 1, 1, 9, 0, ptr(cnt), ptr(one), ptr(one)) == _lib.EINVAL
    assert "bad dims" in err()
    assert lib.plaidhip_romer_shrink(4, ptr(one), 0.0, 1.0, 5.0, ptr(one), ptr(one)) == _lib.EINVAL
    assert "stdev.unscaled" in err()
    assert lib.plaidhip_romer_shrink(4, ptr(one), 1.0, 1.0, 0.0, ptr(one), ptr(one)) == _lib.EINVAL
    assert "df.total" in err()
    assert lib.plaidhip_romer_shrink(4, None, 1.0, 1.0, 5.0, ptr(one), ptr(one)) == _lib.EINVAL
    assert "null argument" in err()
    # the device entries refuse a null context before anything else
    assert lib.plaidhip_dev_romer_keys(None, None, 8, None, 4, 4, 0, 9, 0, None, None, None, None) == _lib.EINVAL
    assert lib.plaidhip_dev_romer_sides(None, None, None, None, 4, 4, None, None, 2, 0, 9, 0, None, None, None) == _lib.EINVAL


def test_python_entries_refuse_before_the_device():
    X = plaid_amd.NamedMatrix(np.arange(24.0).reshape(4, 6), list("abcd"), [f"s{i}" for i in range(6)])
    D = np.column_stack([np.ones(6), np.arange(6) % 2])
    G = {"s1": ["a", "b"], "s2": ["b", "c", "d"]}
    with pytest.raises(ValueError, match="set_statistic"):
        plaid_amd.plaid_romer(X, D, G, set_statistic="msq")
    with pytest.raises(ValueError, match="sort_by"):
        plaid_amd.plaid_romer(X, D, G, sort_by="PValue")
    with pytest.raises(ValueError, match="sort_by"):
        plaid_amd.plaid_romer_contrasts(X, np.arange(6) % 2, G, sort_by="size")
    with pytest.raises(ValueError, match="0, 1 or NA"):
        plaid_amd.plaid_romer_contrasts(X, np.arange(6) % 3, G)
    with pytest.raises(ValueError, match="rotations"):
        engine.romer_multi(X.values, D, [0, 2], [0, 1], rotations=np.zeros((6, 5)), devices=1)
    with pytest.raises(ValueError, match="shrink"):
        engine.romer_multi(X.values, D, [0, 2], [0, 1], shrink=np.ones(3), devices=1)
    with pytest.raises(plaid_amd.PlaidHipError, match="romer: fit 1 has 2 samples"):
        engine.romer_multi(X.values[:, :2], D[:2], [0, 2], [0, 1], devices=1)
    import inspect
    for fn in (plaid_amd.plaid_romer, plaid_amd.plaid_romer_contrasts, plaid_amd.Context.romer, engine.romer_multi):
        par = inspect.signature(fn).parameters
        assert (par["set_statistic"].default, par["nrot"].default, par["seed"].default, par["shrink_resid"].default,
                par["rotations"].default) == ("mean", 9999, 1, True, None)
