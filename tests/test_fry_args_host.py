"""The argument checks of plaid.fry through plaidhip_fry, plaidhip_fry_multi, the sharded test hook and the Python entries,
without a GPU: every fault returns PLAIDHIP_EINVAL and its text before any device is touched (there is none here), in the
order include/plaidhip.h states -- plaid.limma's checks under the name "fry:", then the membership's as plaid.camera makes
them, then standardize, then the number of contrasts; two faults at once report the earlier one."""
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
    return {"fry": (lib.plaidhip_fry, (None,)),                            # (a null context: the checks come first)
            "fry_multi": (lib.plaidhip_fry_multi, (None, 2)),
            "hook": (hook("fry"), (0, 3, -1))}


def good_fry():
    a = good()
    a["Gp"] = np.array([0, 2, 2, 5], dtype=np.int32)
    a["Gi"] = np.array([0, 3, 1, 2, 4], dtype=np.int32)
    a["m"] = M
    a["std"] = 0
    a["out"] = np.full((M, 7, a["q"], a["nfit"]), -7.0, order="F")
    a["hyper"] = np.full((a["nfit"], 7), -7.0)
    return a


def call(which, a):
    fn, head = entries()[which]
    rc = fn(*head, ptr(a["A"]), a["rows"], a["n"], ptr(a["design"]), a["p"], a["nfit"], ptr(a["use"]), ptr(a["K"]), a["q"],
            ptr(a["Gp"]), ptr(a["Gi"]), a["m"], int(a["std"]), ptr(a["out"]), ptr(a["hyper"]))
    return rc, _lib.load().plaidhip_last_error_string().decode()


OWN_FAULTS = [
    ("standardize 3", dict(std=3), _lib.EINVAL, "standardize = 3"),
    ("standardize -1", dict(std=-1), _lib.EINVAL, "standardize = -1"),
]
FAULTS = ([("m", dict(m=-1), _lib.EINVAL, "bad dims m=-1")] + list(LIMMA_FAULTS) +
          [f for f in SET_FAULTS if not f[0].startswith("rho")] + OWN_FAULTS)
WHICH = ["fry", "fry_multi", "hook"]


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name,change,status,word", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_fault_is_refused_with_its_text(which, name, change, status, word):
    a = faulty(good_fry(), change)
    rc, msg = call(which, a)
    assert rc == status, (rc, msg)
    assert word in msg, msg
    assert msg.startswith("fry:"), msg
    out, hyper = good_fry()["out"], good_fry()["hyper"]
    assert a["out"] is None or (a["out"] == out).all()
    assert a["hyper"] is None or (a["hyper"] == hyper).all()


def test_the_order_of_the_checks():
    for i, (name, change, status, word) in enumerate(FAULTS):
        for later, lchange, _, _ in FAULTS[i + 1:]:
            a0 = good_fry()
            first, second = (change(a0) if callable(change) and not isinstance(change, dict) else change,
                             lchange(a0) if callable(lchange) and not isinstance(lchange, dict) else lchange)
            if set(first) & set(second):
                continue
            a = apply(apply(a0, second), first)
            rc, msg = call("fry", a)
            assert rc == status and word in msg, (name, later, msg)


def test_too_many_contrasts_are_refused():
    a = good_fry()
    q = 33
    K = np.asfortranarray(np.random.default_rng(0).normal(size=(a["p"], q)))
    a = apply(a, dict(K=K, q=q, out=np.full((M, 7, q, a["nfit"]), -7.0, order="F")))
    rc, msg = call("fry", a)
    assert rc == _lib.EINVAL and "q = 33 contrasts (at most 32)" in msg, msg


def test_a_valid_call_passes_the_checks_and_stops_at_the_context():
    for std in (0, 1, 2):
        a = good_fry()
        a["std"] = std
        rc, msg = call("fry", a)
        assert rc == _lib.EINVAL and "null plaidhip_ctx" in msg, msg


def test_empty_calls_write_nothing():
    for change in (dict(rows=0, Gp=gp([0, 0, 0, 0])), dict(nfit=0), dict(q=0, K=np.zeros((3, 0), order="F")),
                   dict(m=0, Gp=gp([0]))):
        a = apply(good_fry(), change)
        rc, msg = call("fry_multi", a)
        assert rc == _lib.OK, msg
        assert (a["out"] == -7.0).all() and (a["hyper"] == -7.0).all()


def test_the_host_entries_check_their_arguments():
    lib = _lib.load()
    one = np.ones(8)
    nf = np.array([5], dtype=np.int64)

    def err():
        return lib.plaidhip_last_error_string().decode()
    assert lib.plaidhip_fry_residual_row(4, 0, ptr(one), ptr(one), None, ptr(one), 1.0, ptr(one)) == _lib.EINVAL
    assert "coefficients" in err()
    assert lib.plaidhip_fry_residual_row(4, 1, None, ptr(one), None, ptr(one), 1.0, ptr(one)) == _lib.EINVAL
    assert "null argument" in err()
    assert lib.plaidhip_fry_divisors(4, 1, 1, ptr(one), ptr(nf), 3, ptr(one)) == _lib.EINVAL
    assert "standardize = 3" in err()
    assert lib.plaidhip_fry_divisors(4, 5, 1, ptr(one), ptr(nf), 0, ptr(one)) == _lib.EINVAL
    assert "fit 1 has 5 samples for 5 coefficients" in err()
    assert lib.plaidhip_fry_q2(ptr(one), 4, 1, None, 1, None, None) == _lib.EINVAL
    assert "null Q2" in err()
    args = (2, 1, 1, ptr(one), ptr(one), ptr(one), ptr(one))
    ok = np.ones(1, dtype=np.int8)
    assert lib.plaidhip_fry_finish(*args, None, None, None, None, None, ptr(ok), ptr(one)) == _lib.EINVAL
    assert "mixed test" in err()
    assert lib.plaidhip_fry_finish(*args, None, None, None, None, None, None, None) == _lib.EINVAL
    assert "null argument" in err()
    assert lib.plaidhip_fry_finish(2, 1, 1, ptr(np.zeros(1)), *args[4:], None, None, None, None, None, None, ptr(one)) == _lib.EINVAL
    assert "df.residual = 0" in err()
    assert lib.plaidhip_fry_finish(-1, 1, 1, *args[3:], None, None, None, None, None, None, ptr(one)) == _lib.EINVAL
    assert "bad dims" in err()


def test_python_entries_refuse_before_the_device():
    X = plaid_amd.NamedMatrix(np.arange(24.0).reshape(4, 6), list("abcd"), [f"s{i}" for i in range(6)])
    D = np.column_stack([np.ones(6), np.arange(6) % 2])
    G = {"s1": ["a", "b"], "s2": ["b", "c", "d"]}
    with pytest.raises(ValueError, match="standardize"):
        plaid_amd.plaid_fry(X, D, G, standardize="p2")
    with pytest.raises(ValueError, match="sort_by"):
        plaid_amd.plaid_fry(X, D, G, sort_by="PValue")
    with pytest.raises(ValueError, match="sort_by"):
        plaid_amd.plaid_fry_contrasts(X, np.arange(6) % 2, G, sort_by="size")
    with pytest.raises(ValueError, match="0, 1 or NA"):
        plaid_amd.plaid_fry_contrasts(X, np.arange(6) % 3, G)
    with pytest.raises(plaid_amd.PlaidHipError, match="fry: fit 1 has 2 samples"):
        engine.fry_multi(X.values[:, :2], D[:2], [0, 2], [0, 1], devices=1)
    import inspect
    for fn in (plaid_amd.plaid_fry, plaid_amd.plaid_fry_contrasts, plaid_amd.Context.fry, engine.fry_multi):
        assert inspect.signature(fn).parameters["standardize"].default == "posterior.sd"
    assert inspect.signature(plaid_amd.plaid_fry).parameters["sort_by"].default == "directional"
