"""The argument checks of plaid.limma with na = "fit" through plaidhip_limma_na, plaidhip_limma_na_multi, the sharded test hook
and the Python entries, without a GPU: every fault returns PLAIDHIP_EINVAL and its text before any device is touched (there
is none here), in the order include/plaidhip.h states -- two faults at once report the earlier one."""
import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers.sharded_hooks import hook
from tests.test_limma_args_host import good, ptr

NA_MAX = engine.LIMMA_NA_MAX_COEF


def entries():
    lib = _lib.load()
    return {"limma_na": (lib.plaidhip_limma_na, (None,)),                   # (a null context: the checks come first)
            "limma_na_multi": (lib.plaidhip_limma_na_multi, (None, 2)),
            "hook": (hook("limma_na"), (0, 3, -1))}


def good_na():
    a = good()
    a["hyper"] = np.full((a["nfit"], 5), -7.0)
    a["dfres"] = np.full((a["rows"], a["nfit"]), -7.0, order="F")
    a["max_na"] = 0.2
    return a


def call(which, a):
    fn, head = entries()[which]
    rc = fn(*head, ptr(a["A"]), a["rows"], a["n"], ptr(a["design"]), a["p"], a["nfit"], ptr(a["use"]), ptr(a["K"]), a["q"],
            float(a["max_na"]), ptr(a["out"]), ptr(a["hyper"]), ptr(a["dfres"]))
    return rc, _lib.load().plaidhip_last_error_string().decode()


def wide_design(a, p):
    rng = np.random.default_rng(1)
    return np.asfortranarray(rng.normal(size=(a["n"], p, a["nfit"])))


FAULTS = [   # name, what to change, a word of the text -- in the order of the checks
    ("rows", dict(rows=-1), "bad dims"),
    ("p_zero", dict(p=0), "coefficients"),
    ("p_above_all", dict(p=33), "1 <= p <= 32"),
    ("p_above_na", dict(p=NA_MAX + 1), 'with na = "fit"'),
    ("max_na_negative", dict(max_na=-0.01), "max_na"),
    ("max_na_above_one", dict(max_na=1.5), "max_na"),
    ("max_na_nan", dict(max_na=float("nan")), "max_na"),
    ("q_without_K", dict(K=None, q=2), "without K"),
    ("null_design", dict(design=None), "null design"),
    ("null_A", dict(A=None), "null A"),
    ("null_dfres", dict(dfres=None), "null dfres"),
]


@pytest.mark.parametrize("which", ["limma_na", "limma_na_multi", "hook"])
@pytest.mark.parametrize("name,change,word", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_fault_is_einval_with_its_text(which, name, change, word):
    a = good_na()
    a.update(change)
    if name == "p_above_na":
        a["design"] = wide_design(a, NA_MAX + 1)
    rc, msg = call(which, a)
    assert rc == _lib.EINVAL, (rc, msg)
    assert word in msg, msg
    assert (a["out"] == -7.0).all() and (a["hyper"] == -7.0).all()
    assert a["dfres"] is None or (a["dfres"] == -7.0).all()


def test_the_order_of_the_checks():
    """each fault with every later one at once: the earlier one is reported"""
    for i, (name, change, word) in enumerate(FAULTS):
        for later, lchange, _ in FAULTS[i + 1:]:
            if set(change) & set(lchange):
                continue
            a = good_na()
            a.update(lchange)
            a.update(change)
            if name == "p_above_na":
                a["design"] = wide_design(a, NA_MAX + 1)
            rc, msg = call("limma_na", a)
            assert rc == _lib.EINVAL and word in msg, (name, later, msg)


def test_a_valid_call_passes_the_checks_and_stops_at_the_context():
    rc, msg = call("limma_na", good_na())
    assert rc == _lib.EINVAL and "null plaidhip_ctx" in msg, msg
    a = good_na()
    a["max_na"] = 0.0
    assert "null plaidhip_ctx" in call("limma_na", a)[1]
    a["max_na"] = 1.0
    assert "null plaidhip_ctx" in call("limma_na", a)[1]
    a["p"], a["design"] = NA_MAX, wide_design(a, NA_MAX)    # (9 samples for 10 coefficients: the fit's own check, later)
    a["K"], a["q"] = None, NA_MAX
    assert "samples for" in call("limma_na", a)[1]


def test_empty_calls_write_nothing():
    for change in (dict(rows=0), dict(nfit=0), dict(q=0, K=np.zeros((3, 0), order="F"))):
        a = good_na()
        a.update(change)
        rc, msg = call("limma_na_multi", a)
        assert rc == _lib.OK, msg
        assert (a["out"] == -7.0).all() and (a["hyper"] == -7.0).all() and (a["dfres"] == -7.0).all()


def test_the_host_entries_check_their_arguments():
    lib = _lib.load()
    one = np.ones(4)
    ok = np.zeros(1, dtype=np.int32)
    rc = lib.plaidhip_limma_na_solve(NA_MAX + 1, 0, None, ptr(one), 5, None, 0, ptr(one), None, None, ptr(ok))
    assert rc == _lib.EINVAL and "coefficients" in lib.plaidhip_last_error_string().decode()
    rc = lib.plaidhip_limma_na_solve(2, 1, None, ptr(one), 5, None, 0, ptr(one), None, None, ptr(ok))
    assert rc == _lib.EINVAL and "null argument" in lib.plaidhip_last_error_string().decode()
    rc = lib.plaidhip_limma_finish_na(3, 2, 1, 1, ptr(one), ptr(one), ptr(one), ptr(one), None, None, ptr(one), ptr(one))
    assert rc == _lib.EINVAL and "limma_finish_na: null argument" in lib.plaidhip_last_error_string().decode()


def test_python_entries_refuse_before_the_device():
    S = plaid_amd.NamedMatrix(np.ones((3, 6)), ["a", "b", "c"], [f"s{i}" for i in range(6)])
    D = np.column_stack([np.ones(6), np.arange(6) % 2])
    with pytest.raises(ValueError, match="na must be one of"):
        engine._limma_any(None, None, (), S.values, D, None, None, "drop", 0.2)
    with pytest.raises(plaid_amd.PlaidHipError, match="max_na"):
        engine.limma_multi(S.values, D, devices=1, na="fit", max_na=2.0)
    import inspect
    for fn in (plaid_amd.plaid_limma, plaid_amd.plaid_limma_contrasts, plaid_amd.Context.limma, engine.limma_multi):
        sig = inspect.signature(fn).parameters
        assert sig["na"].default == "propagate" and sig["max_na"].default == 0.2
