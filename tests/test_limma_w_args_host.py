"""The argument checks of plaid.limma with weights through plaidhip_limma_w, plaidhip_limma_w_multi, the sharded test hook and
the Python entries, without a GPU: every fault returns PLAIDHIP_EINVAL and its text before any device is touched (there is
none here), in the order include/plaidhip.h states -- two faults at once report the earlier one."""
import inspect

import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers.sharded_hooks import hook
from tests.test_limma_args_host import good, ptr

NA_MAX = engine.LIMMA_NA_MAX_COEF


def entries():
    lib = _lib.load()
    return {"limma_w": (lib.plaidhip_limma_w, (None,)),                     # (a null context: the checks come first)
            "limma_w_multi": (lib.plaidhip_limma_w_multi, (None, 2)),
            "hook": (hook("limma_w"), (0, 3, -1))}


def good_w():
    a = good()
    a["hyper"] = np.full((a["nfit"], 5), -7.0)
    a["dfres"] = np.full((a["rows"], a["nfit"]), -7.0, order="F")
    a["max_na"] = 0.2
    a["Wt"] = np.asfortranarray(np.full((a["rows"], a["n"]), 2.0))
    a["aw"] = np.full(a["n"], 0.5)
    return a


def call(which, a):
    fn, head = entries()[which]
    rc = fn(*head, ptr(a["A"]), ptr(a["Wt"]), ptr(a["aw"]), a["rows"], a["n"], ptr(a["design"]), a["p"], a["nfit"], ptr(a["use"]),
            ptr(a["K"]), a["q"], float(a["max_na"]), ptr(a["out"]), ptr(a["hyper"]), ptr(a["dfres"]))
    return rc, _lib.load().plaidhip_last_error_string().decode()


def wide_design(a, p):
    rng = np.random.default_rng(1)
    return np.asfortranarray(rng.normal(size=(a["n"], p, a["nfit"])))


FAULTS = [   # name, what to change, a word of the text -- in the order of the checks
    ("rows", dict(rows=-1), "bad dims"),
    ("p_zero", dict(p=0), "coefficients"),
    ("p_above_all", dict(p=33), "1 <= p <= 32"),
    ("p_above_w", dict(p=NA_MAX + 1), "with weights"),
    ("max_na_negative", dict(max_na=-0.01), "max_na"),
    ("max_na_nan", dict(max_na=float("nan")), "max_na"),
    ("no_weights", dict(Wt=None, aw=None), "both null"),
    ("q_without_K", dict(K=None, q=2), "without K"),
    ("null_design", dict(design=None), "null design"),
    ("null_A", dict(A=None), "null A"),
    ("null_dfres", dict(dfres=None), "null dfres"),
]


@pytest.mark.parametrize("which", ["limma_w", "limma_w_multi", "hook"])
@pytest.mark.parametrize("name,change,word", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_fault_is_einval_with_its_text(which, name, change, word):
    a = good_w()
    a.update(change)
    if name == "p_above_w":
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
            a = good_w()
            a.update(lchange)
            a.update(change)
            if name == "p_above_w":
                a["design"] = wide_design(a, NA_MAX + 1)
            rc, msg = call("limma_w", a)
            assert rc == _lib.EINVAL and word in msg, (name, later, msg)


def test_a_valid_call_passes_the_checks_and_stops_at_the_context():
    for change in (dict(), dict(Wt=None), dict(aw=None), dict(max_na=0.0), dict(max_na=1.0)):
        a = good_w()
        a.update(change)
        rc, msg = call("limma_w", a)
        assert rc == _lib.EINVAL and "null plaidhip_ctx" in msg, (change, msg)
    a = good_w()                                            # the entries of the weights are not checked: they are data
    a["Wt"][0, 0], a["Wt"][1, 1], a["aw"][2] = np.nan, -1.0, np.inf
    assert "null plaidhip_ctx" in call("limma_w", a)[1]


def test_empty_calls_write_nothing():
    for change in (dict(rows=0), dict(nfit=0), dict(q=0, K=np.zeros((3, 0), order="F"))):
        a = good_w()
        a.update(change)
        rc, msg = call("limma_w_multi", a)
        assert rc == _lib.OK, msg
        assert (a["out"] == -7.0).all() and (a["hyper"] == -7.0).all() and (a["dfres"] == -7.0).all()


def test_the_host_solve_checks_its_arguments():
    lib = _lib.load()
    one = np.ones(4)
    ok = np.zeros(1, dtype=np.int32)
    rc = lib.plaidhip_limma_w_solve(NA_MAX + 1, ptr(one), ptr(one), 5, None, 0, ptr(one), None, None, ptr(ok))
    assert rc == _lib.EINVAL and "coefficients" in lib.plaidhip_last_error_string().decode()
    rc = lib.plaidhip_limma_w_solve(2, None, ptr(one), 5, None, 0, ptr(one), None, None, ptr(ok))
    assert rc == _lib.EINVAL and "null argument" in lib.plaidhip_last_error_string().decode()
    rc = lib.plaidhip_limma_w_solve(2, ptr(one), ptr(one), -1, None, 0, ptr(one), None, None, ptr(ok))
    assert rc == _lib.EINVAL and "bad dims" in lib.plaidhip_last_error_string().decode()


def test_python_entries_refuse_before_the_device():
    S = plaid_amd.NamedMatrix(np.ones((3, 6)), ["a", "b", "c"], [f"s{i}" for i in range(6)])
    D = np.column_stack([np.ones(6), np.arange(6) % 2])
    with pytest.raises(ValueError, match="shape of the matrix"):
        engine.limma_weights(3, 6, np.ones((3, 5)))
    with pytest.raises(ValueError, match="one entry per sample"):
        engine.limma_weights(3, 6, np.ones(5))
    with pytest.raises(ValueError, match="shape of S"):
        plaid_amd.plaid_limma(S, D, weights=np.ones((2, 6)))
    with pytest.raises(ValueError, match="one entry per sample"):
        plaid_amd.plaid_limma(S, D, weights=np.ones(4))
    with pytest.raises(plaid_amd.PlaidHipError, match="max_na"):
        engine.limma_multi(S.values, D, devices=1, na="fit", max_na=2.0, weights=np.ones(6))
    Wt, aw = engine.limma_weights(3, 6, (np.ones((3, 6)), np.ones(6)))
    assert Wt.flags.f_contiguous and Wt.shape == (3, 6) and aw.shape == (6,)
    assert engine.limma_weights(3, 6, np.ones(6))[0] is None and engine.limma_weights(3, 6, np.ones((3, 6)))[1] is None
    for fn in (plaid_amd.plaid_limma, plaid_amd.plaid_limma_contrasts, plaid_amd.Context.limma, engine.limma_multi):
        assert inspect.signature(fn).parameters["weights"].default is None
