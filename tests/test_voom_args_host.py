"""The argument checks of plaid.voom through plaidhip_voom, plaidhip_voom_multi, the sharded test hook and the Python entries,
without a GPU: every fault returns PLAIDHIP_EINVAL and its text before any device is touched (there is none here), in the
order include/plaidhip.h states -- two faults at once report the earlier one."""
import ctypes as C

import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers.sharded_hooks import hook
from tests.test_limma_args_host import ptr

ROWS, N, P = 6, 9, 3


def entries():
    lib = _lib.load()
    return {"voom": (lib.plaidhip_voom, (None,)), "voom_multi": (lib.plaidhip_voom_multi, (None, 2)), "hook": (hook("voom"), (0, 3, -1))}


def good():
    rng = np.random.default_rng(4)
    D = np.asfortranarray(np.column_stack([np.ones(N), np.arange(N) % 2, rng.normal(size=N)]))
    return dict(counts=np.asfortranarray(rng.poisson(20.0, size=(ROWS, N)).astype(np.float64)), rows=ROWS, n=N, design=D, p=P,
                lib=None, span=0.5, E=np.full((ROWS, N), -7.0, order="F"), W=np.full((ROWS, N), -7.0, order="F"),
                lib_out=np.full(N, -7.0), off=np.full(N, -7.0), kx=np.full(engine.VOOM_MAX_KNOTS, -7.0),
                ky=np.full(engine.VOOM_MAX_KNOTS, -7.0), nk=np.full(1, -7, dtype=np.int32))


OUTS = ("E", "W", "lib_out", "off", "kx", "ky", "nk")


def call(which, a):
    fn, head = entries()[which]
    rc = fn(*head, ptr(a["counts"]), a["rows"], a["n"], ptr(a["design"]), a["p"], ptr(a["lib"]), float(a["span"]), ptr(a["E"]),
            ptr(a["W"]), ptr(a["lib_out"]), ptr(a["off"]), ptr(a["kx"]), ptr(a["ky"]), ptr(a["nk"]))
    return rc, _lib.load().plaidhip_last_error_string().decode()


def dup_design(a):
    D = a["design"].copy(order="F")
    D[:, 2] = D[:, 0]
    return D


FAULTS = [   # name, what to change, a word of the text -- in the order of the checks
    ("rows", dict(rows=-1), "bad dims"),
    ("p_zero", dict(p=0), "coefficients"),
    ("p_above", dict(p=33), "1 <= p <= 32"),
    ("span_zero", dict(span=0.0), "span"),
    ("span_nan", dict(span=float("nan")), "span"),
    ("null_design", dict(design=None), "null design"),
    ("null_counts", dict(counts=None), "null counts"),
    ("lib_negative", dict(lib=np.array([1.0] * 8 + [-2.0])), "lib.size[9]"),
    ("design_rank", dict(design="dup"), "voom"),
]


@pytest.mark.parametrize("which", ["voom", "voom_multi", "hook"])
@pytest.mark.parametrize("name,change,word", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_fault_is_einval_with_its_text(which, name, change, word):
    a = good()
    a.update(change)
    if name == "design_rank":
        a["design"] = dup_design(good())
    rc, msg = call(which, a)
    assert rc == _lib.EINVAL, (rc, msg)
    assert word in msg, msg
    assert all((a[k] == -7).all() for k in OUTS)


def test_the_order_of_the_checks():
    for i, (name, change, word) in enumerate(FAULTS):
        for later, lchange, _ in FAULTS[i + 1:]:
            if set(change) & set(lchange):
                continue
            a = good()
            a.update(lchange)
            a.update(change)
            if "dup" in (str(a["design"]),):
                a["design"] = dup_design(good())
            rc, msg = call("voom", a)
            assert rc == _lib.EINVAL and word in msg, (name, later, msg)


def test_a_valid_call_stops_at_the_context_and_empty_calls_write_nothing():
    rc, msg = call("voom", good())
    assert rc == _lib.EINVAL and "null plaidhip_ctx" in msg, msg
    a = good()
    a["lib"], a["span"] = np.full(N, 1e6), 1.0
    assert "null plaidhip_ctx" in call("voom", a)[1]
    for change in (dict(rows=0), dict(n=0)):
        a = good()
        a.update(change)
        rc, msg = call("voom_multi", a)
        assert rc == _lib.OK, msg
        assert all((a[k] == -7).all() for k in OUTS)


def test_python_entries_refuse_before_the_device():
    S = plaid_amd.NamedMatrix(np.ones((3, 6)), ["a", "b", "c"], [f"s{i}" for i in range(6)])
    D = np.column_stack([np.ones(6), np.arange(6) % 2])
    with pytest.raises(ValueError, match="one row per column"):
        plaid_amd.plaid_voom(S, D[:5])
    with pytest.raises(ValueError, match="span"):
        plaid_amd.plaid_voom(S, D, span=0.0)
    with pytest.raises(ValueError, match="one entry per sample"):
        engine._voom(None, (), S.values, D, lib_size=np.ones(5))
    with pytest.raises(plaid_amd.PlaidHipError, match="span"):
        engine.voom_multi(S.values, D, span=2.0, devices=1)
