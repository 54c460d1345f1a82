"""The argument checks of plaid.camera through plaidhip_camera, plaidhip_camera_multi, the sharded test hook and the Python
entries, without a GPU: every fault returns PLAIDHIP_EINVAL and its text before any device is touched (there is none here),
in the order include/plaidhip.h states -- plaid.limma's checks under the name "camera:", then the membership's, then the
fixed correlation; two faults at once report the earlier one."""
import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers.sharded_hooks import hook
from tests.test_limma_args_host import FAULTS as LIMMA_FAULTS
from tests.test_limma_args_host import apply, good, ptr

M = 3


def entries():
    lib = _lib.load()
    return {"camera": (lib.plaidhip_camera, (None,)),                      # (a null context: the checks come first)
            "camera_multi": (lib.plaidhip_camera_multi, (None, 2)),
            "hook": (hook("camera"), (0, 3, -1))}


def good_camera():
    a = good()
    a["Gp"] = np.array([0, 2, 2, 5], dtype=np.int32)
    a["Gi"] = np.array([0, 3, 1, 2, 4], dtype=np.int32)
    a["m"] = M
    a["rho"] = 0.01
    a["out"] = np.full((M, 8, a["q"], a["nfit"]), -7.0, order="F")
    a["hyper"] = np.full((a["nfit"], 6), -7.0)
    return a


def call(which, a):
    fn, head = entries()[which]
    rc = fn(*head, ptr(a["A"]), a["rows"], a["n"], ptr(a["design"]), a["p"], a["nfit"], ptr(a["use"]), ptr(a["K"]), a["q"],
            ptr(a["Gp"]), ptr(a["Gi"]), a["m"], float(a["rho"]), 0, ptr(a["out"]), ptr(a["hyper"]))
    return rc, _lib.load().plaidhip_last_error_string().decode()


def gp(values):
    return np.array(values, dtype=np.int32)


SET_FAULTS = [   # after plaid.limma's, in the order of the checks
    ("null Gp", dict(Gp=None), _lib.EINVAL, "null Gp"),
    ("Gp start", dict(Gp=gp([1, 2, 2, 5])), _lib.EINVAL, "Gp[0] = 1"),
    ("Gp decreasing", dict(Gp=gp([0, 2, 1, 5])), _lib.EINVAL, "Gp[2] = 1 after 2"),
    ("set above g", lambda a: dict(Gp=gp([0, 2, 2, 2 + a["rows"] + 1]), Gi=np.zeros(3 + a["rows"], dtype=np.int32)), _lib.EINVAL,
     "members (at most the"),
    ("null Gi", dict(Gi=None), _lib.EINVAL, "null Gi"),
    ("Gi range", lambda a: dict(Gi=gp([0, 3, 1, a["rows"], 4])), _lib.EINVAL, "Gi[3] ="),
    ("Gi negative", dict(Gi=gp([0, -1, 1, 2, 4])), _lib.EINVAL, "Gi[1] = -1"),
    ("rho = 1", dict(rho=1.0), _lib.EINVAL, "inter_gene_cor = 1"),
    ("rho = -1", dict(rho=-1.0), _lib.EINVAL, "inter_gene_cor = -1"),
    ("rho inf", dict(rho=np.inf), _lib.EINVAL, "inter_gene_cor = inf"),
]
FAULTS = [("m", dict(m=-1), _lib.EINVAL, "bad dims m=-1")] + list(LIMMA_FAULTS) + SET_FAULTS
WHICH = ["camera", "camera_multi", "hook"]


def faulty(a, change):
    return apply(a, change(a) if callable(change) and not isinstance(change, dict) else change)


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name,change,status,word", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_fault_is_refused_with_its_text(which, name, change, status, word):
    a = faulty(good_camera(), change)
    rc, msg = call(which, a)
    assert rc == status, (rc, msg)
    assert word in msg, msg
    assert msg.startswith("camera:"), msg                   # (plaid.limma's checks speak under this entry's name)
    out, hyper = good_camera()["out"], good_camera()["hyper"]
    assert a["out"] is None or (a["out"] == out).all()
    assert a["hyper"] is None or (a["hyper"] == hyper).all()


def test_the_order_of_the_checks():
    """each fault with every later one at once: the earlier one is reported"""
    for i, (name, change, status, word) in enumerate(FAULTS):
        for later, lchange, _, _ in FAULTS[i + 1:]:
            a0 = good_camera()
            first, second = (change(a0) if callable(change) and not isinstance(change, dict) else change,
                             lchange(a0) if callable(lchange) and not isinstance(lchange, dict) else lchange)
            if set(first) & set(second):
                continue
            a = apply(apply(a0, second), first)
            rc, msg = call("camera", a)
            assert rc == status and word in msg, (name, later, msg)


def test_a_valid_call_passes_the_checks_and_stops_at_the_context():
    rc, msg = call("camera", good_camera())
    assert rc == _lib.EINVAL and "null plaidhip_ctx" in msg, msg
    for rho in (np.nan, 0.0, -0.999, 0.999):                  # NaN asks for the estimate
        a = good_camera()
        a["rho"] = rho
        assert "null plaidhip_ctx" in call("camera", a)[1]


def test_empty_calls_write_nothing():
    for change in (dict(rows=0, Gp=gp([0, 0, 0, 0])), dict(nfit=0), dict(q=0, K=np.zeros((3, 0), order="F")),
                   dict(m=0, Gp=gp([0]))):
        a = apply(good_camera(), change)
        rc, msg = call("camera_multi", a)
        assert rc == _lib.OK, msg
        assert (a["out"] == -7.0).all() and (a["hyper"] == -7.0).all()


def test_the_host_entries_check_their_arguments():
    lib = _lib.load()
    one = np.ones(8)
    ok = np.ones(8, dtype=np.int8)

    def err():
        return lib.plaidhip_last_error_string().decode()
    assert lib.plaidhip_camera_residual_row(4, 0, ptr(one), ptr(one), None, ptr(one), 1.0, 2.0, ptr(one)) == _lib.EINVAL
    assert "coefficients" in err()
    assert lib.plaidhip_camera_residual_row(4, 1, ptr(one), ptr(one), None, ptr(one), 1.0, 0.0, ptr(one)) == _lib.EINVAL
    assert "residual degrees of freedom" in err()
    assert lib.plaidhip_camera_residual_row(4, 1, None, ptr(one), None, ptr(one), 1.0, 2.0, ptr(one)) == _lib.EINVAL
    assert "null argument" in err()
    args = (4, 2, 1, 1, ptr(one), ptr(ok), ptr(one), ptr(one))
    assert lib.plaidhip_camera_finish(*args, None, ptr(one), ptr(one), float("nan"), 0, ptr(one), ptr(one)) == _lib.EINVAL
    assert "without sums of squares" in err()
    assert lib.plaidhip_camera_finish(*args, None, ptr(one), ptr(one), 1.0, 0, ptr(one), ptr(one)) == _lib.EINVAL
    assert "without sums of squares" in err()
    assert lib.plaidhip_camera_finish(*args, ptr(one), ptr(np.zeros(1)), ptr(one), 0.0, 0, ptr(one), ptr(one)) == _lib.EINVAL
    assert "df.residual = 0" in err()
    assert lib.plaidhip_camera_finish(*args, ptr(one), ptr(one), ptr(one), 0.0, 0, None, ptr(one)) == _lib.EINVAL
    assert "null argument" in err()
    assert lib.plaidhip_camera_finish(-1, 2, 1, 1, *args[4:], ptr(one), ptr(one), ptr(one), 0.0, 0, ptr(one), ptr(one)) == _lib.EINVAL
    assert "bad dims" in err()


def test_python_entries_refuse_before_the_device():
    X = plaid_amd.NamedMatrix(np.arange(24.0).reshape(4, 6), list("abcd"), [f"s{i}" for i in range(6)])
    D = np.column_stack([np.ones(6), np.arange(6) % 2])
    G = {"s1": ["a", "b"], "s2": ["b", "c", "d"]}
    with pytest.raises(ValueError, match="inter_gene_cor"):
        plaid_amd.plaid_camera(X, D, G, inter_gene_cor=1.0)
    with pytest.raises(ValueError, match="sort_by"):
        plaid_amd.plaid_camera(X, D, G, sort_by="size")
    with pytest.raises(ValueError, match="sort_by"):
        plaid_amd.plaid_camera_contrasts(X, np.arange(6) % 2, G, sort_by="size")
    with pytest.raises(ValueError, match="0, 1 or NA"):
        plaid_amd.plaid_camera_contrasts(X, np.arange(6) % 3, G)
    with pytest.raises(plaid_amd.PlaidHipError, match="camera: fit 1 has 2 samples"):
        engine.camera_multi(X.values[:, :2], D[:2], [0, 2], [0, 1], devices=1)
    import inspect
    for fn in (plaid_amd.plaid_camera, plaid_amd.plaid_camera_contrasts, plaid_amd.Context.camera, engine.camera_multi):
        sig = inspect.signature(fn).parameters
        assert sig["inter_gene_cor"].default == 0.01 and sig["allow_neg_cor"].default is False
    assert inspect.signature(plaid_amd.plaid_camera).parameters["sort_by"].default == "PValue"
