"""The argument checks of plaid.limma (multi.cpp: check_limma_call) through plaidhip_limma, plaidhip_limma_multi, the sharded
test hook and the Python entries, without a GPU: every fault returns its status and text before any device is touched (there
is none here), and the checks run in the order include/plaidhip.h states -- two faults at once report the earlier one."""
import numpy as np
import pytest
import scipy.sparse as sp

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers.sharded_hooks import hook

ROWS, N, P, NFIT, Q = 6, 9, 3, 2, 2


def entries():
    lib = _lib.load()
    return {"limma": (lib.plaidhip_limma, (None,)),                        # (a null context: the checks come first)
            "limma_multi": (lib.plaidhip_limma_multi, (None, 2)),
            "hook": (hook("limma"), (0, 3, -1))}


def ptr(a):
    return None if a is None else a.ctypes.data


def call(which, A, rows, n, design, p, nfit, use, K, q, out, hyper):
    fn, head = entries()[which]
    rc = fn(*head, ptr(A), rows, n, ptr(design), p, nfit, ptr(use), ptr(K), q, ptr(out), ptr(hyper))
    return rc, _lib.load().plaidhip_last_error_string().decode()


def good():
    """a valid call's arguments, the outputs holding -7: two fits of [1, group, covariate], the second without sample 3"""
    rng = np.random.default_rng(3)
    D = np.empty((N, P, NFIT), order="F")
    for f in range(NFIT):
        D[:, 0, f], D[:, 1, f], D[:, 2, f] = 1.0, (np.arange(N) + f) % 2, rng.normal(size=N)
    use = np.ones((N, NFIT), dtype=np.int8, order="F")
    use[2, 1] = 0
    K = np.asfortranarray([[0.0, 0.0], [1.0, 1.0], [0.0, -1.0]])
    return dict(A=np.asfortranarray(rng.normal(size=(ROWS, N))), rows=ROWS, n=N, design=D, p=P, nfit=NFIT, use=use, K=K, q=Q,
                out=np.full((ROWS, 6, Q, NFIT), -7.0, order="F"), hyper=np.full((NFIT, 4), -7.0))


def design_with(change):
    def make(a):
        D = a["design"].copy(order="F")
        change(D)
        return D
    return make


def k_nan(a):
    K = a["K"].copy(order="F")
    K[2, 1] = np.nan
    return K


def use_three(a):
    """fit 2 keeps three samples: n_f = p"""
    u = a["use"].copy(order="F")
    u[:, 1] = 0
    u[[0, 1, 4], 1] = 1
    return u


def set_(idx, val):
    def f(D):
        D[idx] = val
    return f


def dup(D):
    D[:, 2, 1] = D[:, 1, 1]


FAULTS = [   # name, what to change, status, a word of the text -- in the order of the checks
    ("rows", dict(rows=-1), _lib.EINVAL, "bad dims"),
    ("samples", dict(n=-2), _lib.EINVAL, "bad dims"),
    ("fits", dict(nfit=-1), _lib.EINVAL, "bad dims"),
    ("contrasts", dict(q=-1), _lib.EINVAL, "bad dims"),
    ("too many fits", dict(nfit=15001), _lib.EINVAL, "nfit <= 15000"),          # launch grid extents, refused as arguments
    ("too many samples", dict(n=8388481), _lib.EINVAL, "n <= 8388480"),
    ("p low", dict(p=0), _lib.EINVAL, "p = 0 coefficients (1 <= p <= 32)"),
    ("p high", dict(p=33), _lib.EINVAL, "p = 33 coefficients"),
    ("q without K", dict(K=None), _lib.EINVAL, "q = 2 without K (the p = 3 unit vectors)"),
    ("null design", dict(design=None), _lib.EINVAL, "null design"),
    ("null A", dict(A=None), _lib.EINVAL, "null A / out / hyper"),
    ("null out", dict(out=None), _lib.EINVAL, "null A / out / hyper"),
    ("null hyper", dict(hyper=None), _lib.EINVAL, "null A / out / hyper"),
    ("K value", dict(K=k_nan), _lib.EINVAL, "K[5] = nan"),
    ("design value", dict(design=design_with(set_((4, 2, 0), np.inf))), _lib.EINVAL, "fit 1 is not finite at sample 5, column 3"),
    ("design value, fit 2", dict(design=design_with(set_((0, 1, 1), np.nan))), _lib.EINVAL,
     "fit 2 is not finite at sample 1, column 2"),
    ("n_f = p", dict(use=use_three), _lib.EINVAL, "fit 2 has 3 samples for 3 coefficients"),
    ("duplicated column", dict(design=design_with(dup)), _lib.EINVAL, "column 3 of the design of fit 2 is rank-deficient"),
    ("zero column", dict(design=design_with(set_((slice(None), 1, 1), 0.0))), _lib.EINVAL,
     "column 2 of the design of fit 2 is rank-deficient"),
]
RANK = {name: k for k, (name, _, _, _) in enumerate(FAULTS)}
WHICH = ["limma", "limma_multi", "hook"]


def apply(a, change):
    return {**a, **{k: (v(a) if callable(v) else v) for k, v in change.items()}}


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name,change,status,word", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_fault_is_refused_before_any_device(which, name, change, status, word):
    a = apply(good(), change)
    rc, text = call(which, **a)
    assert rc == status and word in text, (rc, text)
    for o in ("out", "hyper"):
        if a[o] is not None:
            assert (a[o] == -7).all(), o


PAIRS = [("rows", "p low"), ("p high", "null design"), ("q without K", "null out"), ("null design", "K value"),
         ("null hyper", "design value"), ("K value", "duplicated column"), ("design value", "n_f = p"),
         ("design value", "zero column"), ("fits", "zero column")]


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("first,second", PAIRS)
def test_two_faults_report_the_earlier_check(which, first, second):
    assert RANK[first] < RANK[second]
    _, ch1, status, word = FAULTS[RANK[first]]
    _, ch2, _, _ = FAULTS[RANK[second]]
    a = apply(apply(good(), ch2), ch1)
    rc, text = call(which, **a)
    assert rc == status and word in text, (rc, text)


def test_within_a_fit_the_order_is_value_then_samples_then_rank_and_fits_go_in_order():
    a = good()
    both = design_with(lambda D: (set_((0, 1, 1), np.nan)(D), dup(D)))       # fit 2: a NaN in a used row and a duplicate
    rc, text = call("limma", **apply(a, dict(design=both)))
    assert rc == _lib.EINVAL and "not finite at sample 1, column 2" in text
    rc, text = call("limma", **apply(a, dict(design=design_with(dup), use=use_three)))
    assert rc == _lib.EINVAL and "has 3 samples for 3 coefficients" in text
    two = design_with(lambda D: (set_((slice(None), 1, 0), 0.0)(D), dup(D)))  # fit 1: a zero column; fit 2: a duplicate
    rc, text = call("limma", **apply(a, dict(design=two)))
    assert rc == _lib.EINVAL and "column 2 of the design of fit 1" in text


def test_a_nan_in_an_unused_design_row_is_accepted():
    a = good()
    a = apply(a, dict(design=design_with(set_((2, slice(None), 1), np.nan))))    # sample 3 takes no part in fit 2
    rc, text = call("limma", **a)
    assert rc == _lib.EINVAL and "null plaidhip_ctx" in text                     # past the checks: it wants a context
    for which in WHICH:                                                          # with every sample used it is refused
        rc, text = call(which, **apply(a, dict(use=None)))
        assert rc == _lib.EINVAL and "fit 2 is not finite at sample 3, column 1" in text


def test_a_valid_call_passes_the_checks_and_then_wants_a_context():
    rc, text = call("limma", **good())
    assert rc == _lib.EINVAL and "null plaidhip_ctx" in text
    a = good()
    rc, text = call("limma", **{**a, "K": None, "q": 3, "out": np.full((ROWS, 6, 3, NFIT), -7.0, order="F")})
    assert rc == _lib.EINVAL and "null plaidhip_ctx" in text


def test_the_device_list_and_shard_count_come_first():
    a = good()
    args = (ptr(a["A"]), ROWS, N, ptr(a["design"]), 0, NFIT, None, None, Q, ptr(a["out"]), ptr(a["hyper"]))
    assert _lib.load().plaidhip_limma_multi(None, 0, *args) == _lib.EINVAL
    assert "ndev = 0" in _lib.load().plaidhip_last_error_string().decode()
    assert hook("limma")(0, 0, -1, *args) == _lib.EINVAL
    assert "nshards = 0" in _lib.load().plaidhip_last_error_string().decode()


def test_nothing_to_compute_is_the_empty_result():
    """rows == 0, nfit == 0 or q == 0 return PLAIDHIP_OK with nothing written, without a device; the designs are still checked"""
    a = good()
    for change in (dict(rows=0, A=None, out=None), dict(nfit=0, design=None, use=None), dict(q=0, K=np.zeros((3, 0), order="F"))):
        for which in ("limma_multi", "hook"):
            rc, text = call(which, **apply(a, change))
            assert rc == _lib.OK, text
            assert (a["out"] == -7).all() and (a["hyper"] == -7).all()
    rc, text = call("hook", **apply(a, dict(rows=0, design=design_with(dup))))
    assert rc == _lib.EINVAL and "rank-deficient" in text


def test_the_host_entries_check_their_own_arguments():
    lib = _lib.load()
    D = good()["design"][:, :, 0].copy(order="F")
    assert lib.plaidhip_limma_design(ptr(D), N, 0, None, None, 0, 1, None, None, None, None, None) == _lib.EINVAL
    assert "p = 0 coefficients" in lib.plaidhip_last_error_string().decode()
    assert lib.plaidhip_limma_design(ptr(D), N, 3, None, None, 2, 1, None, None, None, None, None) == _lib.EINVAL
    assert "without K" in lib.plaidhip_last_error_string().decode()
    D[:, 2] = 2 * D[:, 0]
    with pytest.raises(_lib.PlaidHipError, match="column 3 of the design of fit 5 is rank-deficient"):
        engine.limma_design(D, fit=5)
    E, rss = np.zeros((3, 4)), np.ones((1, 4))
    with pytest.raises(_lib.PlaidHipError, match="fit 1 has 2 samples for 2 coefficients"):
        engine.limma_finish(E, rss, [2], np.eye(2), [1.0, 1.0])


def test_the_python_entries():
    """what Python sees before the library does, and the library's own text through the marshaller"""
    a = good()
    with pytest.raises(ValueError, match="one row per column"):
        engine.limma_operands(N + 1, a["design"])
    with pytest.raises(ValueError, match="samples x fits"):
        engine.limma_operands(N, a["design"], use=np.ones(N))
    with pytest.raises(ValueError, match="coefficients x contrasts"):
        engine.limma_operands(N, a["design"], contrasts=np.ones((4, 1)))
    D, U, K, q = engine.limma_operands(N, a["design"][:, :, 0], use=[1.0, np.nan, 0.0] + [1] * 6, contrasts=[0, 1, 0])
    assert D.shape == (N, 3, 1) and U.dtype == np.int8 and U[:, 0].tolist() == [1, 0, 0] + [1] * 6 and K.shape == (3, 1) and q == 1
    fn = _lib.load().plaidhip_limma
    with pytest.raises(_lib.PlaidHipError, match="null plaidhip_ctx"):
        engine._limma(fn, (None,), a["A"], a["design"], a["use"], a["K"])
    bad = a["design"].copy(order="F")
    bad[:, 1, 0] = 0.0
    with pytest.raises(_lib.PlaidHipError, match="column 2 of the design of fit 1 is rank-deficient"):
        engine._limma(fn, (None,), a["A"], bad, a["use"], a["K"])
    S = plaid_amd.NamedMatrix(a["A"], [f"s{k}" for k in range(ROWS)], [f"c{k}" for k in range(N)])
    with pytest.raises(ValueError, match="sort_by"):
        plaid_amd.plaid_limma(S, a["design"][:, :, 0], sort_by="B")
    with pytest.raises(ValueError, match="must be dense"):
        plaid_amd.plaid_limma(plaid_amd.NamedMatrix(sp.csc_matrix(a["A"])), a["design"][:, :, 0])
    with pytest.raises(ValueError, match="0, 1 or NA"):
        plaid_amd.plaid_limma_contrasts(S, np.full((N, 1), 3.0))
    with pytest.raises(ValueError, match="one row per column of S"):
        plaid_amd.plaid_limma_contrasts(S, np.arange(N) % 2, B=np.ones(N + 1))
