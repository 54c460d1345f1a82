"""plaidhip_ucell_exact / plaidhip_aucell_exact, their _multi forms and their test hooks refuse a wrong call before any device
is touched: this file runs where there is none.  Each fault goes into the context entry (with a null context, which is
refused only after the arguments), the _multi entry and the hook; all three give the same status and the same text."""
import ctypes as C
import math

import numpy as np
import pytest

from plaid_amd import _lib, engine
from tests.helpers import sharded_hooks

_i32 = lambda *v: np.array(v, dtype=np.int32)   # noqa: E731
_BUF = np.zeros((6, 6), order="F")
UCELL = ["Xp", "Xi", "X", "g", "n", "Gp", "Gi", "Dp", "Di", "m", "max_rank", "w_neg", "impute", "k_full", "k_full_down", "total",
         "up", "down"]
AUCELL = ["Xp", "Xi", "X", "g", "n", "Gp", "Gi", "m", "max_rank", "S"]
BASE = dict(Xp=None, Xi=None, X=np.ones((4, 3), order="F"), g=4, n=3, Gp=_i32(0, 2, 4), Gi=_i32(0, 1, 2, 3), Dp=None, Di=None,
            m=2, max_rank=2.0, w_neg=1.0, impute=0, k_full=None, k_full_down=None, total=None, up=_BUF, down=None, S=_BUF)
NO_VALUES = dict(Xp=_i32(0, 0, 0, 0), Xi=None, X=None)
DOWN = dict(Dp=_i32(0, 1, 2), Di=_i32(0, 3))
EINVAL, EUNSUPPORTED = _lib.EINVAL, _lib.EUNSUPPORTED
# fault -> (changes, status, a piece of the text, entries)
FAULTS = {
    "T = 0": (dict(max_rank=0.0), EINVAL, "must be an integer in 1..nrow(X) = 4", "ucell aucell"),
    "T = N + 1": (dict(max_rank=5.0), EINVAL, "must be an integer in 1..nrow(X) = 4", "ucell aucell"),
    "T = 1.5": (dict(max_rank=1.5), EINVAL, "must be an integer in 1..nrow(X) = 4 (got 1.5)", "ucell aucell"),
    "T = nan": (dict(max_rank=math.nan), EINVAL, "must be an integer", "ucell aucell"),
    "w_neg < 0": (dict(w_neg=-0.5), EINVAL, "w_neg must be finite and >= 0", "ucell"),
    "w_neg = nan": (dict(w_neg=math.nan), EINVAL, "w_neg must be finite and >= 0", "ucell"),
    "w_neg = inf": (dict(w_neg=math.inf), EINVAL, "w_neg must be finite and >= 0", "ucell"),
    "impute without k_full": (dict(impute=1), EINVAL, "impute needs k_full", "ucell"),
    "impute without k_full_down": (dict(DOWN, impute=1, k_full=np.full(2, 2.0), down=_BUF), EINVAL, "impute needs k_full_down",
                                   "ucell"),
    "k_full below the aligned size": (dict(impute=1, k_full=np.array([2.0, 1.0])), EINVAL, "k_full[1] = 1 is no integer >=",
                                      "ucell"),
    "k_full = 2.5": (dict(impute=1, k_full=np.array([2.5, 2.0])), EINVAL, "k_full[0] = 2.5 is no integer >=", "ucell"),
    "k_full over 2^53": (dict(impute=1, k_full=np.array([2.0, 2.0 ** 40])), EUNSUPPORTED, "does not stay below 2^53", "ucell"),
    "total without down sets": (dict(total=_BUF), EINVAL, "total and down results need the down sets", "ucell"),
    "down without down sets": (dict(down=_BUF), EINVAL, "total and down results need the down sets", "ucell"),
    "down sets without Di": (dict(Dp=_i32(0, 1, 2), Di=None, down=_BUF), EINVAL, "null Di", "ucell"),
    "no output requested": (dict(up=None, S=None), EINVAL, "no output requested", "ucell aucell"),
    "2 N T reaches 2^53": (dict(NO_VALUES, g=2 ** 31 - 1, max_rank=float(2 ** 21 + 1)), EUNSUPPORTED, "does not stay below 2^53",
                           "ucell aucell"),
    "rows over 2^26 - 1": (dict(NO_VALUES, g=1 << 26), EINVAL, "at most 2^26 - 1 rows", "ucell aucell"),
    "null X": (dict(X=None), EINVAL, "null X", "ucell aucell"),
    "null Gp": (dict(Gp=None), EINVAL, "", "ucell aucell"),
    "g = 0": (dict(g=0), EINVAL, "", "ucell aucell"),
    "CSC rows not increasing": (dict(Xp=_i32(0, 2, 3, 4), Xi=_i32(1, 0, 2, 3), X=np.arange(1.0, 5.0)), EINVAL,
                                "are not increasing", "ucell aucell"),
}


def _arg(v):
    return v.ctypes.data if isinstance(v, np.ndarray) else v


def _calls(entry, args):
    """(what, status, text) of the context entry (null context), the _multi entry and the hook"""
    lib = _lib.load()
    a = [_arg(args[k]) for k in (UCELL if entry == "ucell" else AUCELL)]
    name = f"{entry}_exact"
    fns = (("context", getattr(lib, f"plaidhip_{name}"), (None,)),
           ("multi", getattr(lib, f"plaidhip_{name}_multi"), (None, 1)),
           ("hook", sharded_hooks.hook(name), (0, 2, -1)))
    for what, fn, head in fns:
        rc = fn(*head, *a)
        yield what, rc, lib.plaidhip_last_error_string().decode()


@pytest.mark.parametrize("fault", list(FAULTS))
def test_refused_before_any_device(fault):
    change, status, text, entries = FAULTS[fault]
    for entry in entries.split():
        args = dict(BASE, **change)
        seen = list(_calls(entry, args))
        for what, rc, msg in seen:
            assert rc == status, (entry, what, rc, msg)
            assert text in msg, (entry, what, msg)
            assert msg == seen[0][2], (entry, what, msg, seen[0][2])


def test_the_rank_bound_comes_before_x_is_read():
    """2 N T >= 2^53 is PLAIDHIP_EUNSUPPORTED; one below the bound the next check answers (the rows)"""
    g = 2 ** 31 - 1
    for entry in ("ucell", "aucell"):
        T = math.ceil(2 ** 52 / g)
        assert 2 * g * T >= 2 ** 53 > 2 * g * (T - 1)
        for what, rc, msg in _calls(entry, dict(BASE, **NO_VALUES, g=g, max_rank=float(T))):
            assert rc == EUNSUPPORTED and "2^53" in msg, (entry, what, msg)
        for what, rc, msg in _calls(entry, dict(BASE, **NO_VALUES, g=g, max_rank=float(T - 1))):
            assert rc == EINVAL and "2^26 - 1 rows" in msg, (entry, what, msg)


@pytest.mark.parametrize("change", [dict(n=0), dict(m=0, Gp=_i32(0))])
def test_empty_calls_return_at_once(change):
    """no sets or no samples: PLAIDHIP_OK with nothing written, whatever the rank, from the _multi entries and the hooks (the
    context entry refuses its null context instead)"""
    for entry in ("ucell", "aucell"):
        out = np.full((6, 6), -7.0, order="F")
        args = dict(BASE, **change, up=out, S=out, max_rank=99.0)
        for what, rc, msg in _calls(entry, args):
            if what == "context":
                assert rc == EINVAL and "null plaidhip_ctx" in msg
            else:
                assert rc == _lib.OK, (entry, what, msg)
        assert (out == -7.0).all()


def test_python_wrappers_check_before_a_device():
    with pytest.raises(ValueError, match="integer in 1..nrow"):
        engine.check_truncated_rank("ucell_exact", "maxRank", 100, 0)
    with pytest.raises(ValueError, match="integer in 1..nrow"):
        engine.check_truncated_rank("aucell_exact", "aucMaxRank", 100, 2.5)
    with pytest.raises(_lib.PlaidHipError) as ei:
        engine.check_truncated_rank("ucell_exact", "maxRank", 2 ** 31 - 1, 2 ** 22)
    assert ei.value.code == EUNSUPPORTED
    assert engine.check_truncated_rank("ucell_exact", "maxRank", 100, 100) == 100.0
    for name in ("plaidhip_ucell_exact", "plaidhip_aucell_exact", "plaidhip_ucell_exact_multi", "plaidhip_aucell_exact_multi",
                 "plaidhip_dev_truncated_ranks_f64", "plaidhip_dev_truncated_ranks_csc_f64"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    with pytest.raises(ValueError, match="w_neg"):
        engine._ucell_exact_call(None, (), np.ones((4, 3)), _i32(0, 2), _i32(0, 1), None, None, 2, -1.0, None, None)
