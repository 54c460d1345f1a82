"""Every plaidhip_*_multi entry and every test hook refuses a wrong call before it touches a device, with one status and
one text per fault.

The table drives one fault at a time into each entry that takes the argument.  EXPECTED was recorded by running this
very table (`python -m tests.test_entry_checks_host`, PLAIDHIP_LIB pointing at that build) against the library of commit
cb8dba8, the last one whose entries each had a path of their own to run_call, on a machine with a device (that build
created a hook's contexts before it checked an argument): dispatch / check_call (multi.cpp) may not change a status or a
text.  Not reachable
without a device, so not here: "multi: device %d out of range" (needs the device count) and what a worker reports.
"scorer: bad method" inside check_call is reachable only through the plaid / sing / ssgsea hook with an ordinal that
is no method at all, which the recorded build did not refuse."""
import math

import numpy as np
import pytest

from plaid_amd import _lib
from tests.helpers import sharded_hooks

_X = ["Xp", "Xi", "X", "g", "n"]
_G = ["Gp", "Gi", "m"]
_SCORER = ["k_full", "rmax", "auc_max_rank", "remove_log2", "score_mean", "tau", "rowtf", "S", "removed"]
# entry -> (its own parameters in C order, the hook that runs it, what the hook puts in front of them)
ENTRIES = {
    "plaid": (_X + _G + ["stat", "normalize", "S"], "", _X + _G + ["stat", "normalize", "alpha", "S"], 0),
    "sing": (["X", "g", "n"] + _G + ["S"], "", _X + _G + ["stat", "normalize", "alpha", "S"], 1),
    "sing_csc": (_X + _G + ["S"], None, None, None),
    "ssgsea": (_X + _G + ["alpha", "S"], "", _X + _G + ["stat", "normalize", "alpha", "S"], 2),
    "ucell": (_X + _G + ["k_full", "rmax", "S"], "scorer", _X + _G + _SCORER, 3),
    "aucell": (_X + _G + ["auc_max_rank", "S"], "scorer", _X + _G + _SCORER, 4),
    "scse": (_X + _G + ["remove_log2", "score_mean", "S", "removed"], "scorer", _X + _G + _SCORER, 5),
    "gsva": (_X + _G + ["tau", "rowtf", "S"], "scorer", _X + _G + _SCORER, 6),
    "plaid_test": (_X + ["y"] + _G + ["gsetX", "tests", "metap", "out"], "plaid_test", None, None),
    "ssgsea_exact": (_X + _G + ["alpha", "scale", "norm", "S"], "ssgsea_exact", None, None),
    "ssgsea_exact_ks": (_X + _G + ["alpha", "scale", "norm", "S"], "ssgsea_exact_ks", None, None),
    "gsva_exact": (_X + _G + ["tau", "rowtf", "max_diff", "S"], "gsva_exact", None, None),
    "sing_exact": (_X + ["Gp", "Gi", "Dp", "Di", "m", "center", "o0", "o1", "o2", "o3", "o4", "o5"], "sing_exact", None, None),
}
_i32 = lambda *v: np.array(v, dtype=np.int32)   # noqa: E731
_BUF = np.zeros((6, 6), order="F")
BASE = dict(Xp=None, Xi=None, X=np.ones((4, 3), order="F"), g=4, n=3, Gp=_i32(0, 2, 4), Gi=_i32(0, 1, 2, 3), m=2, S=_BUF,
            stat=0, normalize=1, alpha=0.25, k_full=np.full(2, 2.0), rmax=5.0, auc_max_rank=2.0, remove_log2=-1, score_mean=0,
            removed=None, tau=1.0, rowtf=0, y=_i32(0, 1, 0), gsetX=None, tests=7, metap=0, out=_BUF, scale=1, norm=0,
            max_diff=1, Dp=None, Di=None, center=1, o0=None, o1=_BUF, o2=None, o3=None, o4=None, o5=None)
CSC = dict(Xp=_i32(0, 2, 3, 4), Xi=_i32(0, 1, 2, 3), X=np.array([1.0, 2.0, 3.0, 4.0]))
NO_VALUES = dict(Xp=_i32(0, 0, 0, 0), Xi=None, X=None)   # a CSC X with no stored values: any row count is cheap
ROWS_KS, ROWS_26 = 131072 + 1, 1 << 26
_EXACT = "ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact"
_CHECK_XI = "ucell aucell scse gsva plaid_test " + _EXACT   # (plaid / sing / ssgsea take a pattern-free CSC: Xi unchecked)
# fault -> (the arguments it changes, the entries it is driven into: None = every entry that takes all of them)
FAULTS = {
    "g = 0": (dict(g=0), None),
    "n < 0": (dict(n=-1), None),
    "m < 0": (dict(m=-1), None),
    "null Gp": (dict(Gp=None), None),
    "null Gi": (dict(Gi=None), _EXACT),
    "null X": (dict(X=None), None),
    "null S_out": (dict(S=None), None),
    "null out": (dict(out=None), None),
    "no output requested": (dict(o1=None), None),
    "bad stat": (dict(stat=2), "plaid"),
    "alpha = inf": (dict(alpha=math.inf), _EXACT),
    "alpha = nan": (dict(alpha=math.nan), _EXACT),
    "tau = nan": (dict(tau=math.nan), "gsva_exact"),
    "tau < 0": (dict(tau=-1.0), "gsva_exact"),
    "rowtf = 4": (dict(rowtf=4), "gsva gsva_exact"),
    "rowtf = 2": (dict(rowtf=2), "gsva"),
    "rowtf = ecdf": (dict(rowtf=1), "gsva"),
    "rowtf = ecdf, two devices": (dict(rowtf=1, ndev=2), "gsva gsva_exact"),
    "rowtf = gauss, one sample": (dict(rowtf=3, n=1), "gsva_exact"),
    "rmax = 0": (dict(rmax=0.0), "ucell"),
    "aucMaxRank = 0": (dict(auc_max_rank=0.0), "aucell"),
    "null k_full": (dict(k_full=None), "ucell"),
    "null y": (dict(y=None), None),
    "y holds a 2": (dict(y=_i32(0, 2, 1)), None),
    "tests = 0": (dict(tests=0), None),
    "tests = 8": (dict(tests=8), None),
    "metap = 2": (dict(metap=2), None),
    "rows over the walk's bound": (dict(NO_VALUES, g=ROWS_KS), "ssgsea_exact_ks gsva_exact sing_exact"),
    "rows over the walk's bound, dispersion": (dict(NO_VALUES, g=ROWS_KS, o4=_BUF), "sing_exact"),
    "rows over 2^26 - 1": (dict(NO_VALUES, g=ROWS_26), _EXACT),
    "totals without down sets": (dict(o0=_BUF), None),
    "down sets without Di": (dict(Dp=_i32(0, 1, 2), Di=None), None),
    "CSC null Xp": (dict(Xp=None, Xi=CSC["Xi"], X=None), None),
    "CSC Xp[0] = 1": (dict(CSC, Xp=_i32(1, 2, 3, 4)), None),
    "CSC Xp decreases": (dict(CSC, Xp=_i32(0, 3, 2, 4)), None),
    "CSC Xi out of range": (dict(CSC, Xi=_i32(0, 1, 2, 4)), None),
    "CSC null Xi": (dict(CSC, Xi=None), _CHECK_XI),
    "CSC null Xx": (dict(CSC, X=None), None),
    "CSC rows not increasing": (dict(CSC, Xi=_i32(1, 0, 2, 3)), _EXACT),
    "CSC more values than cells": (dict(Xp=_i32(0, 7, 13, 13), Xi=np.zeros(13, dtype=np.int32), X=np.ones(13)), "gsva"),
    "ndev = 0": (dict(ndev=0), None),
    "ndev = 65": (dict(ndev=65), None),
    "device listed twice": (dict(devices=_i32(0, 0), ndev=2), None),
}


def _arg(v):
    return v.ctypes.data if isinstance(v, np.ndarray) else v


def rows(target):
    """(entry, fault, call): every fault into every entry of `target` ("multi" or "hook") that takes one of its arguments"""
    lib = _lib.load()
    for entry, (own, hook, hook_params, method) in ENTRIES.items():
        if target == "hook" and hook is None:
            continue
        names = own if target == "multi" or hook_params is None else hook_params
        for fault, (change, only) in FAULTS.items():
            if (target == "hook" and "devices" in change) or (only is not None and entry not in only.split()):
                continue
            if not all(k in names or k in ("ndev", "devices") for k in change):
                continue
            v = {**BASE, **(CSC if entry == "sing_csc" else {}), "devices": None, "ndev": 1, **change}
            args = [_arg(v[k]) for k in names]
            if target == "multi":
                fn, head = getattr(lib, f"plaidhip_{entry}_multi"), [_arg(v["devices"]), v["ndev"]]
            else:
                fn, head = sharded_hooks.hook(hook), [0, v["ndev"], -1] + ([] if method is None else [method])
            yield entry, fault, (lambda fn=fn, a=head + args: fn(*a))


def outcome(call):
    rc = call()
    return rc, _lib.load().plaidhip_last_error_string().decode() if rc else ""


def record():
    """the literal below, from the library PLAIDHIP_LIB names: failures only, entries with one outcome grouped"""
    for target in ("multi", "hook"):
        table = {}
        for entry, fault, call in rows(target):
            rc, text = outcome(call)
            if rc not in (_lib.OK, _lib.EHIP, _lib.ENODEVICE):
                table.setdefault(fault, {}).setdefault((rc, text), []).append(entry)
        print(f'    "{target}": {{')
        for fault, outs in table.items():
            print(f"        {fault!r}: {{")
            for (rc, text), entries in outs.items():
                print(f"            ({rc}, {text!r}): {' '.join(entries)!r},")
            print("        },")
        print("    },")


EXPECTED = {
    "multi": {
        'g = 0': {
            (1, 'bad dims g=0 n=3 m=2'): 'plaid sing sing_csc ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'n < 0': {
            (1, 'bad dims g=4 n=-1 m=2'): 'plaid sing sing_csc ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'm < 0': {
            (1, 'bad dims g=4 n=3 m=-1'): 'plaid sing sing_csc ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'null Gp': {
            (1, 'null Gp'): 'plaid sing sing_csc ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'null X': {
            (1, 'null X'): 'plaid sing sing_csc ssgsea ucell aucell scse gsva',
            (1, 'plaid_test: null X / y'): 'plaid_test',
            (1, 'ssgsea_exact: null X'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'null S_out': {
            (1, 'null S_out'): 'plaid sing sing_csc ssgsea ucell aucell scse gsva',
            (1, 'ssgsea_exact: null S_out'): 'ssgsea_exact ssgsea_exact_ks gsva_exact',
        },
        'bad stat': {
            (1, 'plaid_multi: bad stat 2'): 'plaid',
        },
        'CSC null Xp': {
            (1, 'null X'): 'plaid ssgsea ucell aucell scse gsva',
            (1, 'sing_csc_multi: null Xp'): 'sing_csc',
            (1, 'plaid_test: null X / y'): 'plaid_test',
            (1, 'ssgsea_exact: null X'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'CSC Xp[0] = 1': {
            (1, 'Xp[0] = 1, expected 0'): 'plaid sing_csc ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'CSC Xp decreases': {
            (1, 'Xp decreases at column 1 (more than 2^31-1 stored values? split the matrix by columns)'): 'plaid sing_csc ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'CSC Xi out of range': {
            (1, 'Xi[3] = 4 outside [0, 4)'): 'plaid sing_csc ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'CSC null Xx': {
            (1, 'null X'): 'plaid sing_csc ssgsea ucell aucell scse gsva',
            (1, 'plaid_test: null Xi/Xx'): 'plaid_test',
            (1, 'ssgsea_exact: null X'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'ndev = 0': {
            (1, 'multi: ndev = 0'): 'plaid sing sing_csc ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'ndev = 65': {
            (1, 'multi: ndev = 65'): 'plaid sing sing_csc ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'device listed twice': {
            (1, 'multi: device 0 listed twice'): 'plaid sing sing_csc ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'rmax = 0': {
            (1, 'ucell: rmax must be positive'): 'ucell',
        },
        'null k_full': {
            (1, 'ucell: null k_full'): 'ucell',
        },
        'CSC null Xi': {
            (1, 'null Xi'): 'ucell aucell scse gsva',
            (1, 'plaid_test: null Xi/Xx'): 'plaid_test',
            (1, 'ssgsea_exact: null Xi'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'aucMaxRank = 0': {
            (1, 'aucell: aucMaxRank must be positive'): 'aucell',
        },
        'rowtf = 4': {
            (1, 'Error: unknown row transform 4'): 'gsva gsva_exact',
        },
        'rowtf = 2': {
            (1, 'Error: unknown row transform 2'): 'gsva',
        },
        'rowtf = ecdf': {
            (1, 'gsva: rowtf = "ecdf" ranks all samples of a gene together and is not sharded by sample; score it on one device (plaidhip_gsva / plaidhip_gsva_csc)'): 'gsva',
        },
        'rowtf = ecdf, two devices': {
            (1, 'gsva: rowtf = "ecdf" ranks all samples of a gene together and is not sharded by sample; score it on one device (plaidhip_gsva / plaidhip_gsva_csc)'): 'gsva',
            (1, 'gsva_exact_multi: rowtf = "ecdf" ranks all samples of a gene together and is not sharded by sample; score it on one device (plaidhip_gsva_exact)'): 'gsva_exact',
        },
        'CSC more values than cells': {
            (1, 'gsva: 13 stored values in a 4 x 3 matrix (repeated row indices?)'): 'gsva',
        },
        'null out': {
            (1, 'plaid_test: null out'): 'plaid_test',
        },
        'null y': {
            (1, 'plaid_test: null X / y'): 'plaid_test',
        },
        'y holds a 2': {
            (1, 'elements of y must be 0 or 1'): 'plaid_test',
        },
        'tests = 0': {
            (1, 'plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)'): 'plaid_test',
        },
        'tests = 8': {
            (1, 'plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)'): 'plaid_test',
        },
        'metap = 2': {
            (1, 'Invalid method: 2'): 'plaid_test',
        },
        'null Gi': {
            (1, 'ssgsea_exact: null Gi'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'alpha = inf': {
            (1, 'ssgsea_exact: alpha must be finite (got inf)'): 'ssgsea_exact ssgsea_exact_ks',
        },
        'alpha = nan': {
            (1, 'ssgsea_exact: alpha must be finite (got nan)'): 'ssgsea_exact ssgsea_exact_ks',
        },
        'rows over 2^26 - 1': {
            (1, 'ssgsea_exact: nrow(X) = 67108864 (at most 2^26 - 1 rows)'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'CSC rows not increasing': {
            (1, 'ssgsea_exact: row indices of column 0 are not increasing (Xi[1] = 0 after 1)'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        "rows over the walk's bound": {
            (4, 'ssgsea_exact_ks: nrow(X) = 131073 (at most 131072 rows with single = FALSE)'): 'ssgsea_exact_ks',
            (4, 'gsva_exact: nrow(X) = 131073 (at most 131072 rows)'): 'gsva_exact',
        },
        'tau = nan': {
            (1, 'gsva_exact: tau must be finite and >= 0 (got nan)'): 'gsva_exact',
        },
        'tau < 0': {
            (1, 'gsva_exact: tau must be finite and >= 0 (got -1)'): 'gsva_exact',
        },
        'rowtf = gauss, one sample': {
            (1, 'gsva_exact: rowtf = "gauss" needs at least 2 samples (got 1)'): 'gsva_exact',
        },
        'no output requested': {
            (1, 'sing_exact: no output requested'): 'sing_exact',
        },
        "rows over the walk's bound, dispersion": {
            (4, 'sing_exact: nrow(X) = 131073 (at most 131072 rows with the dispersion)'): 'sing_exact',
        },
        'totals without down sets': {
            (1, 'sing_exact: total and down results need the down sets'): 'sing_exact',
        },
        'down sets without Di': {
            (1, 'sing_exact: null Di'): 'sing_exact',
        },
    },
    "hook": {
        'g = 0': {
            (1, 'bad dims g=0 n=3 m=2'): 'plaid sing ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'n < 0': {
            (1, 'bad dims g=4 n=-1 m=2'): 'plaid sing ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'm < 0': {
            (1, 'bad dims g=4 n=3 m=-1'): 'plaid sing ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'null Gp': {
            (1, 'null Gp'): 'plaid sing ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'null X': {
            (1, 'null X'): 'plaid sing ssgsea ucell aucell scse gsva',
            (1, 'plaid_test: null X / y'): 'plaid_test',
            (1, 'ssgsea_exact: null X'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'null S_out': {
            (1, 'null S_out'): 'plaid sing ssgsea ucell aucell scse gsva',
            (1, 'ssgsea_exact: null S_out'): 'ssgsea_exact ssgsea_exact_ks gsva_exact',
        },
        'CSC null Xp': {
            (1, 'null X'): 'plaid sing ssgsea ucell aucell scse gsva',
            (1, 'plaid_test: null X / y'): 'plaid_test',
            (1, 'ssgsea_exact: null X'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'CSC Xp[0] = 1': {
            (1, 'Xp[0] = 1, expected 0'): 'plaid sing ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'CSC Xp decreases': {
            (1, 'Xp decreases at column 1 (more than 2^31-1 stored values? split the matrix by columns)'): 'plaid sing ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'CSC Xi out of range': {
            (1, 'Xi[3] = 4 outside [0, 4)'): 'plaid sing ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'CSC null Xx': {
            (1, 'null X'): 'plaid sing ssgsea ucell aucell scse gsva',
            (1, 'plaid_test: null Xi/Xx'): 'plaid_test',
            (1, 'ssgsea_exact: null X'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'ndev = 0': {
            (1, 'debug_sharded: nshards = 0'): 'plaid sing ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'ndev = 65': {
            (1, 'debug_sharded: nshards = 65'): 'plaid sing ssgsea ucell aucell scse gsva plaid_test ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'rmax = 0': {
            (1, 'ucell: rmax must be positive'): 'ucell',
        },
        'null k_full': {
            (1, 'ucell: null k_full'): 'ucell',
        },
        'CSC null Xi': {
            (1, 'null Xi'): 'ucell aucell scse gsva',
            (1, 'plaid_test: null Xi/Xx'): 'plaid_test',
            (1, 'ssgsea_exact: null Xi'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'aucMaxRank = 0': {
            (1, 'aucell: aucMaxRank must be positive'): 'aucell',
        },
        'rowtf = 4': {
            (1, 'Error: unknown row transform 4'): 'gsva gsva_exact',
        },
        'rowtf = 2': {
            (1, 'Error: unknown row transform 2'): 'gsva',
        },
        'rowtf = ecdf, two devices': {
            (1, 'gsva: rowtf = "ecdf" ranks all samples of a gene together and is not sharded by sample; score it on one device (plaidhip_gsva / plaidhip_gsva_csc)'): 'gsva',
            (1, 'gsva_exact_multi: rowtf = "ecdf" ranks all samples of a gene together and is not sharded by sample; score it on one device (plaidhip_gsva_exact)'): 'gsva_exact',
        },
        'CSC more values than cells': {
            (1, 'gsva: 13 stored values in a 4 x 3 matrix (repeated row indices?)'): 'gsva',
        },
        'null out': {
            (1, 'plaid_test: null out'): 'plaid_test',
        },
        'null y': {
            (1, 'plaid_test: null X / y'): 'plaid_test',
        },
        'y holds a 2': {
            (1, 'elements of y must be 0 or 1'): 'plaid_test',
        },
        'tests = 0': {
            (1, 'plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)'): 'plaid_test',
        },
        'tests = 8': {
            (1, 'plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)'): 'plaid_test',
        },
        'metap = 2': {
            (1, 'Invalid method: 2'): 'plaid_test',
        },
        'null Gi': {
            (1, 'ssgsea_exact: null Gi'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'alpha = inf': {
            (1, 'ssgsea_exact: alpha must be finite (got inf)'): 'ssgsea_exact ssgsea_exact_ks',
        },
        'alpha = nan': {
            (1, 'ssgsea_exact: alpha must be finite (got nan)'): 'ssgsea_exact ssgsea_exact_ks',
        },
        'rows over 2^26 - 1': {
            (1, 'ssgsea_exact: nrow(X) = 67108864 (at most 2^26 - 1 rows)'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        'CSC rows not increasing': {
            (1, 'ssgsea_exact: row indices of column 0 are not increasing (Xi[1] = 0 after 1)'): 'ssgsea_exact ssgsea_exact_ks gsva_exact sing_exact',
        },
        "rows over the walk's bound": {
            (4, 'ssgsea_exact_ks: nrow(X) = 131073 (at most 131072 rows with single = FALSE)'): 'ssgsea_exact_ks',
            (4, 'gsva_exact: nrow(X) = 131073 (at most 131072 rows)'): 'gsva_exact',
        },
        'tau = nan': {
            (1, 'gsva_exact: tau must be finite and >= 0 (got nan)'): 'gsva_exact',
        },
        'tau < 0': {
            (1, 'gsva_exact: tau must be finite and >= 0 (got -1)'): 'gsva_exact',
        },
        'rowtf = gauss, one sample': {
            (1, 'gsva_exact: rowtf = "gauss" needs at least 2 samples (got 1)'): 'gsva_exact',
        },
        'no output requested': {
            (1, 'sing_exact: no output requested'): 'sing_exact',
        },
        "rows over the walk's bound, dispersion": {
            (4, 'sing_exact: nrow(X) = 131073 (at most 131072 rows with the dispersion)'): 'sing_exact',
        },
        'totals without down sets': {
            (1, 'sing_exact: total and down results need the down sets'): 'sing_exact',
        },
        'down sets without Di': {
            (1, 'sing_exact: null Di'): 'sing_exact',
        },
    },
}


@pytest.mark.parametrize("target", ["multi", "hook"])
def test_single_faults_keep_their_status_and_text(target):
    want = {(e, fault): out for fault, outs in EXPECTED[target].items() for out, es in outs.items() for e in es.split()}
    seen = set()
    for entry, fault, call in rows(target):
        if (entry, fault) in want:
            assert outcome(call) == want[entry, fault], (target, entry, fault)
            seen.add((entry, fault))
    assert seen == set(want)


if __name__ == "__main__":
    record()
