"""The test hooks of replaid.ucell.exact and replaid.aucell.exact (multi.cpp: plaidhip_debug_ucell_exact_sharded_on_one_device,
plaidhip_debug_aucell_exact_sharded_on_one_device), bound as tests/helpers/sharded_hooks.py binds the others: `nshards`
contexts on one device behind the engine of the plaidhip_*_multi entry; a failed call returns its status."""
from plaid_amd import engine

from .sharded_hooks import _status, hook, score


def ucell_exact(nshards, X, Gp, Gi, Dp=None, Di=None, max_rank=1500, w_neg=1.0, k_full=None, k_full_down=None, fail=-1):
    """(status, dict of results or None); the results hold -7 before the call"""
    return _status(lambda: engine._ucell_exact_call(hook("ucell_exact"), (0, nshards, fail), X, Gp, Gi, Dp, Di, max_rank, w_neg,
                                                    k_full, k_full_down, fill=-7.0))


def aucell_exact(nshards, X, Gp, Gi, auc_max_rank, fail=-1):
    """(status, S); S holds NaN before the call"""
    return score("aucell_exact", nshards, X, Gp, Gi, float(auc_max_rank), fail=fail)
