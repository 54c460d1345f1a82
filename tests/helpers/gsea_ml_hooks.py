"""The test hook of plaid.gsea's multilevel p-values (multi.cpp: plaidhip_debug_gsea_multilevel_sharded_on_one_device), bound
as tests/helpers/gsea_hooks.py binds plaid.gsea's: `nshards` contexts on one device behind the engine of
plaidhip_gsea_multilevel_multi; a failed call returns its status."""
from plaid_amd import engine

from .sharded_hooks import _status, hook


def gsea_multilevel(nshards, stat, weight, Gp, Gi, fail=-1, **kw):
    """(status, (out, ml, null, le_len, le_idx) or None) of engine._gsea_multilevel on the hook, null scores and edges included"""
    return _status(lambda: engine._gsea_multilevel(hook("gsea_multilevel"), (0, nshards, fail), stat, weight, Gp, Gi, null=True,
                                                   leading_edge=True, **kw))
