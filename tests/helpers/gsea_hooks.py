"""The test hook of plaid.gsea (multi.cpp: plaidhip_debug_gsea_sharded_on_one_device), bound as tests/helpers/sharded_hooks.py
binds the others: `nshards` contexts on one device behind the engine of plaidhip_gsea_multi; a failed call returns its
status."""
from plaid_amd import engine

from .sharded_hooks import _status, hook


def gsea(nshards, stat, weight, Gp, Gi, perm=None, nperm=1000, seed=0, fail=-1):
    """(status, (out, null) or None) of engine._gsea on the hook, the null scores included"""
    return _status(lambda: engine._gsea(hook("gsea"), (0, nshards, fail), stat, weight, Gp, Gi, perm, nperm, seed, null=True))
