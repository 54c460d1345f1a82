"""The pair plan's flex steps on the host (geneset.cpp, plan_tile_flex; no GPU).

A register-partial pair plan lends the step-7 cells of short lanes (hosts) to the overflow of long lanes (owners) of the
same tile, so a tile takes T steps where its longest lane alone would ask for up to 9T/8.

Figures of the benchmark's collection, synth.geneset_csc(20000, 5000), from plaidhip_debug_pair_flex_probe on this build
(measured):

    padded gather slots per column pair   798,720 with flex steps, 861,696 without (the parent's plan)
    double-booked slot reads                  692 with flex steps,     780 without
    owner <-> host pairs                      397

test_benchmark_collection_slots_and_double_booked_reads holds the plan to the two bounds its issue set: at most 810,000
slots, and no more double-booked reads than the plan without flex steps.  Fewer steps for the same lanes mean fuller
slots; with the sets in the lanes they had the plan stood at 810,496 slots and 2,587 double-booked reads.  A tile that can
take flex steps therefore deals its sets to the four 16-lane groups first (balance_tile_lanes), which levels the slot
degrees of the groups.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from plaid_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plaid_amd", "csrc")


def _probe(g, Gp, Gi, flex=1):
    fn = _lib.load().plaidhip_debug_pair_flex_probe
    fn.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_void_p,
                   C.c_int64]
    fn.restype = C.c_int
    out = (C.c_int64 * 16)()
    cap = 64 * 96 * 3
    pairs = np.full((cap, 4), -9, dtype=np.int32)
    Gp = np.ascontiguousarray(Gp, dtype=np.int32)
    Gi = np.ascontiguousarray(Gi, dtype=np.int32)
    assert fn(g, len(Gp) - 1, Gp.ctypes.data, Gi.ctypes.data, 16, flex, out, pairs.ctypes.data, cap) == 0
    keys = ("slices", "chunks", "found", "double_booked", "wrong", "regp", "most_tiles", "waves", "slots", "pairs", "broken",
            "plan_us", "flex")
    d = dict(zip(keys, (int(v) for v in out)))
    d["list"] = pairs[:d["pairs"]].copy()
    return d


def _self_check(g, Gp, Gi):
    """every membership scheduled exactly once, own or guest; a read on a flex step of a host lane belongs to the host's
    owner and every other read to the lane's own set (so no host has an own gene on a flex step and no guest gene sits on a
    normal step: either would count as wrong); owner <-> host one to one inside a tile, overflow <= T/8 and above 0, host
    length <= 7T/8 (any breach counts as broken)"""
    d = _probe(g, Gp, Gi)
    z = int(Gp[-1])
    assert d["found"] == z and d["wrong"] == 0 and d["broken"] == 0, d
    if d["pairs"]:
        assert d["regp"] == 1 and d["flex"] == 1
        lst = d["list"]
        m = len(Gp) - 1
        assert np.all((lst[:, 1] >= 0) & (lst[:, 1] < m) & (lst[:, 2] < m) & (lst[:, 3] >= 0) & (lst[:, 3] < g))
        for s in np.unique(lst[:, 0]):      # one host per owner and one owner per host in a slice (hosts without a set: -1)
            one = lst[lst[:, 0] == s]
            assert len(np.unique(one[:, 1])) == len(one)
            hosts = one[one[:, 2] >= 0][:, 2]
            assert len(np.unique(hosts)) == len(hosts)
            assert not set(one[:, 1]) & set(hosts)
    d0 = _probe(g, Gp, Gi, flex=0)
    assert d0["found"] == z and d0["wrong"] == 0 and d0["pairs"] == 0 and d["slots"] <= d0["slots"]
    return d, d0


@pytest.fixture(scope="module")
def c2():
    Gp, Gi = synth.geneset_csc(20000, 5000)
    return (Gp, Gi) + _self_check(20000, Gp, Gi)


def test_benchmark_collection_slots_and_double_booked_reads(c2):
    """at most 810,000 slots (861,696 without flex steps) and no more double-booked reads than without them"""
    _, _, d, d0 = c2
    print("slots", d["slots"], "without flex steps", d0["slots"], "double-booked", d["double_booked"], "without", d0["double_booked"])
    assert d0["slots"] == 861696
    assert d["slots"] <= 810000
    assert d["double_booked"] <= d0["double_booked"]


def test_benchmark_collection_prepare_time(c2, tmp_path):
    """preparing the collection (`make plan-probe`: plaidhip_geneset_create, all plans) stays under twice what it takes
    without flex steps -- this build's time less what the pair plan's flex steps add, the difference of the two pair-plan
    builds the same probe times (best of three each)"""
    import json
    Gp, Gi = c2[0], c2[1]
    out = subprocess.run(["make", "-C", CSRC, "plan-probe"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    path = str(tmp_path / "gs.bin")
    with open(path, "wb") as f:
        f.write(np.array([20000, 5000], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(Gp, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(Gi, dtype=np.int32).tobytes())
    best = None
    for _ in range(3):
        r = subprocess.run([os.path.join(CSRC, "diag", "plan_probe"), path, "check"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        d = json.loads(r.stdout)
        assert d["flex_slots"] == c2[2]["slots"] and d["noflex_slots"] == c2[3]["slots"] and d["flex_broken"] == 0
        assert d["flex_double_booked"] == c2[2]["double_booked"] and d["flex_pairs"] == c2[2]["pairs"]
        if best is None or d["create_s"] < best["create_s"]:
            best = d
    added = max(0.0, 1e-6 * (best["flex_plan_us"] - best["noflex_plan_us"]))
    print("create_s", best["create_s"], "pair plan us with / without flex steps", best["flex_plan_us"], best["noflex_plan_us"])
    assert best["create_s"] < 2 * (best["create_s"] - added)


@pytest.mark.parametrize("g,m,kw", [(500, 70, {}), (10224, 300, {}), (10225, 130, {}), (20000, 700, {}), (30001, 200, {}),
                                    (20000, 6144, {"kmax": 40}), (20000, 6145, {"kmax": 40})])
def test_small_collections(g, m, kw):
    """one to three slices, plans that are not register-partial (one slice; 6,145 sets) and so get no flex steps"""
    kw = dict({"kmin": 1, "kmax": min(g, 400), "sort_by_size": False}, **kw)
    Gp, Gi = synth.geneset_csc(g, m, **kw)
    d, d0 = _self_check(g, Gp, Gi)
    if not (g > 10224 and (m + 63) // 64 <= 96):
        assert d["pairs"] == 0 and d["slots"] == d0["slots"] and d["flex"] == 0


def test_reference_shaped_collection():
    """sizes 3 ... 5,000 and an all-genes set, Zipf gene popularity, duplicated sets (synth.geneset_csc_real)"""
    Gp, Gi = synth.geneset_csc_real(25000, 3000)
    d, d0 = _self_check(25000, Gp, Gi)
    assert d["pairs"] > 0 and d["slots"] < d0["slots"]


def test_self_check_stand_alone_under_asan_and_ubsan(tmp_path):
    """the same self-check as a program of its own, geneset.cpp compiled with -fsanitize=address,undefined
    (`make host-asan-flex`), on its built-in collections, the benchmark's and the reference-shaped one"""
    files = []
    for name, (g, m, gen) in {"c2": (20000, 5000, synth.geneset_csc), "real": (25000, 3000, synth.geneset_csc_real)}.items():
        Gp, Gi = gen(g, m)
        path = str(tmp_path / (name + ".bin"))
        with open(path, "wb") as f:
            f.write(np.array([g, m], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(Gp, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(Gi, dtype=np.int32).tobytes())
        files.append(path)
    for args in ("", " ".join(files)):
        out = subprocess.run(["make", "-C", CSRC, "host-asan-flex", "ARGS=" + args], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "[host-asan-flex] ok" in out.stdout
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
