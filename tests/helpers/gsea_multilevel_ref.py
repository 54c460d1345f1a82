"""Host restatement of plaid.gsea's multilevel p-values as include/plaidhip.h pins them (plaidhip_gsea_multilevel,
plaidhip_gsea_ruler), on top of tests/helpers/gsea_perm_ref.py and gsea_edge_ref.py.

run_ruler is the statement itself in two forms that give the same trace: the literal one takes a slot and a proposal at a
time with gsea_perm_ref.philox4x32_10 and gsea_edge_ref.extremes_numpy; the fast one takes all n slots of a proposal step
at once (the slots of one stage do not see each other) with the same element-wise IEEE operations and the same sequential
cumsum along each state.  read_off, table and all_scores complete it: a set's row, a whole call, and the exhaustive
enumeration the estimator is held to."""
import itertools
import math

import numpy as np

from . import gsea_edge_ref as edge
from . import gsea_perm_ref as ref

MAX_STAGES = 256          # PLAIDHIP_GSEA_ML_MAX_STAGES
MAX_SAMPLE = 1023         # PLAIDHIP_GSEA_ML_MAX_SAMPLE
ESTIMATED, FLOOR, STALLED = 0, 1, 2
STATUS = {ESTIMATED: "estimated", FLOOR: "floor", STALLED: "stalled"}
ML_COLUMNS = ("pvalML", "log2err", "stage", "status", "qhat", "denom")
M32 = ref.M32


def tag_of(l, side):
    return 0x80000000 | (int(l) << 1) | int(side)


def below(o, R):
    """an integer in 0..R-1 from a 32-bit word"""
    return (int(o) * int(R)) >> 32


def key_of(seed):
    return int(seed) & M32, (int(seed) >> 32) & M32


def side_of(score_type, es):
    """0 positive, 1 negative, None: no ruler"""
    if es != es:
        return None
    if score_type == edge.POS:
        return 0
    if score_type == edge.NEG:
        return 1
    return 0 if es > 0.0 else (1 if es < 0.0 else None)


# ---- Philox over arrays of counters -------------------------------------------------------------------------------------------
def philox_columns(c0, c1, c2, c3, key):
    """the four output words for arrays of counter words (uint64 arrays holding 32-bit values; scalars broadcast)"""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)))
    k0, k1 = key
    m, s32 = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


# ---- h(S) -----------------------------------------------------------------------------------------------------------------------
def h_literal(positions, Wpos, score_type, side):
    """h of the state whose members stand at `positions` (0-based), by gsea_edge_ref.extremes_numpy on the identity placement"""
    N = len(Wpos)
    ex = edge.extremes_numpy(np.arange(N, dtype=np.int32), np.asarray(positions, dtype=np.int64), Wpos)
    es = edge.es_of(ex, score_type)
    return -es if side else es


def h_rows(pos, Wpos, score_type, side):
    """h of every row of pos (r x k sorted 0-based positions): extremes_numpy's operations, row by row at once"""
    r, k = pos.shape
    N = len(Wpos)
    p = pos.astype(np.int64) + 1
    cw = np.cumsum(Wpos[pos], axis=1)
    zero = cw[:, -1] == 0.0
    t = np.arange(1, k + 1, dtype=np.int64)[None, :]
    cw = np.where(zero[:, None], t.astype(np.float64), cw)
    B = np.where(zero, float(k), cw[:, -1])[:, None]
    miss = (p - t).astype(np.float64) / float(N - k)
    maxP = (cw / B - miss).max(axis=1)
    minP = (np.concatenate([np.zeros((r, 1)), cw[:, :-1]], axis=1) / B - miss).min(axis=1)
    if score_type == edge.POS:
        es = maxP
    elif score_type == edge.NEG:
        es = minP
    else:
        es = np.where(maxP > -minP, maxP, np.where(maxP < -minP, minP, 0.0))
    return -es if side else es


# ---- the initial states ---------------------------------------------------------------------------------------------------------
def initial_state(N, k, slot, l, side, seed):
    """the sorted positions of S_slot: the first min(k, N - k) distinct draws, or their complement when 2 k > N"""
    key, tag = key_of(seed), tag_of(l, side)
    target = min(k, N - k)
    T0, d, words = set(), 0, None
    while len(T0) < target:
        if d & 3 == 0:
            words = ref.philox4x32_10((0x80000000 | (d >> 2), slot, k, tag), key)
        T0.add(below(words[d & 3], N))
        d += 1
    return np.array(sorted(T0 if 2 * k <= N else set(range(N)) - T0), dtype=np.int64)


# ---- one ruler ------------------------------------------------------------------------------------------------------------------
def run_ruler(Wpos, k, l, side, score_type, gamma_max, seed, n=101, sweeps=4, eps=1e-50, fast=True):
    """the trace of one ruler run to gamma_max: {"stages", "status", "m", "s", "h" (stages x n), "gap"}.  gap: the smallest
    distance the run met between two values it compared -- a proposal's score and the level, two scores of one stage, a
    level and gamma_max -- that belong to DIFFERENT states (0.0 where two different states had one score): roundings below
    half of it cannot change the discrete trace.  Equal scores of one and the same state (a proposal that lands on the
    state the level came from, copies of a survivor) do not count: a score is a function of the state alone, here and on
    the device, so they are equal there too."""
    Wpos = np.asarray(Wpos, dtype=np.float64)
    N = len(Wpos)
    assert n % 2 == 1 and 3 <= n <= MAX_SAMPLE and 1 <= sweeps <= 32 and 1 <= k < N
    key, tag = key_of(seed), tag_of(l, side)
    M = np.zeros((n, N), dtype=bool)
    for i in range(n):
        M[i, initial_state(N, k, i, l, side, seed)] = True
    rows_of = lambda A: np.nonzero(A)[1].reshape(A.shape[0], k)
    h = h_rows(rows_of(M), Wpos, score_type, side)
    if not fast:
        assert all(h[i] == h_literal(np.flatnonzero(M[i]), Wpos, score_type, side) for i in range(n))
    ms, ss, hs, gap, P, status = [], [], [], math.inf, 1.0, None
    T = sweeps * k
    for stage in range(MAX_STAGES):
        m = float(np.sort(h)[(n + 1) // 2 - 1])
        s = int(np.sum(h > m))
        ms.append(m)
        ss.append(s)
        hs.append(h.copy())
        u, first, inv = np.unique(h, return_index=True, return_inverse=True)
        if len(u) > 1:
            gap = min(gap, float(np.min(np.diff(u))))
        if not np.array_equal(M, M[first[inv]]):      # two different states with one score
            gap = 0.0
        level_states = {M[i].tobytes() for i in np.flatnonzero(h == m)}
        if m != gamma_max:
            gap = min(gap, abs(m - gamma_max))
        if m >= gamma_max:
            status = ESTIMATED
            break
        if s == 0:
            status = STALLED
            break
        P = P * (float(s) / float(n))
        if P < eps or stage + 1 == MAX_STAGES:
            status = FLOOR
            break
        surv = np.flatnonzero(h > m)
        for j, i in enumerate(np.flatnonzero(h <= m)):
            M[i], h[i] = M[surv[j % s]], h[surv[j % s]]
        assert (stage + 1) * T < 2 ** 31
        if fast:
            slots = np.arange(n, dtype=np.uint64)
            for step in range(T):
                o0, o1, _, _ = philox_columns(stage * T + step, slots, k, tag, key)
                a = ((o0 * np.uint64(k)) >> np.uint64(32)).astype(np.int64)
                b = ((o1 * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
                idx = np.flatnonzero(~M[np.arange(n), b])
                if len(idx) == 0:
                    continue
                pa = rows_of(M[idx])[np.arange(len(idx)), a[idx]]
                M2 = M[idx].copy()
                M2[np.arange(len(idx)), pa] = False
                M2[np.arange(len(idx)), b[idx]] = True
                h2 = h_rows(rows_of(M2), Wpos, score_type, side)
                again = np.array([h2[q] == m and M2[q].tobytes() in level_states for q in range(len(idx))])
                if not again.all():
                    gap = min(gap, float(np.min(np.abs(h2[~again] - m))))
                ok = h2 > m
                M[idx[ok]], h[idx[ok]] = M2[ok], h2[ok]
        else:
            for i in range(n):
                for step in range(T):
                    o = ref.philox4x32_10((stage * T + step, i, k, tag), key)
                    a, b = below(o[0], k), below(o[1], N)
                    if M[i, b]:
                        continue
                    pa = np.flatnonzero(M[i])[a]
                    M[i, pa], M[i, b] = False, True
                    h2 = h_literal(np.flatnonzero(M[i]), Wpos, score_type, side)
                    if not (h2 == m and M[i].tobytes() in level_states):
                        gap = min(gap, abs(h2 - m))
                    if h2 > m:
                        h[i] = h2
                    else:
                        M[i, pa], M[i, b] = True, False
    return {"stages": len(ms), "status": status, "m": np.array(ms), "s": np.array(ss, dtype=np.int32), "h": np.array(hs),
            "gap": gap}


def read_off(trace, gamma):
    """(qhat, log2err, stage, status, c) of a set with target gamma from its ruler's trace"""
    n = trace["h"].shape[1]
    hit = np.flatnonzero(trace["m"] >= gamma)
    lstar = int(hit[0]) if len(hit) else trace["stages"] - 1
    status = ESTIMATED if len(hit) else trace["status"]
    c = int(np.sum(trace["h"][lstar] >= gamma))
    c1 = max(c, 1)
    P, total = 1.0, 0.0
    for j in range(lstar):
        s = int(trace["s"][j])
        P = P * (float(s) / float(n))
        total = total + float(n - s) / (float(n) * float(s))
    qhat = P * (float(c1) / float(n))
    total = total + float(n - c1) / (float(n) * float(c1))
    return qhat, math.sqrt(total) / math.log(2.0), lstar, status, c


# ---- a whole call ---------------------------------------------------------------------------------------------------------------
def table(stat, weight, Gp, Gi, P, seed, score_type=edge.STD, n=101, sweeps=4, eps=1e-50, ml_min=10):
    """(out m x 12 x c, ml m x 6 x c, null m x B x c) of plaidhip_gsea_multilevel for placements P (g x B).  Every set is run
    on a ruler of its own to its own target: by the pinned form a row does not depend on the sets that share its ruler."""
    stat = np.asarray(stat, dtype=np.float64).reshape(len(stat), -1)
    weight = np.asarray(weight, dtype=np.float64).reshape(stat.shape)
    out, null, _, _ = edge.gsea_scored_ref(stat, weight, Gp, Gi, P)[score_type]
    out = out.copy(order="F")
    m, c, B = len(Gp) - 1, stat.shape[1], P.shape[1]
    ml = np.full((m, 6, c), np.nan, order="F")
    for l in range(c):
        if not np.all(np.isfinite(stat[:, l])):
            continue
        Wpos = ref.walk_weights(ref.observed_placement(stat[:, l]), weight[:, l])
        for j in range(m):
            es = out[j, 0, l]
            side = side_of(score_type, es)
            if side is None:
                continue
            k = int(Gp[j + 1] - Gp[j])
            tr = run_ruler(Wpos, k, l, side, score_type, abs(es), seed, n, sweeps, eps)
            qhat, log2err, lstar, status, _ = read_off(tr, abs(es))
            denom = (1.0 + out[j, 8 if side == 0 else 9, l]) / (1.0 + float(B))
            ml[j, :, l] = min(1.0, qhat / denom), log2err, lstar, status, qhat, denom
            if out[j, 4, l] < ml_min:
                out[j, 2, l] = ml[j, 0, l]
        out[:, 3, l] = ref.bh(out[:, 2, l])
    return out, ml, null


# ---- exhaustive enumeration -----------------------------------------------------------------------------------------------------
def all_scores(Wpos, k, score_type, side, chunk=200000):
    """h of every k-subset of the positions, in chunks"""
    N = len(Wpos)
    res = []
    it = itertools.combinations(range(N), k)
    while True:
        block = np.fromiter(itertools.chain.from_iterable(itertools.islice(it, chunk)), dtype=np.int64)
        if len(block) == 0:
            break
        res.append(h_rows(block.reshape(-1, k), Wpos, score_type, side))
    return np.concatenate(res)


# ---- the cases of the tests -----------------------------------------------------------------------------------------------------
def ruler_case(N, k, score_type, side, weights, data_seed):
    """(stat, weight, Wpos, gamma) of one ruler test: a normal draw; weights "unit", "int" (integers below 2^20: every walk
    has host bits) or "abs" (|stat|); gamma = the score of the k genes at the side's end of the list"""
    rng = np.random.default_rng(data_seed)
    stat = rng.standard_normal(N)
    weight = {"unit": np.ones(N), "int": rng.integers(1, 1 << 20, N).astype(np.float64), "abs": np.abs(stat)}[weights]
    Wpos = ref.walk_weights(ref.observed_placement(stat), weight)
    top = np.arange(k) if side == 0 else np.arange(N - k, N)
    return stat, weight, Wpos, float(h_literal(top, Wpos, score_type, side))


# the rulers whose restatement takes minutes (k next to N = 4097: thousands of proposals a stage over thousands of members):
# their traces are recorded in tests/golden/gsea_ml_traces.npz by `python -m tests.helpers.gsea_multilevel_ref`
GOLDEN_RULERS = (   # N, k, score type, side, weights, data seed, chain seed, n, sweeps
    (4097, 4094, edge.STD, 0, "int", 11, 5, 5, 1),
    (4097, 4096, edge.STD, 1, "unit", 12, 6, 5, 1),
    (4097, 4094, edge.NEG, 1, "unit", 13, 7, 5, 1),
    (4097, 4096, edge.POS, 0, "int", 14, 8, 5, 1),
)


def golden_key(case):
    return "N%d_k%d_st%d_side%d_%s_d%d_c%d_n%d_sw%d" % case


if __name__ == "__main__":   # records the golden traces
    import os
    out = {}
    for case in GOLDEN_RULERS:
        N, k, st, side, weights, dseed, cseed, n, sweeps = case
        _, _, Wpos, gamma = ruler_case(N, k, st, side, weights, dseed)
        tr = run_ruler(Wpos, k, 3, side, st, gamma, cseed, n, sweeps, 1e-50)
        key = golden_key(case)
        out[key + "_m"], out[key + "_s"], out[key + "_h"] = tr["m"], tr["s"], tr["h"]
        out[key + "_status"] = np.array([tr["status"]])
        print(key, tr["stages"], tr["status"], flush=True)
    np.savez_compressed(os.path.join(os.path.dirname(__file__), "..", "golden", "gsea_ml_traces.npz"), **out)
