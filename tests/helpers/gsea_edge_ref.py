"""Host restatements of plaid.gsea's score types and leading edges as include/plaidhip.h pins them (plaidhip_gsea_scored;
DESIGN.md section 18), on top of tests/helpers/gsea_perm_ref.py.

Three forms of the extremes of one set under one placement -- maxP, minP and the first t at which each is met -- a
vectorised numpy form (argmax / argmin: the reference of the GPU tests), a literal member-by-member loop with strict
updates, and the same operations in exact integers over one denominator (fractions.Fraction); from the extremes, ES and the
edge of each score type; and the 12 columns, null matrix and edge buffers of a whole call."""
from fractions import Fraction

import numpy as np

from . import gsea_perm_ref as ref

STD, POS, NEG = 0, 1, 2
SCORE_TYPES = {"std": STD, "pos": POS, "neg": NEG}


def walk_order(pos, members):
    """the set's rows in walk order (increasing position), and their 1-based positions p_1 < ... < p_k"""
    members = np.asarray(members, dtype=np.int64)
    o = np.argsort(pos[members].astype(np.int64), kind="stable")
    return members[o], pos[members[o]].astype(np.int64) + 1


# ---- the extremes, three ways: (maxP, minP, t_top, t_bot), t 1-based; None for k = 0 or k = N --------------------------------
def extremes_numpy(pos, members, Wpos):
    """the operations of gsea_perm_ref.es_numpy; argmax / argmin return the first occurrence, as which.max / which.min"""
    N, k = len(pos), len(members)
    if k == 0 or k == N:
        return None
    _, p = walk_order(pos, members)
    cw = np.cumsum(Wpos[p - 1])
    B = cw[-1]
    if B == 0.0:
        cw = np.arange(1, k + 1, dtype=np.float64)
        B = float(k)
    t = np.arange(1, k + 1, dtype=np.int64)
    miss = (p - t).astype(np.float64) / float(N - k)
    after = cw / B - miss
    before = np.concatenate([[0.0], cw[:-1]]) / B - miss
    return float(after.max()), float(before.min()), int(np.argmax(after)) + 1, int(np.argmin(before)) + 1


def extremes_numpy_columns(P, members, Wpos):
    """extremes_numpy for every column of P (g x B placements) at once: the same element-wise IEEE operations and the same
    sequential cumsum down each column, so the same bits.  Returns four arrays of length B, or None for k = 0 or k = N"""
    N, k = P.shape[0], len(members)
    if k == 0 or k == N:
        return None
    p = np.sort(P[np.asarray(members, dtype=np.int64), :].astype(np.int64), axis=0) + 1      # k x B
    cw = np.cumsum(Wpos[p - 1], axis=0)
    zero = cw[-1, :] == 0.0
    t = np.arange(1, k + 1, dtype=np.int64)[:, None]
    cw = np.where(zero[None, :], t.astype(np.float64), cw)
    B = np.where(zero, float(k), cw[-1, :])[None, :]
    miss = (p - t).astype(np.float64) / float(N - k)
    after = cw / B - miss
    before = np.concatenate([np.zeros((1, P.shape[1])), cw[:-1, :]], axis=0) / B - miss
    return after.max(axis=0), before.min(axis=0), np.argmax(after, axis=0) + 1, np.argmin(before, axis=0) + 1


def extremes_literal(pos, members, Wpos):
    """member by member; an extreme moves only on a strictly larger (smaller) value, so the first occurrence stays"""
    N, k = len(pos), len(members)
    if k == 0 or k == N:
        return None
    _, p = walk_order(pos, members)
    B = 0.0
    for q in p:
        B = B + float(Wpos[q - 1])
    unweighted = B == 0.0
    if unweighted:
        B = float(k)
    cw, maxP, minP, t_top, t_bot = 0.0, -np.inf, np.inf, 0, 0
    for t in range(1, k + 1):
        q = int(p[t - 1])
        prev = cw
        cw = float(t) if unweighted else cw + float(Wpos[q - 1])
        miss = float(q - t) / float(N - k)
        after, before = cw / B - miss, prev / B - miss
        if after > maxP:
            maxP, t_top = after, t
        if before < minP:
            minP, t_bot = before, t
    return float(maxP), float(minP), t_top, t_bot


def extremes_fraction(pos, members, Wpos, gaps=False):
    """exact: every candidate over the one denominator B (N - k), so the extremes and their first places are found among
    integers.  gaps: also (gap_top, gap_bot), the distance from each extreme to the nearest candidate at another t (a
    Fraction; None where k = 1) -- 0 where the extreme is met twice"""
    N, k = len(pos), len(members)
    if k == 0 or k == N:
        return None
    _, p = walk_order(pos, members)
    p = [int(x) for x in p]
    w = [Fraction(float(x)) for x in Wpos[np.asarray(p) - 1]]
    scale = max(f.denominator for f in w)
    wi = [f.numerator * (scale // f.denominator) for f in w]
    B = sum(wi)
    if B == 0:
        wi, B = [1] * k, k
    D = N - k
    cw, after, before = 0, [], []
    for t in range(1, k + 1):
        miss = (p[t - 1] - t) * B
        before.append(cw * D - miss)
        cw += wi[t - 1]
        after.append(cw * D - miss)
    mx, mn = max(after), min(before)
    t_top, t_bot = after.index(mx) + 1, before.index(mn) + 1
    res = (Fraction(mx, B * D), Fraction(mn, B * D), t_top, t_bot)
    if not gaps:
        return res
    if k == 1:
        return res + (None, None)
    g_top = mx - max(a for t, a in enumerate(after, 1) if t != t_top)
    g_bot = min(b for t, b in enumerate(before, 1) if t != t_bot) - mn
    return res + (Fraction(g_top, B * D), Fraction(g_bot, B * D))


# ---- ES and the edge from the extremes ----------------------------------------------------------------------------------------
def branch(maxP, minP, score_type):
    """+1 the top branch, -1 the bottom branch, 0 none"""
    if score_type == POS:
        return 1
    if score_type == NEG:
        return -1
    return 1 if maxP > -minP else (-1 if maxP < -minP else 0)


def es_of(ex, score_type, zero=0.0, nan=float("nan")):
    if ex is None:
        return nan
    maxP, minP = ex[0], ex[1]
    if score_type == POS:
        return maxP
    if score_type == NEG:
        return minP
    return maxP if maxP > -minP else (minP if maxP < -minP else zero)


def edge_of(ex, pos, members, score_type):
    """the rows of the leading edge in the pinned order (a list; empty for a NaN pair or a std tie)"""
    if ex is None:
        return []
    rows, _ = walk_order(pos, members)
    k = len(rows)
    b = branch(ex[0], ex[1], score_type)
    if b > 0:
        return [int(r) for r in rows[:ex[2]]]                       # t = 1 .. t_top
    if b < 0:
        return [int(r) for r in rows[ex[3] - 1:k][::-1]]            # t = k .. t_bot
    return []


def edge_is_decided(ex, score_type, bound):
    """whether roundings of at most `bound` per candidate cannot move the edge of a pair whose rational extremes and gaps
    are ex (extremes_fraction(..., gaps=True)): the branch's runner-up lies further than twice the bound from its extreme
    and, for std, so does maxP from -minP"""
    if ex is None:
        return True
    b = branch(ex[0], ex[1], score_type)
    if b == 0 or (score_type == STD and abs(ex[0] + ex[1]) <= 2 * bound):
        return False
    gap = ex[4] if b > 0 else ex[5]
    return gap is None or gap > 2 * bound


def score_and_edge(pos, members, Wpos, score_type, form=extremes_numpy):
    """(ES, edge) of one set under one placement by one of the three forms (the Fraction form: ES a Fraction or None)"""
    ex = form(pos, members, Wpos)
    if form is extremes_fraction:
        return (None if ex is None else es_of(ex, score_type, Fraction(0))), edge_of(ex, pos, members, score_type)
    return es_of(ex, score_type), edge_of(ex, pos, members, score_type)


# ---- a whole call ---------------------------------------------------------------------------------------------------------------
def null_stats(es, null, score_type):
    """gsea_perm_ref.null_stats (the six partials in the pinned order; NES, pval, nMoreExtreme of std), with the three
    columns that depend on the score type redone for pos / neg"""
    out = ref.null_stats(es, null)
    if es != es or score_type == STD:
        return out
    n_ge, n_le, n_ge0, n_le0, sum_pos, sum_neg = (np.float64(x) for x in out[6:])
    d = np.float64
    with np.errstate(divide="ignore", invalid="ignore"):
        if score_type == POS:
            out[1], out[2], out[4] = d(es) / (sum_pos / n_ge0), (d(1.0) + n_ge) / (d(1.0) + n_ge0), n_ge
        else:
            out[1], out[2], out[4] = d(es) / np.abs(sum_neg / n_le0), (d(1.0) + n_le) / (d(1.0) + n_le0), n_le
    return out


def gsea_scored_ref(stat, weight, Gp, Gi, P, form=extremes_numpy):
    """{score type: (out m x 12 x c, null m x B x c, le_len m x c, le_idx nnz x c)} of plaidhip_gsea_scored for placements P
    (g x B): every walk is taken once and serves the three score types"""
    stat = np.asarray(stat, dtype=np.float64).reshape(len(stat), -1)
    weight = np.asarray(weight, dtype=np.float64).reshape(stat.shape)
    g, c = stat.shape
    m, B, nnz = len(Gp) - 1, P.shape[1], int(Gp[-1])
    res = {}
    for st in (STD, POS, NEG):
        out = np.full((m, 12, c), np.nan, order="F")
        for j in range(m):
            out[j, 5, :] = Gp[j + 1] - Gp[j]
        res[st] = (out, np.full((m, B, c), np.nan, order="F"), np.zeros((m, c), dtype=np.int32, order="F"),
                   np.full((nnz, c), -1, dtype=np.int32, order="F"))
    for l in range(c):
        if not np.all(np.isfinite(stat[:, l])):
            continue
        pos = ref.observed_placement(stat[:, l])
        Wpos = ref.walk_weights(pos, weight[:, l])
        for j in range(m):
            mem = np.asarray(Gi[Gp[j]:Gp[j + 1]], dtype=np.int64)
            ex = form(pos, mem, Wpos)
            if ex is None:
                continue
            if form is extremes_numpy:
                exb = list(zip(*extremes_numpy_columns(P, mem, Wpos)))
            else:
                exb = [form(P[:, b], mem, Wpos) for b in range(B)]
            for st in (STD, POS, NEG):
                out, null, le_len, le_idx = res[st]
                null[j, :, l] = [es_of(e, st) for e in exb]
                size = out[j, 5, l]
                out[j, :, l] = null_stats(es_of(ex, st), null[j, :, l], st)
                out[j, 5, l] = size
                edge = edge_of(ex, pos, mem, st)
                le_len[j, l] = len(edge)
                le_idx[Gp[j]:Gp[j] + len(edge), l] = edge
        for st in (STD, POS, NEG):
            res[st][0][:, 3, l] = ref.bh(res[st][0][:, 2, l])
    return res


def edges_of(le_len, le_idx, Gp, l=0):
    """the edge buffers of list l as a list of lists"""
    return [[int(r) for r in le_idx[Gp[j]:Gp[j] + le_len[j, l], l]] for j in range(len(Gp) - 1)]


def odd_positions_set(N):
    """the rows at walk positions 1, 3, 5, ... of a list whose statistic decreases with the row (N even, k = N / 2): with
    unit weights after_t = t / k - (t - 1) / k = 1 / k and before_t = 0 for every t, exactly when N is a power of two"""
    return np.arange(0, N, 2, dtype=np.int32)
