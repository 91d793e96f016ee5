"""The definition of po_agentsets_batch (include/po_hip.h) in numpy: per ego path, the records of its pool of two source lists that are
not its own and that come near the path in space and in time, in the po_agent_lists layout the moving-obstacle stages read.

Tests only.  One ufunc per operation of the definition, in the order it writes them, so every compared value is the same rounded IEEE double the kernel
compares; comparisons against this file are bit equality.  The vectors run over the CANDIDATES of one ego; egos and sources are Python loops
(tests/test_agentsets.py checks this file against a scalar loop).  Minima and maxima are numpy's reductions: over finite values any order gives the same
value, and a record with a non-finite point is dropped whatever its minimum is."""
import numpy as np

HOLD_BEFORE, HOLD_AFTER, MAX_PTS = 1, 2, 8
AGENT_DTYPE = np.dtype([("n_pts", np.int32), ("flags", np.int32), ("radius", np.float64), ("t", np.float64, (8,)), ("x", np.float64, (8,)), ("y", np.float64, (8,))])
INF = np.float64(np.inf)


def clamp(v, hi):
    return min(max(int(v), 0), hi)


def ego_box(st, t, okb, ap):
    """(exl, exh, eyl, eyh, W0, W1) of ONE ego: st [n, 5], t [n] or None; None when the ego is not composed."""
    n = len(st)
    if okb == 0 or n < 1 or not (np.isfinite(st[:, 0]).all() and np.isfinite(st[:, 1]).all()):
        return None
    if t is not None and not np.isfinite(t).all():
        return None
    with np.errstate(all="ignore"):
        if t is None:
            W0, W1 = np.float64(ap.win_lo), np.float64(ap.win_hi)
        else:
            W0, W1 = t.min() - np.float64(ap.t_before), t.max() + np.float64(ap.t_after)
    return st[:, 0].min(), st[:, 0].max(), st[:, 1].min(), st[:, 1].max(), W0, W1


def pool_range(first, n_agents, pool_b):
    """[lo, hi) of one source for an ego: agent_set_range's clamps."""
    S = len(first) - 1
    if S < 1 or n_agents < 1:
        return 0, 0
    k = clamp(pool_b, S - 1)
    return clamp(first[k], n_agents), clamp(first[k + 1], n_agents)


def keep_mask(rec, idx, box, ap, b, owners):
    """Which of the candidate records rec (their indices idx into the source array) ego b keeps.  owners: None (source 1, or nobody owns anything) or the owner of
    every candidate."""
    exl, exh, eyl, eyh, W0, W1 = box
    np_ = rec["n_pts"]
    live = np.arange(MAX_PTS)[None, :] < np_[:, None]
    T, X, Y, R = rec["t"], rec["x"], rec["y"], rec["radius"]
    with np.errstate(all="ignore"):
        covers = (np_ >= 1) & (np_ <= MAX_PTS) & (R >= 0)
        covers &= (np.isfinite(T) | ~live).all(axis=1) & (np.isfinite(X) | ~live).all(axis=1) & (np.isfinite(Y) | ~live).all(axis=1)
        A0 = np.where(live, T, INF).min(axis=1)
        A1 = np.where(live, T, -INF).max(axis=1)
        A0 = np.where(rec["flags"] & HOLD_BEFORE, -INF, A0)
        A1 = np.where(rec["flags"] & HOLD_AFTER, INF, A1)
        in_time = (A0 <= W1) & (A1 >= W0)
        rr = R + np.float64(ap.reach)
        axl, axh = np.where(live, X, INF).min(axis=1), np.where(live, X, -INF).max(axis=1)
        ayl, ayh = np.where(live, Y, INF).min(axis=1), np.where(live, Y, -INF).max(axis=1)
        in_space = (axl - rr <= exh) & (axh + rr >= exl) & (ayl - rr <= eyh) & (ayh + rr >= eyl)
    keep = covers & in_time & in_space
    if owners is not None:
        keep &= owners != b
    return keep


def owners_of(idx, owner, owner_div):
    """The owner of the records idx of source 0 (int64), or None when nobody owns anything."""
    if owner is not None:
        return np.asarray(owner, dtype=np.int64)[idx]
    if owner_div > 0:
        return idx // owner_div
    return None


def compose(states, t, sources, ap, n_states=None, ok=None, pool_of=None, owner=None, capacity=None, fill_byte=0, fill_index=0):
    """po_agentsets_batch on host arrays.  sources: [(agents, first)] or [(agents, first), (agents1, first1) or None], as binding.pack_agents returns them
    (unvalidated: read as the device entry reads them).  capacity None: exactly total.  The slots the stage does not write hold fill_byte / fill_index.  Returns the
    dict Engine.agentsets_batch returns, plus kept: the list per ego of the src_index values of its FULL set."""
    states = np.asarray(states, dtype=np.float64)
    B, N = states.shape[0], states.shape[1]
    srcs = [s for s in sources]
    n0 = len(srcs[0][0])
    count, status, kept = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), []
    for b in range(B):
        n = N if n_states is None else clamp(n_states[b], N)
        box = ego_box(states[b, :n], None if t is None else np.asarray(t, dtype=np.float64)[b, :n], 1 if ok is None else int(ok[b]), ap)
        mine = []
        if box is not None:
            status[b] = 1
            for s, src in enumerate(srcs[:2]):
                if src is None:
                    continue
                agents, first = src
                lo, hi = pool_range(first, len(agents), 0 if pool_of is None else pool_of[b])
                if hi <= lo:
                    continue
                idx = np.arange(lo, hi, dtype=np.int64)
                keep = keep_mask(agents[lo:hi], idx, box, ap, b, owners_of(idx, owner, int(ap.owner_div)) if s == 0 else None)
                mine += [(s, int(a)) for a in idx[keep]]
        kept.append(mine)
        count[b] = len(mine)
    F = np.concatenate(([0], np.cumsum(count.astype(np.int64))))
    total = int(F[-1])
    cap = total if capacity is None else int(capacity)
    r = {"agents": np.full(cap * AGENT_DTYPE.itemsize, fill_byte, dtype=np.uint8).view(AGENT_DTYPE), "first": np.minimum(F, cap).astype(np.int32), "count": count,
         "status": status, "set_of": np.arange(B, dtype=np.int32), "src_index": np.full(cap, fill_index, dtype=np.int32), "total": total, "capacity": cap,
         "kept": [[a if s == 0 else n0 + a for s, a in mine] for mine in kept]}
    for b in range(B):
        if status[b] and F[b] + count[b] > cap:
            status[b] = 2
        for q, (s, a) in enumerate(kept[b]):
            p = int(F[b]) + q
            if p < cap:
                r["agents"][p] = srcs[s][0][a]
                r["src_index"][p] = a if s == 0 else n0 + a
    return r
