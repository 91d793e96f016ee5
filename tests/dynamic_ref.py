"""The definition of po_dynamic_batch (include/po_hip.h) in numpy: timed paths against moving agents -> gaps, the first conflict, v_limit rows.

Tests only.  One ufunc per operation of the definition, in the order it writes them, so every value is the same sequence of rounded IEEE double operations the
kernel runs; comparisons against this file are bit equality.  The vectors run over the INTERVALS of one path; agents, pieces and circles are Python loops in the
definition's order (tests/test_dynamic.py checks this file against a scalar loop).  Circle centres: select_ref's footprint circles and portable sin / cos."""
import numpy as np

import select_ref
from select_ref import DBL_MAX, vmax, vmin

HOLD_BEFORE, HOLD_AFTER, MAX_PTS = 1, 2, 8


def centres(params, st):
    """gx, gy [n, 6] of the rows of st [n, 5]."""
    cx, cy, _ = select_ref.car_circles(params)
    cz, sz = select_ref._trig(st[:, 2])
    gx = np.stack([(cx[q] * cz - cy[q] * sz) + st[:, 0] for q in range(6)], axis=1)
    gy = np.stack([(cx[q] * sz + cy[q] * cz) + st[:, 1] for q in range(6)], axis=1)
    return gx, gy


def covers(ag):
    """n_pts of an agent record, 0 when it covers nothing."""
    np_ = int(ag["n_pts"])
    if np_ < 1 or np_ > MAX_PTS or not (ag["radius"] >= 0):
        return 0
    if not (np.isfinite(ag["t"][:np_]).all() and np.isfinite(ag["x"][:np_]).all() and np.isfinite(ag["y"][:np_]).all()):
        return 0
    return np_


def pieces(ag, np_):
    """(kind, j) in the definition's order: 'before', segments 0 .. np - 2, 'after'."""
    out = []
    if int(ag["flags"]) & HOLD_BEFORE:
        out.append(("before", 0))
    out += [("segment", j) for j in range(np_ - 1)]
    if int(ag["flags"]) & HOLD_AFTER:
        out.append(("after", np_ - 1))
    return out


def path_gaps(params, st, t, agents, lo, hi):
    """gap_i, arg_i of the n - 1 intervals of ONE checked path: st [n, 5], t [n], agents lo .. hi - 1 of the record array."""
    n = len(st)
    _, _, cr = select_ref.car_circles(params)
    gx, gy = centres(params, st)
    t0, t1 = t[:-1], t[1:]
    g = np.full(n - 1, DBL_MAX)
    arg = np.full(n - 1, -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        dt = t1 - t0
        live = dt > 0
        ex, ey = gx[1:] - gx[:-1], gy[1:] - gy[:-1]
        for a in range(lo, hi):
            ag = agents[a]
            np_ = covers(ag)
            if not np_:
                continue
            T, X, Y, R = ag["t"], ag["x"], ag["y"], np.float64(ag["radius"])
            for kind, j in pieces(ag, np_):
                if kind == "before":
                    ta, tb = t0, vmin(t1, T[0])
                    axa = axb = np.full(n - 1, X[0]); aya = ayb = np.full(n - 1, Y[0])
                elif kind == "after":
                    ta, tb = vmax(t0, T[j]), t1
                    axa = axb = np.full(n - 1, X[j]); aya = ayb = np.full(n - 1, Y[j])
                else:
                    D = T[j + 1] - T[j]
                    if not (D > 0):
                        continue
                    ta, tb = vmax(t0, T[j]), vmin(t1, T[j + 1])
                    wa, wb = (ta - T[j]) / D, (tb - T[j]) / D
                    DX, DY = X[j + 1] - X[j], Y[j + 1] - Y[j]
                    axa, aya = X[j] + wa * DX, Y[j] + wa * DY
                    axb, ayb = X[j] + wb * DX, Y[j] + wb * DY
                m = live & (ta <= tb)
                if not m.any():
                    continue
                ua, ub = (ta - t0) / dt, (tb - t0) / dt
                for q in range(6):
                    rax, ray = (gx[:-1, q] + ua * ex[:, q]) - axa, (gy[:-1, q] + ua * ey[:, q]) - aya
                    rbx, rby = (gx[:-1, q] + ub * ex[:, q]) - axb, (gy[:-1, q] + ub * ey[:, q]) - ayb
                    dx, dy, px, py = rbx - rax, rby - ray, -rax, -ray
                    L2, dot = dx * dx + dy * dy, px * dx + py * dy
                    u = np.where(L2 > 0, dot / L2, 0.0)
                    u = np.where(u < 0, 0.0, u)
                    u = np.where(u > 1, 1.0, u)
                    qx, qy = px - u * dx, py - u * dy
                    gap = (np.sqrt(qx * qx + qy * qy) - cr[q]) - R
                    low = m & (gap < g)
                    g = np.where(low, gap, g)
                    arg = np.where(low, a, arg)
    return g, arg


def check(params, states, t, agents, first, dp, n_states=None, ok=None, set_of=None, v_limit_in=None):
    """po_dynamic_batch on host arrays: agents / first as binding.pack_agents returns them (unvalidated: read as the device entry reads them).  Returns the dict
    Engine.dynamic_batch returns."""
    states, t = np.asarray(states, dtype=np.float64), np.asarray(t, dtype=np.float64)
    B, N = states.shape[0], states.shape[1]
    S, n_agents = len(first) - 1, len(agents)
    clamp = lambda v, hi: min(max(int(v), 0), hi)
    L = np.full((B, N), -1.0) if v_limit_in is None else np.array(v_limit_in, dtype=np.float64)
    r = {"status": np.zeros(B, dtype=np.int32), "ok_out": np.zeros(B, dtype=np.int32), "gap_min": np.full(B, DBL_MAX), "first_state": np.full(B, -1, dtype=np.int32),
         "first_agent": np.full(B, -1, dtype=np.int32), "stop_state": np.full(B, -1, dtype=np.int32), "first_time": np.zeros(B), "gap": np.full((B, N), DBL_MAX),
         "v_limit": L.copy()}
    for b in range(B):
        n = N if n_states is None else clamp(n_states[b], N)
        st, tt = states[b, :n], t[b, :n]
        if (ok is not None and ok[b] == 0) or n < 2 or not (np.isfinite(st[:, :3]).all() and np.isfinite(tt).all()):
            continue
        k = 0 if set_of is None else clamp(set_of[b], S - 1)
        lo, hi = clamp(first[k], n_agents), clamp(first[k + 1], n_agents)
        g, arg = path_gaps(params, st, tt, agents, lo, hi)
        r["gap"][b, :n - 1] = g
        r["gap_min"][b] = g.min()
        below = np.flatnonzero(g < dp.margin)
        if not len(below):
            r["status"][b] = 1; r["ok_out"][b] = 1
            continue
        f = int(below[0])
        s = st[:, 4]
        s_stop = s[f] - np.float64(dp.stop_distance)
        reach = np.flatnonzero(s[:f + 1] <= s_stop)
        j = int(reach[-1]) if len(reach) else 0
        r["status"][b] = 2 if s[0] <= s_stop else 3
        r["first_state"][b], r["first_agent"][b], r["stop_state"][b], r["first_time"][b] = f, arg[f], j, tt[f]
        r["v_limit"][b, j:n] = 0.0
    return r
