"""The definition of po_select_batch (include/po_hip.h) in numpy: candidate paths -> eight features and a cost, one winner per group.

Tests only.  One ufunc per operation of the definition, in the order it writes them, so every value is the same sequence of rounded IEEE double operations the
kernels run; comparisons against this file are bit equality.  Trig comes from the oracle's portable sin / cos (include/po_pmath.h), map distances from
oracle_py.map_distance on an oracle_py.make_map of the candidate's layer, the footprint circles from po_params with the formulas of CarGeometry."""
import ctypes
import math

import numpy as np

from oracle import oracle_py

DBL_MAX = float(np.finfo(np.float64).max)
INF = float("inf")


def car_circles(p):
    """cx, cy, cr [6] of the footprint circles rr, rl, fr, fl, fm, rm (car_geometry.cpp:38-56 as po_capi.cpp's make_car writes it)."""
    width, back, front = p.car_width, p.car_length / 2.0 - p.rear_axle_to_center, p.car_length / 2.0 + p.rear_axle_to_center
    length = front + back
    bx = (front - back) / 2.0
    shift = width / 4.0
    small_r = math.sqrt(2 * (shift * shift))
    large_r = math.sqrt(width * width + ((length - width) / 2.0) * ((length - width) / 2.0)) / 2
    cx = [-back + shift, -back + shift, front - shift, front - shift, bx + (length - width) / 4, bx - (length - width) / 4]
    cy = [-width / 2.0 + shift, width / 2.0 - shift, -width / 2.0 + shift, width / 2.0 - shift, 0.0, 0.0]
    return np.array(cx), np.array(cy), np.array([small_r] * 4 + [large_r] * 2)


def trig_lib():
    """The oracle library with its portable sin / cos typed for ctypes."""
    L = oracle_py.lib()
    for f in ("po_oracle_psin", "po_oracle_pcos"):
        getattr(L, f).restype = ctypes.c_double
        getattr(L, f).argtypes = [ctypes.c_double]
    return L


def _trig(z):
    L = trig_lib()
    return np.array([L.po_oracle_pcos(float(v)) for v in z]), np.array([L.po_oracle_psin(float(v)) for v in z])


def vmin(a, b):
    return np.where(b < a, b, a)


def vmax(a, b):
    return np.where(b > a, b, a)


def fold(op, init, v):
    """F(op, init, v) of the definition: a (64, ceil(n / 64)) accumulation, then six folds."""
    v = np.asarray(v, dtype=np.float64)
    P = np.full(64, init, dtype=np.float64)
    for r in range(0, len(v), 64):
        row = v[r:r + 64]
        P[:len(row)] = op(P[:len(row)], row)
    h = 32
    while h:
        P[:h] = op(P[:h], P[h:2 * h])
        h //= 2
    return P[0]


def clearances(params, m, st):
    """c_i of every row of st [n, 5] on the po_map m."""
    cx, cy, cr = car_circles(params)
    cz, sz = _trig(st[:, 2])
    c = None
    for q in range(6):
        gx = (cx[q] * cz - cy[q] * sz) + st[:, 0]
        gy = (cx[q] * sz + cy[q] * cz) + st[:, 1]
        d, _ = oracle_py.map_distance(m, np.stack([gx, gy], axis=1))
        cq = d - cr[q]
        c = cq if q == 0 else vmin(c, cq)
    return c


def prev_dist2(x, y, uv):
    """e_i for states (x, y) against the polyline uv [np, 2], np >= 2."""
    e = None
    for j in range(len(uv) - 1):
        dx, dy = uv[j + 1, 0] - uv[j, 0], uv[j + 1, 1] - uv[j, 1]
        px, py = x - uv[j, 0], y - uv[j, 1]
        L2 = dx * dx + dy * dy
        dot = px * dx + py * dy
        with np.errstate(all="ignore"):
            t = dot / L2 if L2 > 0 else np.zeros_like(dot)
        t = np.where(t < 0, 0.0, t)
        t = np.where(t > 1, 1.0, t)
        qx, qy = px - t * dx, py - t * dy
        D = qx * qx + qy * qy
        e = D if j == 0 else vmin(e, D)
    return e


def features(params, m, st, sp, goal=None, prev=None):
    """The eight features of ONE candidate: st [n, 5] (rows < n only), goal (gx, gy) or None, prev [np, 2] or None (no previous path)."""
    add = lambda a, b: a + b
    n = len(st)
    f = np.zeros(8)
    f[4] = DBL_MAX
    if n == 0:
        return f
    with np.errstate(all="ignore"):
        x, y, k, s = st[:, 0], st[:, 1], st[:, 3], st[:, 4]
        c = clearances(params, m, st)
        t = sp.d_safe - c
        t = np.where(t > 0, t, 0.0)
        p = t * t
        e = prev_dist2(x, y, prev) if prev is not None and len(prev) >= 2 else np.zeros(n)
        ds = s[1:] - s[:-1]
        T1 = (0.5 * (k[:-1] * k[:-1] + k[1:] * k[1:])) * ds
        dk = k[1:] - k[:-1]
        T2 = np.where(ds > 0, (dk * dk) / ds, 0.0)
        T5 = (0.5 * (p[:-1] + p[1:])) * ds
        T7 = (0.5 * (e[:-1] + e[1:])) * ds
        f[0] = s[-1]
        f[1] = fold(add, 0.0, T1)
        f[2] = fold(add, 0.0, T2)
        f[3] = fold(vmax, 0.0, np.abs(k))
        f[4] = fold(vmin, DBL_MAX, c)
        f[5] = fold(add, 0.0, T5)
        if goal is not None:
            ex, ey = x[-1] - goal[0], y[-1] - goal[1]
            f[6] = np.sqrt(ex * ex + ey * ey)
        f[7] = fold(add, 0.0, T7)
    return f


def clamp_table(gs, B):
    """gs' of the definition: what the kernels read of an unvalidated group table."""
    out = np.zeros(len(gs), dtype=np.int64)
    out[0] = min(max(int(gs[0]), 0), B)
    for g in range(1, len(gs)):
        out[g] = min(max(max(int(gs[g]), int(out[g - 1])), 0), B)
    return out


def select(params, maps, states, group_start, sp, n_states=None, ok=None, goal=None, prev_states=None, prev_n=None, layer_of=None):
    """po_select_batch on host arrays.  maps: list of po_map (oracle_py.make_map), layer_of [B] or None (layer 0).  Returns the dict Engine.select_batch returns."""
    states = np.asarray(states, dtype=np.float64)
    B, N = states.shape[0], states.shape[1]
    G = len(group_start) - 1
    gs = clamp_table(group_start, B)
    group = np.full(B, -1)
    for g in range(G):
        group[gs[g]:gs[g + 1]] = g
    Np = 0 if prev_states is None else prev_states.shape[1]
    w = [float(v) for v in sp.w]
    feat = np.zeros((B, 8)); cost = np.full(B, INF)
    nn = np.zeros(B, dtype=np.int64)
    for b in range(B):
        n = N if n_states is None else min(max(int(n_states[b]), 0), N)
        nn[b] = n
        st = states[b, :n]
        prev = None
        if Np > 0 and group[b] >= 0:
            g = group[b]
            npv = Np if prev_n is None else min(max(int(prev_n[g]), 0), Np)
            prev = prev_states[g, :npv, :2]
        m = maps[0 if layer_of is None else int(layer_of[b])]
        f = features(params, m, st, sp, None if goal is None else goal[b, :2], prev)
        feat[b] = f
        feas = (ok is None or ok[b] != 0) and n >= 2 and bool(np.isfinite(st).all()) and bool(np.isfinite(f).all())
        with np.errstate(all="ignore"):
            c = np.float64(w[0]) * f[0]
            for j in range(1, 8):
                c = c + np.float64(w[j]) * f[j]
        feas = feas and f[4] >= sp.min_clearance and f[3] <= sp.max_kmax and f[6] <= sp.max_goal_dist and bool(np.isfinite(c))
        cost[b] = c if feas else INF
    best = np.full(G, -1, dtype=np.int32); best_cost = np.full(G, INF); n_feasible = np.zeros(G, dtype=np.int32)
    sel_states = np.zeros((G, N, 5)); sel_n = np.zeros(G, dtype=np.int32)
    for g in range(G):
        for b in range(gs[g], gs[g + 1]):
            if cost[b] < INF:
                n_feasible[g] += 1
                if best[g] < 0 or cost[b] < best_cost[g]:
                    best[g] = b; best_cost[g] = cost[b]
        if best[g] >= 0:
            sel_n[g] = nn[best[g]]
            sel_states[g, :sel_n[g]] = states[best[g], :sel_n[g]]
    return {"feat": feat, "cost": cost, "best": best, "best_cost": best_cost, "n_feasible": n_feasible, "sel_states": sel_states, "sel_n": sel_n}
