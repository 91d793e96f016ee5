"""The definition of po_nudge_batch (include/po_hip.h) in numpy: reference lines, corridor bounds and predicted agents -> the side each agent
is passed on and the carved bounds.

Tests only, and the single arbiter of the definition.  One ufunc per operation of the definition, in the order it writes them, so every value is the same
sequence of rounded IEEE double operations the kernel runs; comparisons against this file are bit equality.  The vectors run over the 4 n PAIRS (state, circle) of
one path; agents and pieces are Python loops in the definition's order (tests/test_nudge.py checks this file against a scalar loop).  Agents that cover nothing
and the order of an agent's pieces are dynamic_ref's; sin / cos are the portable ones."""
import numpy as np

import dynamic_ref
import select_ref
from select_ref import DBL_MAX, vmax, vmin


def radius(params):
    """The covering-circle radius po_bounds_batch* derives from the parameters."""
    L, Wd = np.float64(params.car_length), np.float64(params.car_width)
    return np.sqrt((L / 8) * (L / 8) + (Wd / 2) * (Wd / 2)) + np.float64(params.safety_margin)


def fold(c, take, lo, hi):
    """lo = min(lo, c), hi = max(hi, c) where take."""
    return np.where(take & (c < lo), c, lo), np.where(take & (c > hi), c, hi)


def hull_piece(ua, la, ub, lb, rho, live, lo, hi):
    """The candidates of one piece whose ends are (ua, la) and (ub, lb) in the pair's frame, folded into lo, hi where live."""
    with np.errstate(all="ignore"):
        for u, l in ((ua, la), (ub, lb)):
            q = rho * rho - u * u
            has = live & (q >= 0)
            w = np.sqrt(np.where(has, q, 0.0))
            lo, hi = fold(l - w, has, lo, hi)
            lo, hi = fold(l + w, has, lo, hi)
        du, dl = ub - ua, lb - la
        L2 = du * du + dl * dl
        side = live & (L2 > 0) & (du != 0)
        length = np.sqrt(L2)
        ox, oy = (rho * dl) / length, (rho * du) / length
        tp = (ox - ua) / du
        lo, hi = fold((la + oy) + tp * dl, side & (0 <= tp) & (tp <= 1), lo, hi)
        tm = (0.0 - (ox + ua)) / du
        lo, hi = fold((la - oy) + tm * dl, side & (0 <= tm) & (tm <= 1), lo, hi)
    return lo, hi


def frames(params, x, y, z):
    """cx, cy, cz, sz [4 n] of the pairs p = 4 i + j of ONE path."""
    cz, sz = select_ref._trig(z)
    d = np.array([np.float64(params.d[j]) for j in range(4)])
    cz, sz = np.repeat(cz, 4), np.repeat(sz, 4)
    dd = np.tile(d, len(x))
    return np.repeat(x, 4) + dd * cz, np.repeat(y, 4) + dd * sz, cz, sz


def agent_hull(ag, np_, fr, w0, w1, rho):
    """lo, hi [4 n] of one agent that covers something: fr = frames(...), w0, w1 [4 n] the window of each pair's state."""
    cx, cy, cz, sz = fr
    P = len(cx)
    lo, hi = np.full(P, DBL_MAX), np.full(P, -DBL_MAX)
    T, X, Y = ag["t"], ag["x"], ag["y"]
    with np.errstate(all="ignore"):
        for kind, j in dynamic_ref.pieces(ag, np_):
            if kind == "before":
                ta, tb = w0, vmin(w1, T[0])
                axa = axb = np.full(P, X[0]); aya = ayb = np.full(P, Y[0])
            elif kind == "after":
                ta, tb = vmax(w0, T[j]), w1
                axa = axb = np.full(P, X[j]); aya = ayb = np.full(P, Y[j])
            else:
                D = T[j + 1] - T[j]
                if not (D > 0):
                    continue
                ta, tb = vmax(w0, T[j]), vmin(w1, T[j + 1])
                wa, wb = (ta - T[j]) / D, (tb - T[j]) / D
                DX, DY = X[j + 1] - X[j], Y[j + 1] - Y[j]
                axa, aya = X[j] + wa * DX, Y[j] + wa * DY
                axb, ayb = X[j] + wb * DX, Y[j] + wb * DY
            live = ta <= tb
            if not live.any():
                continue
            dxa, dya, dxb, dyb = axa - cx, aya - cy, axb - cx, ayb - cy
            ua, la = dxa * cz + dya * sz, (-dxa) * sz + dya * cz
            ub, lb = dxb * cz + dyb * sz, (-dxb) * sz + dyb * cz
            lo, hi = hull_piece(ua, la, ub, lb, rho, live, lo, hi)
    return lo, hi


def decide(rl, rr, min_width, sp):
    """The side of an agent that touches the corridor."""
    left, right = bool(rl >= min_width), bool(rr >= min_width)
    if sp == 1 and left:
        return 1
    if sp == -1 and right:
        return -1
    if left and right:
        return 1 if rl >= rr else -1
    if left:
        return 1
    if right:
        return -1
    return 2


def nudge(params, ref_x, ref_y, ref_z, t, bounds, agents, first, npar, n_points=None, ok=None, set_of=None, side_prev=None, W=None):
    """po_nudge_batch on host arrays: agents / first as binding.pack_agents returns them (unvalidated: read as the device entry reads them).  W: the columns of
    side (None: side_prev's, else the largest set, at least 1 — Engine.nudge_batch's rule).  Returns the dict Engine.nudge_batch returns."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    ref_x, ref_y, ref_z, t, bounds = f64(ref_x), f64(ref_y), f64(ref_z), f64(t), f64(bounds)
    B, N = ref_x.shape[0], ref_x.shape[1]
    S, n_agents = len(first) - 1, len(agents)
    if W is None:
        W = np.asarray(side_prev).shape[1] if side_prev is not None else max(1, int(np.diff(first).max()) if S > 0 else 1)
    clamp = lambda v, hi: min(max(int(v), 0), hi)
    margin, t_before, t_after, min_width = (np.float64(getattr(npar, k)) for k in ("margin", "t_before", "t_after", "min_width"))
    skip, rad = int(npar.skip_states), radius(params)
    r = {"status": np.zeros(B, dtype=np.int32), "ok_out": np.zeros(B, dtype=np.int32), "bounds": bounds.reshape(B, N, 4, 2).copy(),
         "side": np.zeros((B, W), dtype=np.int32), "first_blocked_state": np.full(B, -1, dtype=np.int32),
         "first_blocked_agent": np.full(B, -1, dtype=np.int32), "width_min": np.full(B, DBL_MAX)}
    for b in range(B):
        n = N if n_points is None else clamp(n_points[b], N)
        x, y, z, tt = ref_x[b, :n], ref_y[b, :n], ref_z[b, :n], t[b, :n]
        Wl, Wu = r["bounds"][b, :n, :, 0].reshape(-1).copy(), r["bounds"][b, :n, :, 1].reshape(-1).copy()
        if (ok is not None and ok[b] == 0) or n < 1 or not all(np.isfinite(v).all() for v in (x, y, z, tt, Wl, Wu)):
            continue
        fr = frames(params, x, y, z)
        with np.errstate(all="ignore"):
            w0, w1 = np.repeat(tt - t_before, 4), np.repeat(tt + t_after, 4)
        state = np.repeat(np.arange(n), 4)
        k = 0 if set_of is None else clamp(set_of[b], S - 1)
        lo_a, hi_a = clamp(first[k], n_agents), clamp(first[k + 1], n_agents)
        carved = False
        for a in range(lo_a, hi_a):
            e = a - lo_a
            ag = agents[a]
            np_ = dynamic_ref.covers(ag)
            if not np_:
                continue
            rho = (rad + np.float64(ag["radius"])) + margin
            lo, hi = agent_hull(ag, np_, fr, w0, w1, rho)
            with np.errstate(all="ignore"):
                touched = (state >= skip) & (lo <= hi) & (hi > Wl) & (lo < Wu)
                if not touched.any():
                    continue
                rl, rr, f = (Wu - hi)[touched].min(), (lo - Wl)[touched].min(), int(state[touched].min())
            sp = int(side_prev[b][e]) if side_prev is not None and e < W else 0
            side = decide(rl, rr, min_width, sp)
            if e < W:
                r["side"][b, e] = side
            if side == 2:
                if r["first_blocked_agent"][b] < 0:
                    r["first_blocked_agent"][b], r["first_blocked_state"][b] = a, f
            elif side == 1:
                Wl, carved = np.where(touched, hi, Wl), True
            else:
                Wu, carved = np.where(touched, lo, Wu), True
        r["bounds"][b, :n, :, 0], r["bounds"][b, :n, :, 1] = Wl.reshape(n, 4), Wu.reshape(n, 4)
        with np.errstate(all="ignore"):
            wd = Wu - Wl
        r["width_min"][b] = np.where(wd == 0, 0.0, wd).min()
        r["status"][b] = 3 if r["first_blocked_agent"][b] >= 0 else (2 if carved else 1)
        r["ok_out"][b] = 1 if r["status"][b] != 3 else 0
    return r
