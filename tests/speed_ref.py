"""The definition of po_speed_batch (include/po_hip.h) in numpy: planned paths -> v, a, t per state, total time and a status.

Tests only.  One ufunc per operation of the definition, in the order it writes them, so every value is the same sequence of rounded IEEE double operations the
kernels run; comparisons against this file are bit equality.  The caps are vectors over the states of one path; the three sweeps are vectors over the PATHS of the
batch, one state per step (tests/test_speed.py checks both against a scalar loop over one path).  The clearance is select_ref.clearances."""
import numpy as np

import select_ref
from select_ref import vmax, vmin

G = 9.8


def friction(params):
    """A = mu * g: one multiply."""
    return np.float64(params.mu) * np.float64(G)


def clamp_n(n_states, B, N):
    return np.full(B, N, dtype=np.int64) if n_states is None else np.clip(np.asarray(n_states, dtype=np.int64), 0, N)


def caps(params, sp, st, limit=None, m=None):
    """W_i of ONE path: st [n, 5] (rows < n only, n >= 2), limit [n] or None, m the path's po_map when sp.use_map."""
    k, s = st[:, 3], st[:, 4]
    n = len(st)
    with np.errstate(all="ignore"):
        W = np.full(n, np.float64(sp.v_max) * np.float64(sp.v_max))
        ak = np.abs(k)
        W = np.where(ak > 0, vmin(W, np.float64(sp.a_lat_max) / ak), W)
        ds = s[1:] - s[:-1]
        r = np.where(ds > 0, np.abs(k[1:] - k[:-1]) / ds, 0.0)
        rr = np.zeros(n)
        rr[1:] = vmax(rr[1:], r)
        rr[:-1] = vmax(rr[:-1], r)
        q = np.float64(params.max_curvature_rate) / rr
        W = np.where(rr > 0, vmin(W, q * q), W)
        if limit is not None:
            l = np.asarray(limit, dtype=np.float64)
            W = np.where(l >= 0, vmin(W, l * l), W)
        if sp.use_map:
            c = select_ref.clearances(params, m, st)
            cc = np.where(c > 0, c, 0.0)
            vc = np.float64(sp.clear_v0) + np.float64(sp.clear_gain) * cc
            W = vmin(W, vc * vc)
    return W


def profile(params, states, v0, sp, n_states=None, ok=None, v_end=None, v_limit=None, maps=None, layer_of=None):
    """po_speed_batch on host arrays.  maps: list of po_map (oracle_py.make_map) when sp.use_map, layer_of [B] or None (layer 0).  Returns the dict
    Engine.speed_batch returns, plus W [B, N] (the caps) and w [B, N] (the squared speeds)."""
    states = np.asarray(states, dtype=np.float64)
    B, N = states.shape[0], states.shape[1]
    v0 = np.asarray(v0, dtype=np.float64)
    n = clamp_n(n_states, B, N)
    A = friction(params)
    AA = A * A
    valid = np.zeros(B, dtype=bool)
    W = np.zeros((B, N))
    for b in range(B):
        st = states[b, :n[b]]
        cols = slice(0, 5) if sp.use_map else slice(3, 5)
        if (ok is not None and ok[b] == 0) or n[b] < 2 or not (np.isfinite(v0[b]) and v0[b] >= 0) or not np.isfinite(st[:, cols]).all():
            continue
        valid[b] = True
        m = maps[0 if layer_of is None else int(layer_of[b])] if sp.use_map else None
        W[b, :n[b]] = caps(params, sp, st, None if v_limit is None else v_limit[b, :n[b]], m)
    k, s = np.abs(states[:, :, 3]), states[:, :, 4]
    w = np.zeros((B, N))
    nmax = int(n[valid].max()) if valid.any() else 0
    two = np.float64(2.0)
    with np.errstate(all="ignore"):
        # forward
        if nmax:
            w[:, 0] = vmin(W[:, 0], v0 * v0)
        for i in range(nmax - 1):
            lat = w[:, i] * k[:, i]
            rem = AA - lat * lat
            rem = np.where(rem > 0, rem, 0.0)
            ax = vmin(np.sqrt(rem), np.float64(sp.a_max))
            ds = s[:, i + 1] - s[:, i]
            d = np.where(ds > 0, ds, 0.0)
            w[:, i + 1] = vmin(W[:, i + 1], w[:, i] + (two * ax) * d)
        # backward
        if v_end is not None:
            e = np.asarray(v_end, dtype=np.float64)
            use = valid & np.isfinite(e) & (e >= 0)
            last = np.maximum(n - 1, 0)
            rows = np.flatnonzero(use)
            w[rows, last[rows]] = vmin(w[rows, last[rows]], e[rows] * e[rows])
        for i in range(nmax - 2, -1, -1):
            act = valid & (i < n - 1)
            lat = w[:, i + 1] * k[:, i + 1]
            rem = AA - lat * lat
            rem = np.where(rem > 0, rem, 0.0)
            bx = vmin(np.sqrt(rem), np.float64(sp.b_max))
            ds = s[:, i + 1] - s[:, i]
            d = np.where(ds > 0, ds, 0.0)
            w[:, i] = np.where(act, vmin(w[:, i], w[:, i + 1] + (two * bx) * d), w[:, i])
        # outputs
        inside = valid[:, None] & (np.arange(N)[None, :] < n[:, None])
        w = np.where(inside, w, 0.0)
        v = np.sqrt(w)
        a = np.zeros((B, N)); t = np.zeros((B, N))
        for i in range(nmax - 1):
            act = valid & (i < n - 1)
            ds = s[:, i + 1] - s[:, i]
            d = np.where(ds > 0, ds, 0.0)
            ai = np.where(ds > 0, (w[:, i + 1] - w[:, i]) / (two * ds), 0.0)
            ai = vmax(-A, vmin(ai, A))
            a[:, i] = np.where(act, ai, 0.0)
            vs = v[:, i] + v[:, i + 1]
            t[:, i + 1] = np.where(act, t[:, i] + np.where(vs > 0, (two * d) / vs, 0.0), 0.0)
        total = np.where(valid, t[np.arange(B), np.maximum(n - 1, 0)], 0.0) if N else np.zeros(B)
        status = np.where(valid, np.where(w[:, 0] < v0 * v0, 2, 1), 0).astype(np.int32) if N else np.zeros(B, dtype=np.int32)
    W = np.where(inside, W, 0.0)
    return {"v": v, "a": a, "t": t, "total_time": total, "status": status, "W": W, "w": w}
