"""The definition of po_speedqp_batch (include/po_hip.h) in numpy: a station-time plan and its cell map -> the tunnel lo_q <= s(T_q) <= hi_q,
and the piecewise-jerk QP inside it solved by OSQP's ADMM, unscaled, with a banded LDL^T.

Tests only.  One ufunc per operation of the definition, in the order it writes them, so every value is the same sequence of rounded IEEE double operations the
kernel runs; comparisons against this file are bit equality.  A and A^T are the two nested difference operators of the header (rows_of, cols_of); the matrix of
the x-update is those operators on the unit vectors.  The three chains (factorisation, two substitutions) are Python loops over the samples whose every step is a
ufunc over the PATHS of a group: paths with the same n_q run in lockstep, each frozen where it stops, which changes no bit of any of them.  The state of a sample
is found by the kernel's bisection (not searchsorted: a NaN iterate must land where the kernel puts it); the interpolation is stgo_ref's line by line."""
import numpy as np

from stplan_ref import MAX_STATIONS, vmin
from trajectory_ref import PI, TWO_PI

MAX_SAMPLES = 256
KEYS = ("status", "iters", "n_fact", "r_prim", "r_dual", "n_q", "states", "v", "a", "jerk", "t", "lo", "hi", "index")
CLASSES = ("p", "v", "a", "j")


def times(qp):
    """T_q = (double)q * dts, q < Q."""
    return np.arange(int(qp.Q)).astype(np.float64) * np.float64(qp.dts)


def absmax(rows):
    """The norm of the definition over a dict of row arrays [G, .] (or one array): the largest |v| compared as 64-bit patterns, so a NaN outranks every number and
    no order of the reduction can change the result.  [G]."""
    arrs = list(rows.values()) if isinstance(rows, dict) else [rows]
    a = np.abs(np.concatenate([np.asarray(v, dtype=np.float64) for v in arrs], axis=-1))
    return np.ascontiguousarray(a).view(np.uint64).max(axis=-1).view(np.float64) if a.shape[-1] else np.zeros(a.shape[:-1])


def _shift_right(a):  # a[r - 1], 0 in front
    return np.concatenate([np.zeros(a.shape[:-1] + (1,)), a[..., :-1]], axis=-1)


def _shift_left(a):  # a[r + 1], 0 behind
    return np.concatenate([a[..., 1:], np.zeros(a.shape[:-1] + (1,))], axis=-1)


def inv_steps(h):
    i1 = np.float64(1.0) / h
    i2 = i1 / h
    return i1, i2, i2 / h


def rows_of(x, h):
    """A x: the position rows [.., n], the velocity rows [.., n - 1], the acceleration rows [.., n - 1] (row 0 without its constant) and the jerk rows
    [.., max(n - 3, 0)] (row r = 1 .. n - 3 at index r - 1)."""
    i1, i2, i3 = inv_steps(h)
    with np.errstate(all="ignore"):
        d1 = x[..., 1:] - x[..., :-1]
        e = d1 - _shift_right(d1)
        f = e[..., 2:] - e[..., 1:-1]
        return {"p": x, "v": d1 * i1, "a": e * i2, "j": f * i3}


def cols_of(w, h):
    """A^T w for a dict of row arrays: [.., n]."""
    i1, i2, i3 = inv_steps(h)
    n = w["p"].shape[-1]
    with np.errstate(all="ignore"):
        pj = np.zeros(w["p"].shape[:-1] + (n - 1,))
        if n >= 4:
            pj[..., 1:n - 2] = w["j"] * i3
        tj = _shift_right(pj) - pj
        ta = w["a"] * i2 + tj
        tb = ta - _shift_left(ta)
        tv = w["v"] * i1 + tb
        z1 = np.zeros(w["p"].shape[:-1] + (1,))
        return w["p"] + (np.concatenate([z1, tv], axis=-1) - np.concatenate([tv, z1], axis=-1))


def row_rho(l, u, rho):
    """rho per row: 1e3 * rho where l and u have the same bits."""
    out = {}
    for c in CLASSES:
        eq = np.ascontiguousarray(l[c]).view(np.int64) == np.ascontiguousarray(u[c]).view(np.int64)
        out[c] = np.where(eq, np.float64(1e3) * rho[:, None], rho[:, None] + np.zeros(l[c].shape))
    return out


def band_of(l, u, rho, qp):
    """The lower band of P + sigma I + A^T diag(rho) A, [G, 4, n]: band[:, k, c] = the entry (c + k, c) of column c = the operators applied to unit vector c."""
    h = np.float64(qp.dts)
    G, n = l["p"].shape
    rr = row_rho(l, u, rho)
    two_ws, two_wa, two_wj = (np.float64(2.0) * np.float64(getattr(qp, f)) for f in ("w_s", "w_a", "w_j"))
    r = rows_of(np.eye(n)[None], h)  # [1, n columns, rows]
    w = {"p": (rr["p"] + (two_ws + np.float64(qp.sigma)))[:, None, :] * r["p"], "v": rr["v"][:, None, :] * r["v"],
         "a": (rr["a"] + two_wa)[:, None, :] * r["a"], "j": (rr["j"] + two_wj)[:, None, :] * r["j"]}
    col = cols_of(w, h)  # [G, c, q]
    band = np.zeros((G, 4, n))
    for k in range(4):
        for c in range(n - k):
            band[:, k, c] = col[:, c, c + k]
    return band


def factor(band):
    """Banded LDL^T, column by column: D [G, n], L [G, 3, n] with L[:, k - 1, j] = L_{j + k, j}."""
    G, _, n = band.shape
    D, L = np.zeros((G, n)), np.zeros((G, 3, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            d = band[:, 0, j].copy()
            c1, c2 = band[:, 1, j].copy(), band[:, 2, j].copy()
            for k in (1, 2, 3):
                if j - k >= 0:
                    d = d - (L[:, k - 1, j - k] * D[:, j - k]) * L[:, k - 1, j - k]
            if j >= 1:
                c1 = c1 - (L[:, 1, j - 1] * D[:, j - 1]) * L[:, 0, j - 1]
            if j >= 2:
                c1 = c1 - (L[:, 2, j - 2] * D[:, j - 2]) * L[:, 1, j - 2]
            if j >= 1:
                c2 = c2 - (L[:, 2, j - 1] * D[:, j - 1]) * L[:, 0, j - 1]
            D[:, j] = d
            L[:, 0, j], L[:, 1, j], L[:, 2, j] = c1 / d, c2 / d, band[:, 3, j] / d
    return D, L


def solve_band(D, L, rhs):
    G, n = rhs.shape
    yv = np.zeros((G, n))
    with np.errstate(all="ignore"):
        for q in range(n):
            t = rhs[:, q]
            for k in (3, 2, 1):
                if q - k >= 0:
                    t = t - L[:, k - 1, q - k] * yv[:, q - k]
            yv[:, q] = t
        w = yv / D
        xt = np.zeros((G, n))
        for q in range(n - 1, -1, -1):
            t = w[:, q]
            for k in (3, 2, 1):
                if q + k < n:
                    t = t - L[:, k - 1, q] * xt[:, q + k]
            xt[:, q] = t
    return xt


def _keep(active, new, old):
    return np.where(active[:, None], new, old)


def admm(l, u, qv, qp):
    """OSQP's ADMM on a group of G paths with the same n: l, u dicts of row bounds, qv [G, n].  Returns x [G, n], status, iters, n_fact, r_prim, r_dual, eps_prim [G]
    (the primal threshold of the last check) and the row values A x of the final iterate."""
    h = np.float64(qp.dts)
    G, n = qv.shape
    f = lambda k: np.float64(getattr(qp, k))
    sigma, alpha, eps_abs, eps_rel = f("sigma"), f("alpha"), f("eps_abs"), f("eps_rel")
    om = np.float64(1.0) - alpha
    two_ws, two_wa, two_wj = np.float64(2.0) * f("w_s"), np.float64(2.0) * f("w_a"), np.float64(2.0) * f("w_j")
    max_iter, every, adaptive = int(qp.max_iter), int(qp.check_every), int(qp.adaptive_rho)
    rho = np.full(G, f("rho"))
    x = np.zeros((G, n))
    z = {c: np.zeros(l[c].shape) for c in CLASSES}
    y = {c: np.zeros(l[c].shape) for c in CLASSES}
    status, iters, n_fact = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32), np.ones(G, dtype=np.int32)
    r_prim, r_dual, eps_prim = np.zeros(G), np.zeros(G), np.zeros(G)
    active = np.ones(G, dtype=bool)
    rr = row_rho(l, u, rho)
    D, L = factor(band_of(l, u, rho, qp))
    nq = absmax(qv)
    with np.errstate(all="ignore"):
        for it in range(1, max_iter + 1):
            rhs = (sigma * x - qv) + cols_of({c: rr[c] * z[c] - y[c] for c in CLASSES}, h)
            xt = solve_band(D, L, rhs)
            zt = rows_of(xt, h)
            x = _keep(active, alpha * xt + om * x, x)
            for c in CLASSES:
                zr = alpha * zt[c] + om * z[c]
                zc = zr + y[c] / rr[c]
                zn = np.where(l[c] > zc, l[c], zc)
                zn = np.where(u[c] < zn, u[c], zn)
                y[c] = _keep(active, y[c] + rr[c] * (zr - zn), y[c])
                z[c] = _keep(active, zn, z[c])
            if it % every != 0 and it != max_iter:
                continue
            ax = rows_of(x, h)
            rp = absmax({c: ax[c] - z[c] for c in CLASSES})
            nax, nz = absmax(ax), absmax(z)
            px = two_ws * x + cols_of({"p": np.zeros((G, n)), "v": np.zeros(ax["v"].shape), "a": two_wa * ax["a"], "j": two_wj * ax["j"]}, h)
            aty = cols_of(y, h)
            rd = absmax((px + qv) + aty)
            npx, naty = absmax(px), absmax(aty)
            mp = np.where(nz > nax, nz, nax)
            md = np.where(naty > npx, naty, npx)
            md = np.where(nq > md, nq, md)
            ep, ed = eps_abs + eps_rel * mp, eps_abs + eps_rel * md
            done = (rp <= ep) & (rd <= ed)
            r_prim, r_dual, eps_prim = np.where(active, rp, r_prim), np.where(active, rd, r_dual), np.where(active, ep, eps_prim)
            iters = np.where(active, it, iters).astype(np.int32)
            status = np.where(active & done, 1, status).astype(np.int32)
            active = active & ~done
            if it == max_iter:
                status = np.where(active, 2, status).astype(np.int32)
                break
            if not active.any():
                break
            if adaptive:
                rn = rho * np.sqrt((rp / mp) / (rd / md))
                rn = np.where(np.float64(1e-6) > rn, np.float64(1e-6), rn)
                rn = np.where(np.float64(1e6) < rn, np.float64(1e6), rn)
                move = active & ((rn > np.float64(5.0) * rho) | (rn < rho / np.float64(5.0)))
                if move.any():
                    rho = np.where(move, rn, rho)
                    n_fact = (n_fact + move).astype(np.int32)
                    rr = row_rho(l, u, rho)
                    D, L = factor(band_of(l, u, rho, qp))  # (paths whose rho did not move get the bits they had)
    return {"x": x, "status": status, "iters": iters, "n_fact": n_fact, "r_prim": r_prim, "r_dual": r_dual, "eps_prim": eps_prim, "ax": rows_of(x, h), "z": z}


def tunnel(S, Vc, station, nl, cells, qp):
    """The geometry half for ONE path: S [M] the stations' s, Vc [M] their caps, station [nl + 1], cells [K, MAX_STATIONS] or None.  Returns n_q, lo [n_q], hi [n_q]
    and C [n_q - 1], the cap of every velocity row."""
    M, dt = len(S), np.float64(qp.dt)
    T = times(qp)
    n_q = int((T <= np.float64(nl) * dt).sum())
    kt = np.arange(nl + 1).astype(np.float64) * dt
    lo, hi, C = np.zeros(n_q), np.zeros(n_q), np.zeros(max(n_q - 1, 0))

    def window(w):
        p, j = int(station[w]), int(station[w + 1])
        lo_m, hi_m = 0, M - 1
        if cells is not None:
            below = [m for m in range(p) if cells[w][m] >= 0]
            above = [m for m in range(j + 1, M) if cells[w][m] >= 0]
            lo_m = 1 + below[-1] if below else 0
            hi_m = above[0] - 1 if above else M - 1
        return S[lo_m] - S[0], S[hi_m] - S[0]

    for q in range(n_q):
        kk = int(np.searchsorted(kt, T[q], side="right")) - 1  # the largest k in 0 .. nl with (double)k * dt <= T
        ws = [w for w in ([kk - 1] if (kk >= 1 and T[q] == kt[kk]) else []) + [kk] if w <= nl - 1]
        for n_, w in enumerate(ws):
            a, b = window(w)
            lo[q] = a if n_ == 0 else (a if a > lo[q] else lo[q])
            hi[q] = b if n_ == 0 else (b if b < hi[q] else hi[q])
        if q < n_q - 1:
            w = min(kk, nl - 1)
            c = Vc[station[w]]
            for m in range(int(station[w]) + 1, int(station[w + 1]) + 1):
                c = vmin(c, Vc[m])
            C[q] = c
    lo[0] = hi[0] = 0.0
    return n_q, lo, hi, C


def sample_rows(st, sq):
    """The rows of ONE path at the arc lengths sq [m]: the kernel's bisection over the whole path, then stgo's interpolation.  Returns rows [m, 5] and index [m]."""
    n = len(st)
    s = st[:, 4]
    with np.errstate(all="ignore"):
        sx = np.where(sq < s[0], s[0], sq)
        sx = np.where(sx > s[n - 1], s[n - 1], sx)
        lo, hi = np.zeros(len(sq), dtype=np.int64), np.full(len(sq), n - 1, dtype=np.int64)
        while ((hi - lo) > 1).any():
            go = (hi - lo) > 1
            mid = lo + ((hi - lo) >> 1)
            le = s[mid] <= sx
            lo, hi = np.where(go & le, mid, lo), np.where(go & ~le, mid, hi)
        i, i1 = lo, lo + 1
        ds = s[i1] - s[i]
        lam = np.where(ds > 0, (sx - s[i]) / ds, 0.0)
        lam = np.where(lam < 0, 0.0, lam)
        lam = np.where(lam > 1, 1.0, lam)
        x = st[i, 0] + lam * (st[i1, 0] - st[i, 0])
        y = st[i, 1] + lam * (st[i1, 1] - st[i, 1])
        k = st[i, 3] + lam * (st[i1, 3] - st[i, 3])
        so = s[i] + lam * ds
        dz = st[i1, 2] - st[i, 2]
        dz = np.where(dz > PI, dz - TWO_PI, np.where(dz < -PI, dz + TWO_PI, dz))
        z = st[i, 2] + lam * dz
    return np.stack([x, y, z, k, so], axis=1), i.astype(np.int32)


def setup(states, v0, station, n_layers, ref_states, qp, n_states=None, ok=None, v_cap=None, cells=None, check_tunnel=False):
    """Everything before the iterations, path by path: a list with None for a path that is not run, else a dict n_q, lo, hi, C, S0, rp (r_q - S_0), n."""
    states, v0, ref_states = np.asarray(states, dtype=np.float64), np.asarray(v0, dtype=np.float64), np.asarray(ref_states, dtype=np.float64)
    B, N = states.shape[0], states.shape[1]
    K, stride = int(qp.K), int(qp.stride)
    clamp = lambda v, hi: min(max(int(v), 0), hi)
    out = []
    for b in range(B):
        out.append(None)
        n = N if n_states is None else clamp(n_states[b], N)
        st = states[b, :n]
        if (ok is not None and ok[b] == 0) or n < 2 or not (np.isfinite(v0[b]) and v0[b] >= 0) or not np.isfinite(st[:, [0, 1, 2, 4]]).all():
            continue
        if (st[1:, 4] < st[:-1, 4]).any():
            continue
        M = min((n - 1) // stride + 1, MAX_STATIONS)
        nl = clamp(n_layers[b], K)
        if M < 2 or nl < 1:
            continue
        stn = np.clip(np.asarray(station[b][:nl + 1], dtype=np.int64), 0, MAX_STATIONS - 1)
        if (stn[1:] < stn[:-1]).any() or stn[nl] > M - 1:
            continue
        at = np.arange(M) * stride
        S = st[at, 4]
        Vc = np.full(M, np.float64(qp.v_max))
        if v_cap is not None:
            e = np.asarray(v_cap, dtype=np.float64)[b, at]
            with np.errstate(all="ignore"):
                Vc = np.where(e >= 0, vmin(Vc, e), Vc)
        n_q, lo, hi, C = tunnel(S, Vc, stn, nl, None if cells is None else np.asarray(cells)[b], qp)
        rs = ref_states[b, :n_q, 4]
        if not np.isfinite(rs).all():
            continue
        rp = rs - S[0]
        if check_tunnel:
            assert ((rp >= lo) & (rp <= hi)).all(), (b, rp, lo, hi)
        out[-1] = dict(n_q=n_q, lo=lo, hi=hi, C=C, S0=S[0], rp=rp, n=n)
    return out


def bounds_of(group, v0, qp):
    """l, u (dicts of [G, .]) and qv [G, n] of a group of set-up paths with the same n_q."""
    h = np.float64(qp.dts)
    i1, _, _ = inv_steps(h)
    G, n = len(group), group[0]["n_q"]
    a_max, b_max, j_max = (np.float64(getattr(qp, f)) for f in ("a_max", "b_max", "j_max"))
    c0 = np.asarray(v0, dtype=np.float64) * i1
    l = {"p": np.stack([g["lo"] for g in group]), "v": np.zeros((G, n - 1)), "a": np.full((G, n - 1), -b_max), "j": np.full((G, max(n - 3, 0)), -j_max)}
    u = {"p": np.stack([g["hi"] for g in group]), "v": np.stack([g["C"] for g in group]), "a": np.full((G, n - 1), a_max), "j": np.full((G, max(n - 3, 0)), j_max)}
    l["a"][:, 0], u["a"][:, 0] = -b_max + c0, a_max + c0
    two_ws, two_wa = np.float64(2.0) * np.float64(qp.w_s), np.float64(2.0) * np.float64(qp.w_a)
    cv = np.zeros((G, n - 1))
    cv[:, 0] = two_wa * c0
    rp = np.stack([g["rp"] for g in group])
    lin = two_ws * rp + cols_of({"p": np.zeros((G, n)), "v": np.zeros((G, n - 1)), "a": cv, "j": np.zeros((G, max(n - 3, 0)))}, h)
    return l, u, -lin


def solve(states, v0, station, n_layers, ref_states, qp, n_states=None, ok=None, v_cap=None, cells=None, check_tunnel=False):
    """po_speedqp_batch on host arrays, read as the device entry reads them (n_layers and station clamped).  Returns the dict Engine.speedqp_batch returns plus
    x [B, Q] (the iterate, zeros behind n_q), eps_prim [B] and viol [B]: the largest violation of [l, u] by a row of A x."""
    states, v0 = np.asarray(states, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    B, Q, h = states.shape[0], int(qp.Q), np.float64(qp.dts)
    T = times(qp)
    i32 = lambda shape, fill=0: np.full(shape, fill, dtype=np.int32)
    r = {"status": i32(B), "iters": i32(B), "n_fact": i32(B), "r_prim": np.zeros(B), "r_dual": np.zeros(B), "n_q": i32(B), "states": np.zeros((B, Q, 5)),
         "v": np.zeros((B, Q)), "a": np.zeros((B, Q)), "jerk": np.zeros((B, Q)), "t": np.zeros((B, Q)), "lo": np.zeros((B, Q)), "hi": np.zeros((B, Q)),
         "index": i32((B, Q), -1), "x": np.zeros((B, Q)), "eps_prim": np.zeros(B), "viol": np.zeros(B)}
    su = setup(states, v0, station, n_layers, ref_states, qp, n_states=n_states, ok=ok, v_cap=v_cap, cells=cells, check_tunnel=check_tunnel)
    groups = {}
    for b, g in enumerate(su):
        if g is not None:
            groups.setdefault(g["n_q"], []).append(b)
    for n, bs in groups.items():
        group = [su[b] for b in bs]
        if n >= 2:
            l, u, qv = bounds_of(group, v0[bs], qp)
            o = admm(l, u, qv, qp)
            with np.errstate(all="ignore"):
                viol = absmax({c: np.maximum(np.maximum(l[c] - o["ax"][c], o["ax"][c] - u[c]), 0.0) for c in CLASSES})
        for k, b in enumerate(bs):
            g = su[b]
            x = o["x"][k] if n >= 2 else np.zeros(1)
            r["n_q"][b] = n
            if n >= 2:
                for f in ("status", "iters", "n_fact", "r_prim", "r_dual", "eps_prim"):
                    r[f][b] = o[f][k]
                r["viol"][b] = viol[k]
            else:
                r["status"][b] = 1
            rows, idx = sample_rows(states[b, :g["n"]], g["S0"] + x)
            with np.errstate(all="ignore"):
                v = np.concatenate([[v0[b]], (x[1:] - x[:-1]) / h])
                a = np.concatenate([(v[1:] - v[:-1]) / h, [0.0]])
                jk = np.concatenate([(a[1:-1] - a[:-2]) / h, [0.0, 0.0]]) if n >= 2 else np.zeros(1)
            r["states"][b, :n], r["states"][b, n:] = rows, rows[n - 1]
            r["index"][b, :n], r["index"][b, n:] = idx, idx[n - 1]
            r["v"][b, :n], r["v"][b, n:] = v, v[n - 1]
            r["a"][b, :n], r["jerk"][b, :n] = a, jk
            r["t"][b] = T
            r["lo"][b, :n], r["lo"][b, n:] = g["lo"], g["lo"][n - 1]
            r["hi"][b, :n], r["hi"][b, n:] = g["hi"], g["hi"][n - 1]
            r["x"][b, :n] = x
    return r
