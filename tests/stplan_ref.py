"""The definition of po_stplan_batch (include/po_hip.h) in numpy: paths and predicted agents -> blocked (window, station) cells, the cheapest
speed plan through the free ones, v_limit rows.

Tests only.  One ufunc per operation of the definition, in the order it writes them, so every value is the same sequence of rounded IEEE double operations the
kernel runs; comparisons against this file are bit equality.  Phase 1 runs its vectors over the K * M CELLS of one path (agents, pieces and circles are Python
loops in the definition's order); the search runs them over the stations j for one (k, u, u') at a time, u' ascending, which is the definition's scan order
(tests/test_stplan.py checks this file against a scalar loop).  Circle centres, agents that cover nothing and the order of an agent's pieces are dynamic_ref's."""
import numpy as np

import dynamic_ref
import select_ref
from select_ref import DBL_MAX, vmax, vmin

MAX_LAYERS, MAX_STEP, MAX_STATIONS = 16, 31, 128


def blocked_cells(params, st, agents, lo, hi, sp, want_gap=False):
    """cell [K, M] of ONE planned path: st [M, 5] the rows of its stations, agents lo .. hi - 1 of the record array.  want_gap: also the smallest gap of every
    cell over all its evaluations [K, M] (DBL_MAX where there was none) — what the tests place a margin beside; the kernel does not report it."""
    K, M = int(sp.K), len(st)
    _, _, cr = select_ref.car_circles(params)
    gx, gy = dynamic_ref.centres(params, st)
    kk, mm = np.repeat(np.arange(K), M), np.tile(np.arange(M), K)
    dt, margin = np.float64(sp.dt), np.float64(sp.margin)
    t0, t1 = kk.astype(np.float64) * dt, (kk + 1).astype(np.float64) * dt
    cell = np.full(K * M, -1, dtype=np.int32)
    gmin = np.full(K * M, DBL_MAX)
    with np.errstate(all="ignore"):
        for a in range(lo, hi):
            ag = agents[a]
            np_ = dynamic_ref.covers(ag)
            if not np_:
                continue
            T, X, Y, R = ag["t"], ag["x"], ag["y"], np.float64(ag["radius"])
            for kind, j in dynamic_ref.pieces(ag, np_):
                if kind == "before":
                    ta, tb = t0, vmin(t1, T[0])
                    axa = axb = np.full(K * M, X[0]); aya = ayb = np.full(K * M, Y[0])
                elif kind == "after":
                    ta, tb = vmax(t0, T[j]), t1
                    axa = axb = np.full(K * M, X[j]); aya = ayb = np.full(K * M, Y[j])
                else:
                    D = T[j + 1] - T[j]
                    if not (D > 0):
                        continue
                    ta, tb = vmax(t0, T[j]), vmin(t1, T[j + 1])
                    wa, wb = (ta - T[j]) / D, (tb - T[j]) / D
                    DX, DY = X[j + 1] - X[j], Y[j + 1] - Y[j]
                    axa, aya = X[j] + wa * DX, Y[j] + wa * DY
                    axb, ayb = X[j] + wb * DX, Y[j] + wb * DY
                live = ta <= tb
                if not live.any():
                    continue
                for q in range(6):
                    rax, ray, rbx, rby = gx[mm, q] - axa, gy[mm, q] - aya, gx[mm, q] - axb, gy[mm, q] - ayb
                    dx, dy, px, py = rbx - rax, rby - ray, -rax, -ray
                    L2, dot = dx * dx + dy * dy, px * dx + py * dy
                    u = np.where(L2 > 0, dot / L2, 0.0)
                    u = np.where(u < 0, 0.0, u)
                    u = np.where(u > 1, 1.0, u)
                    qx, qy = px - u * dx, py - u * dy
                    gap = (np.sqrt(qx * qx + qy * qy) - cr[q]) - R
                    cell = np.where(live & (gap < margin) & (cell < 0), np.int32(a), cell)
                    gmin = np.where(live & (gap < gmin), gap, gmin)
    return (cell.reshape(K, M), gmin.reshape(K, M)) if want_gap else cell.reshape(K, M)


def step_table(S, Vc, sp):
    """v, c [M, U + 1] and the mask of the pairs that exist (u <= min(U, j))."""
    M, U, dt = len(S), int(sp.U), np.float64(sp.dt)
    v, c, exists = np.zeros((M, U + 1)), np.zeros((M, U + 1)), np.zeros((M, U + 1), dtype=bool)
    with np.errstate(all="ignore"):
        for u in range(min(U, M - 1) + 1):
            j = np.arange(u, M)
            v[j, u] = (S[j] - S[j - u]) / dt
            cc = Vc[j - u]
            for off in range(1, u + 1):
                cc = vmin(cc, Vc[j - u + off])
            c[j, u] = cc
            exists[j, u] = True
    return v, c, exists


def search(S, Vc, cell, v0, sp):
    """The search and the choice of ONE path: (n_layers, cost, stations [n_layers + 1]) or None when there is no candidate."""
    M, U, K = len(S), int(sp.U), int(sp.K)
    dt, a_max, b_max, w_acc, w_slow = (np.float64(getattr(sp, f)) for f in ("dt", "a_max", "b_max", "w_acc", "w_slow"))
    v, c, exists = step_table(S, Vc, sp)
    pre = np.concatenate([np.zeros((K, 1), dtype=np.int64), np.cumsum(cell >= 0, axis=1)], axis=1)  # blocked cells in front of station m
    with np.errstate(all="ignore"):
        drivable = exists & ((np.arange(U + 1)[None, :] == 0) | ((v > 0) & (v <= c)))
        dv = c - v
        slow = (w_slow * dv) * dv
        bp = np.zeros((K + 1, M, U + 1), dtype=np.int64)
        prev, best = None, (DBL_MAX, 0, 0, 0)
        for k in range(1, K + 1):
            cur = np.full((M, U + 1), DBL_MAX)
            for u in range(min(U, M - 1) + 1):
                j = np.arange(u, M)
                p = j - u
                base = drivable[j, u] & ((pre[k - 1, j + 1] - pre[k - 1, p]) == 0) & (p != M - 1)
                for up in ([0] if k == 1 else range(1 if u > 0 else 0, U + 1)):
                    if k == 1:
                        feas, vp, cp = base & (p == 0), np.full(len(j), v0), np.zeros(len(j))
                    else:
                        feas = base & (up <= p)
                        cp = np.where(feas, prev[p, up], DBL_MAX)
                        feas, vp = feas & (cp < DBL_MAX), v[p, up]
                    if not feas.any():
                        continue
                    acc = (v[j, u] - vp) / dt
                    feas = feas & (acc <= a_max) & (acc >= -b_max)
                    cand = cp + ((w_acc * acc) * acc + slow[j, u])
                    take = feas & (cand < cur[j, u])
                    cur[j, u] = np.where(take, cand, cur[j, u])
                    bp[k, j, u] = np.where(take, up, bp[k, j, u])
            rows = cur if k == K else cur[M - 1:]
            i = int(np.argmin(rows))  # the first of the minima in (j, u) order
            if rows.flat[i] < best[0]:
                best = (rows.flat[i], k, i // (U + 1) + (0 if k == K else M - 1), i % (U + 1))
            prev = cur
    if best[1] == 0:
        return None
    cost, nl, j, u = best
    stations = [0] * (nl + 1)
    for k in range(nl, 0, -1):
        stations[k] = j
        j, u = j - u, int(bp[k, j, u])
    stations[0] = j
    return nl, cost, stations


def plan(params, states, v0, agents, first, sp, n_states=None, ok=None, v_cap=None, set_of=None, v_limit_in=None):
    """po_stplan_batch on host arrays: agents / first as binding.pack_agents returns them (unvalidated: read as the device entry reads them).  Returns the dict
    Engine.stplan_batch returns."""
    states, v0 = np.asarray(states, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    B, N = states.shape[0], states.shape[1]
    S_, n_agents, K, stride, dt = len(first) - 1, len(agents), int(sp.K), int(sp.stride), np.float64(sp.dt)
    clamp = lambda v, hi: min(max(int(v), 0), hi)
    L = np.full((B, N), -1.0) if v_limit_in is None else np.array(v_limit_in, dtype=np.float64)
    r = {"status": np.zeros(B, dtype=np.int32), "ok_out": np.zeros(B, dtype=np.int32), "n_layers": np.zeros(B, dtype=np.int32), "cost": np.full(B, DBL_MAX),
         "station": np.full((B, MAX_LAYERS + 1), -1, dtype=np.int32), "cells": np.full((B, K, MAX_STATIONS), -1, dtype=np.int32), "v_limit": L.copy()}
    for b in range(B):
        n = N if n_states is None else clamp(n_states[b], N)
        st = states[b, :n]
        if (ok is not None and ok[b] == 0) or n < 2 or not (np.isfinite(v0[b]) and v0[b] >= 0) or not np.isfinite(st[:, [0, 1, 2, 4]]).all():
            continue
        M = min((n - 1) // stride + 1, MAX_STATIONS)
        if M < 2:
            continue
        at = np.arange(M) * stride
        S = st[at, 4]
        Vc = np.full(M, np.float64(sp.v_max))
        if v_cap is not None:
            e = np.asarray(v_cap, dtype=np.float64)[b, at]
            with np.errstate(all="ignore"):
                Vc = np.where(e >= 0, vmin(Vc, e), Vc)
        ks = 0 if set_of is None else clamp(set_of[b], S_ - 1)
        lo, hi = clamp(first[ks], n_agents), clamp(first[ks + 1], n_agents)
        cell = blocked_cells(params, st[at], agents, lo, hi, sp)
        r["cells"][b, :, :M] = cell
        found = search(S, Vc, cell, v0[b], sp)
        if found is None:
            r["status"][b] = 3
            continue
        nl, cost, stations = found
        r["status"][b], r["ok_out"][b], r["n_layers"][b], r["cost"][b] = (1 if (cell < 0).all() else 2), 1, nl, cost
        r["station"][b, :nl + 1] = stations
        m = np.arange(n) // stride
        row = L[b, :n].copy()
        if stations[nl] == stations[nl - 1]:
            row[m >= stations[nl]] = 0.0
        with np.errstate(all="ignore"):
            for k in range(nl):
                inside = (stations[k] <= m) & (m < stations[k + 1])
                V = (S[stations[k + 1]] - S[stations[k]]) / dt
                row = np.where(inside, np.where(row >= 0, vmin(row, V), V), row)
        r["v_limit"][b, :n] = row
    return r
