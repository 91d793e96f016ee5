"""The definition of po_stgo_batch (include/po_hip.h) in numpy: paths and predicted agents -> blocked (window, station) cells, the cheapest
speed plan through the free ones WITH resuming after a stop allowed, and that plan sampled at uniform time steps.

Tests only.  One ufunc per operation of the definition, in the order it writes them, so every value is the same sequence of rounded IEEE double operations the
kernel runs; comparisons against this file are bit equality.  Blocked cells and the step table are stplan_ref's functions themselves (the definition is the same
text); the search is stplan_ref.search with the one clause "for k > 1, u' == 0 implies u == 0" deleted, which that function cannot be asked to do, so it is written
out here (tests/test_stgo.py checks it, and the sampler, against a scalar loop).  The sampler's interpolation is trajectory_ref's line by line, with
lam = (sx - s_i) / ds in the place of sig / ds; PI and TWO_PI are its constants.  The vectors of the sampler run over the SAMPLES of one path; the state of a
moving sample is numpy's searchsorted on the s rows of its edge: s is non-decreasing, so the largest i with s_i <= sx is the same whatever finds it."""
import numpy as np

import stplan_ref
from select_ref import DBL_MAX
from stplan_ref import MAX_LAYERS, MAX_STATIONS
from trajectory_ref import PI, TWO_PI


def search(S, Vc, cell, v0, gp):
    """The search and the choice of ONE path: (n_layers, cost, stations [n_layers + 1]) or None when there is no candidate.  A predecessor at rest (u' == 0) may
    have any successor."""
    M, U, K = len(S), int(gp.U), int(gp.K)
    dt, a_max, b_max, w_acc, w_slow = (np.float64(getattr(gp, f)) for f in ("dt", "a_max", "b_max", "w_acc", "w_slow"))
    v, c, exists = stplan_ref.step_table(S, Vc, gp)
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
                for up in ([0] if k == 1 else range(0, U + 1)):
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


def times(gp):
    """T_q = t0 + (double)q * dts, q < Q."""
    with np.errstate(all="ignore"):
        return np.float64(gp.t0) + np.arange(int(gp.Q)).astype(np.float64) * np.float64(gp.dts)


def plan_speeds(S, stations, v0, dt):
    """V [nl + 1] and A [nl + 1] (A_0 unused, 0): V_0 = v0, V_k = v(station[k], u_k), A_k = (V_k - V_{k-1}) / dt."""
    stn = np.asarray(stations)
    with np.errstate(all="ignore"):
        V = np.concatenate([[np.float64(v0)], (S[stn[1:]] - S[stn[:-1]]) / dt])
        A = np.concatenate([[0.0], (V[1:] - V[:-1]) / dt])
    return V, A


def path_samples(st, S, stations, v0, gp, T):
    """The samples of ONE planned path at the times T [Q]: a dict of x, y, z, k, s, v, a [Q], index [Q], held [Q], kk [Q] (-1 where T < 0) and lam [Q] (NaN where
    the sample is not interpolated)."""
    Q, nl, stride, dt = len(T), len(stations) - 1, int(gp.stride), np.float64(gp.dt)
    stn = np.asarray(stations)
    V, A = plan_speeds(S, stations, v0, dt)
    with np.errstate(all="ignore"):
        kt = np.arange(nl + 1).astype(np.float64) * dt
        early = T < 0
        kk = np.where(early, -1, np.searchsorted(kt, T, side="right") - 1)  # the largest k with (double)k * dt <= T
        held = ~early & (kk == nl)
        edge = ~early & ~held
        k0 = np.where(edge, kk, 0)
        p, j = stn[k0], stn[k0 + 1]
        standing, moving = edge & (j == p), edge & (j != p)
        row = np.where(early, 0, np.where(held, stn[nl] * stride, p * stride))  # the state of a sample that is a row
        tau = T - k0.astype(np.float64) * dt
        sig = V[k0 + 1] * tau
        sx = S[p] + sig
        sx = np.where(sx > S[j], S[j], sx)
        i = row.copy()
        for q in np.flatnonzero(moving):
            lo, hi = p[q] * stride, j[q] * stride
            i[q] = lo + np.searchsorted(st[lo:hi, 4], sx[q], side="right") - 1
        i1 = np.where(moving, i + 1, i)
        ds = st[i1, 4] - st[i, 4]
        lam = np.where(ds > 0, (sx - st[i, 4]) / ds, 0.0)
        lam = np.where(lam < 0, 0.0, lam)
        lam = np.where(lam > 1, 1.0, lam)
        x = st[i, 0] + lam * (st[i1, 0] - st[i, 0])
        y = st[i, 1] + lam * (st[i1, 1] - st[i, 1])
        k = st[i, 3] + lam * (st[i1, 3] - st[i, 3])
        s = st[i, 4] + lam * ds
        dz = st[i1, 2] - st[i, 2]
        dz = np.where(dz > PI, dz - TWO_PI, np.where(dz < -PI, dz + TWO_PI, dz))
        z = st[i, 2] + lam * dz
    o = {c: st[row, q].copy() for q, c in enumerate("xyzks")}
    for c, val in (("x", x), ("y", y), ("z", z), ("k", k), ("s", s)):
        o[c] = np.where(moving, val, o[c])
    o["v"] = np.where(early, np.float64(v0), np.where(held, V[nl], np.where(standing, 0.0, V[k0 + 1])))
    o["a"] = np.where(edge, A[k0 + 1], 0.0)
    o.update(index=i.astype(np.int32), held=held, kk=kk, lam=np.where(moving, lam, np.nan))
    return o


def plan(params, states, v0, agents, first, gp, n_states=None, ok=None, v_cap=None, set_of=None):
    """po_stgo_batch on host arrays: agents / first as binding.pack_agents returns them (unvalidated: read as the device entry reads them).  Returns the dict
    Engine.stgo_batch returns, plus lam [B, Q] (NaN where a sample is not interpolated) and kk [B, Q] (the window of a sample; -1 before time 0 and without a plan)."""
    states, v0 = np.asarray(states, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    B, N = states.shape[0], states.shape[1]
    S_, n_agents, K, stride, Q = len(first) - 1, len(agents), int(gp.K), int(gp.stride), int(gp.Q)
    clamp = lambda v, hi: min(max(int(v), 0), hi)
    T = times(gp)
    i32 = lambda shape, fill=0: np.full(shape, fill, dtype=np.int32)
    r = {"status": i32(B), "ok_out": i32(B), "n_layers": i32(B), "cost": np.full(B, DBL_MAX), "station": i32((B, MAX_LAYERS + 1), -1),
         "cells": i32((B, K, MAX_STATIONS), -1), "n_resumes": i32(B), "states": np.zeros((B, Q, 5)), "v": np.zeros((B, Q)), "a": np.zeros((B, Q)),
         "t": np.zeros((B, Q)), "index": i32((B, Q), -1), "first_held": i32(B, -1), "end": i32(B), "lam": np.full((B, Q), np.nan), "kk": i32((B, Q), -1)}
    for b in range(B):
        n = N if n_states is None else clamp(n_states[b], N)
        st = states[b, :n]
        if (ok is not None and ok[b] == 0) or n < 2 or not (np.isfinite(v0[b]) and v0[b] >= 0) or not np.isfinite(st[:, [0, 1, 2, 4]]).all():
            continue
        if (st[1:, 4] < st[:-1, 4]).any():  # the sampler looks a state up by s
            continue
        M = min((n - 1) // stride + 1, MAX_STATIONS)
        if M < 2:
            continue
        at = np.arange(M) * stride
        S = st[at, 4]
        Vc = np.full(M, np.float64(gp.v_max))
        if v_cap is not None:
            e = np.asarray(v_cap, dtype=np.float64)[b, at]
            with np.errstate(all="ignore"):
                Vc = np.where(e >= 0, stplan_ref.vmin(Vc, e), Vc)
        ks = 0 if set_of is None else clamp(set_of[b], S_ - 1)
        lo, hi = clamp(first[ks], n_agents), clamp(first[ks + 1], n_agents)
        cell = stplan_ref.blocked_cells(params, st[at], agents, lo, hi, gp)
        r["cells"][b, :, :M] = cell
        found = search(S, Vc, cell, v0[b], gp)
        if found is None:
            r["status"][b] = 3
            continue
        nl, cost, stations = found
        r["status"][b], r["ok_out"][b], r["n_layers"][b], r["cost"][b] = (1 if (cell < 0).all() else 2), 1, nl, cost
        r["station"][b, :nl + 1] = stations
        u = np.diff(stations)
        r["n_resumes"][b] = int(((u[:-1] == 0) & (u[1:] > 0)).sum())
        o = path_samples(st, S, stations, v0[b], gp, T)
        for q, c in enumerate("xyzks"):
            r["states"][b, :, q] = o[c]
        r["v"][b], r["a"][b], r["t"][b], r["index"][b], r["lam"][b], r["kk"][b] = o["v"], o["a"], T, o["index"], o["lam"], o["kk"]
        held = np.flatnonzero(o["held"])
        fh = int(held[0]) if len(held) else Q
        r["first_held"][b] = fh
        r["end"][b] = 1 if fh == Q else (2 if stations[nl] == M - 1 else (3 if u[nl - 1] == 0 else 4))
    return r
