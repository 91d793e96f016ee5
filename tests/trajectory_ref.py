"""The definition of po_trajectory_batch (include/po_hip.h) in numpy: speed-profiled paths -> K samples at uniform time steps, a status,
and the samples as po_agent records.

Tests only.  One ufunc per operation of the definition, in the order it writes them, so every value is the same sequence of rounded IEEE double operations the
kernel runs; comparisons against this file are bit equality.  The vectors run over the SAMPLES of one path; paths are a Python loop (tests/test_trajectory.py
checks this file against a scalar loop).  The interval of a sample is numpy's searchsorted on the t row: t is non-decreasing, so the largest i with t_i <= T is
the same whatever finds it.  Portable sin / cos: select_ref's."""
import numpy as np

import select_ref

PI, TWO_PI = np.float64(3.141592653589793), np.float64(6.283185307179586)
MAX_PTS, MAX_DISCS = 8, 4
AGENT_DTYPE = np.dtype([("n_pts", np.int32), ("flags", np.int32), ("radius", np.float64), ("t", np.float64, (8,)), ("x", np.float64, (8,)), ("y", np.float64, (8,))])


def sampled(st, v, t, okb=1):
    """The status-0 test on the rows < n of one path: st [n, 5], v, t [n]."""
    n = len(st)
    if okb == 0 or n < 1 or not (np.isfinite(st).all() and np.isfinite(v).all() and np.isfinite(t).all()):
        return False
    return bool((v >= 0).all() and not (t[1:] < t[:-1]).any())


def end_state(st, v):
    """E: the smallest i < n - 1 with v_i == 0, v_{i+1} == 0 and s_{i+1} - s_i > 0; n - 1 when there is none."""
    rest = np.flatnonzero((v[:-1] == 0) & (v[1:] == 0) & ((st[1:, 4] - st[:-1, 4]) > 0))
    return int(rest[0]) if len(rest) else len(st) - 1


def times(tp):
    """T_k = t0 + (double)k * dt, k < K."""
    with np.errstate(all="ignore"):
        return np.float64(tp.t0) + np.arange(int(tp.K)).astype(np.float64) * np.float64(tp.dt)


def path_samples(st, v, t, T):
    """The samples of ONE sampled path at the times T [K]: a dict of x, y, z, k, s, v, a [K], index [K], held [K], and lam, lam_raw [K] (NaN where the sample is
    not interpolated), E."""
    K = len(T)
    E = end_state(st, v)
    held = T >= t[E]
    early = ~held & (T < t[0])
    mid = ~held & ~early
    i = np.where(held, E, 0)
    i[mid] = np.searchsorted(t[:E + 1], T[mid], side="right") - 1
    j = np.where(mid, i + 1, i)  # row i + 1 where there is one to read
    o = {c: st[i, q].copy() for q, c in enumerate("xyzks")}
    o.update(v=v[i].copy(), a=np.zeros(K), index=i.astype(np.int32), held=held, E=E, lam=np.full(K, np.nan), lam_raw=np.full(K, np.nan))
    with np.errstate(all="ignore"):
        Dt = t[j] - t[i]
        tau = T - t[i]
        acc = (v[j] - v[i]) / Dt
        sig = (v[i] + (np.float64(0.5) * acc) * tau) * tau
        ds = st[j, 4] - st[i, 4]
        raw = np.where(ds > 0, sig / ds, 0.0)
        lam = np.where(raw < 0, 0.0, raw)
        lam = np.where(lam > 1, 1.0, lam)
        x = st[i, 0] + lam * (st[j, 0] - st[i, 0])
        y = st[i, 1] + lam * (st[j, 1] - st[i, 1])
        k = st[i, 3] + lam * (st[j, 3] - st[i, 3])
        s = st[i, 4] + lam * ds
        dz = st[j, 2] - st[i, 2]
        dz = np.where(dz > PI, dz - TWO_PI, np.where(dz < -PI, dz + TWO_PI, dz))
        z = st[i, 2] + lam * dz
        vv = v[i] + acc * tau
        vv = np.where(vv > 0, vv, 0.0)
    for c, val in (("x", x), ("y", y), ("z", z), ("k", k), ("s", s), ("v", vv), ("a", acc), ("lam", lam), ("lam_raw", raw)):
        o[c] = np.where(mid, val, o[c])
    return o


def trajectory(states, v, t, tp, n_states=None, ok=None):
    """po_trajectory_batch on host arrays.  Returns the dict Engine.trajectory_batch returns (agents: records of AGENT_DTYPE, None when n_discs = 0), plus lam and
    lam_raw [B, K] (NaN where a sample is not interpolated), held [B, K] and E [B] (-1 when not sampled)."""
    states, v, t = (np.asarray(a, dtype=np.float64) for a in (states, v, t))
    B, N = states.shape[0], states.shape[1]
    K, D, P, stride = int(tp.K), int(tp.n_discs), int(tp.agent_pts), int(tp.agent_stride)
    T = times(tp)
    r = {"status": np.zeros(B, dtype=np.int32), "states": np.zeros((B, K, 5)), "v": np.zeros((B, K)), "a": np.zeros((B, K)), "t": np.zeros((B, K)),
         "index": np.full((B, K), -1, dtype=np.int32), "first_held": np.full(B, -1, dtype=np.int32), "agents": np.zeros(B * D, dtype=AGENT_DTYPE) if D > 0 else None,
         "lam": np.full((B, K), np.nan), "lam_raw": np.full((B, K), np.nan), "held": np.zeros((B, K), dtype=bool), "E": np.full(B, -1)}
    for b in range(B):
        n = N if n_states is None else min(max(int(n_states[b]), 0), N)
        st, vb, tb = states[b, :n], v[b, :n], t[b, :n]
        if not sampled(st, vb, tb, 1 if ok is None else int(ok[b])):
            continue
        o = path_samples(st, vb, tb, T)
        for q, c in enumerate("xyzks"):
            r["states"][b, :, q] = o[c]
        r["v"][b], r["a"][b], r["t"][b], r["index"][b] = o["v"], o["a"], T, o["index"]
        r["lam"][b], r["lam_raw"][b], r["held"][b], r["E"][b] = o["lam"], o["lam_raw"], o["held"], o["E"]
        first = np.flatnonzero(o["held"])
        fh = int(first[0]) if len(first) else K
        r["first_held"][b] = fh
        r["status"][b] = 1 if fh == K else (2 if vb[o["E"]] == 0 else 3)
        if D > 0:
            ks = np.arange(P) * stride
            cz, sz = select_ref._trig(o["z"][ks])
            for d in range(D):
                g = r["agents"][b * D + d]
                g["n_pts"], g["flags"], g["radius"] = P, int(tp.agent_flags), tp.disc_radius[d]
                g["t"][:P] = T[ks]
                g["x"][:P] = o["x"][ks] + np.float64(tp.disc_offset[d]) * cz
                g["y"][:P] = o["y"][ks] + np.float64(tp.disc_offset[d]) * sz
    return r
