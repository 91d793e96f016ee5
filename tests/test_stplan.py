"""Station-time speed planning: po_stplan_batch* (csrc/po_stplan.hip; include/po_hip.h states the definition).

Every cell, cost, station and v_limit entry is a fixed sequence of rounded IEEE double operations and integer choices, so every comparison with the device here is
BIT equality on byte views against tests/stplan_ref.py (numpy, one ufunc per operation).  There is no tolerance in this file: the closed scenes are built on a grid
(stations 1 m apart, dt = 1 s, caps of whole m/s), where every speed, acceleration and cost is a small integer and exact.

CPU: the reference against a scalar loop over the definition, closed scenes (accelerating to the cap, a held agent, a crosser the plan eases off behind, an agent the
plan passes ahead of, a blocked first cell), properties of the reference on random inputs, the all-ties case, every status-0 trigger, the closure stplan -> speed ->
dynamic on the three references, exports and the ABI mirror, argument and range checks without a device, the kernel's chunk constant, the host mirror compiles and
links.  GPU: station counts around one and two waves and at the clamp, strides, layer and step counts at their limits (and all three limits in one call: the largest LDS), agent counts around the LDS chunk, batch
sizes, position in the batch, sets, every kind of piece with boundaries on the window times, the margin one ulp either side of a gap, the all-ties case, a v0 no
braking absorbs, status-0 triggers, NULL optional inputs and outputs, empty calls, lists read clamped, the chain stplan -> speed -> dynamic on one stream, the C++
mirror's program against the Python call, host validation."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import dynamic_ref
import select_ref
import speed_ref
import stplan_ref
from path_optimizer_amd import abi, binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["po_default_stplan_params", "po_stplan_batch", "po_stplan_batch_device"]
KEYS = ("status", "ok_out", "n_layers", "cost", "station", "cells", "v_limit")
DBL_MAX = select_ref.DBL_MAX
BEFORE, AFTER = abi.PO_AGENT_HOLD_BEFORE, abi.PO_AGENT_HOLD_AFTER
ST_CHUNK = 32  # kAgentChunk of po_agents.hpp (po_stplan.hip's chunk): agents per LDS chunk
MAX_M = abi.PO_ST_MAX_STATIONS


def test_boundary_cases_follow_the_kernel_constant():
    """The agent counts below are built from ST_CHUNK: it must be the kernel's own constant."""
    agents = open(os.path.join(ROOT, "path_optimizer_amd", "csrc", "po_agents.hpp")).read()
    assert int(re.search(r"constexpr int kAgentChunk = (\d+);", agents).group(1)) == ST_CHUNK


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(got, want, keys=KEYS, tag=""):
    for k in keys:
        if not same(got[k], want[k]):
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert g.shape == w.shape and g.dtype == w.dtype, (tag, k, g.shape, w.shape, g.dtype, w.dtype)
            bad = np.flatnonzero((g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)).any(axis=1))
            raise AssertionError(f"{tag} {k}: paths {bad[:8]} differ; got {g[bad[0]]} want {w[bad[0]]}")


def params_of(**kw):
    sp = binding.default_stplan_params()
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


def small(**kw):
    """Knobs for the random cases: states about 0.3 m apart, so stations 0.6 m apart and speeds in steps of 1.2 m/s; a search small enough for the reference."""
    return params_of(**dict(dict(dt=0.5, K=5, stride=2, U=6, margin=0.4), **kw))


def straight(n, ds, y=0.0, N=None):
    """One straight path along +x from the origin: states [1, N, 5]."""
    N = N or n
    st = np.zeros((1, N, 5))
    st[0, :n, 0] = ds * np.arange(n); st[0, :n, 1] = y; st[0, :n, 4] = ds * np.arange(n)
    return st


def disc(x, y, r, flags=BEFORE | AFTER, t=0.0):
    return (r, flags, [(t, x, y)])


def make_paths(seed, B, N, ds=0.3, box=4.0):
    """B smooth paths of N states around the origin."""
    rng = np.random.default_rng([29, seed])
    st = np.zeros((B, N, 5))
    for b in range(B):
        step = ds * rng.uniform(0.7, 1.3, N - 1) if N > 1 else np.zeros(0)
        s = np.concatenate(([0.0], np.cumsum(step)))
        k = rng.uniform(0, 0.15) * np.sin(s / rng.uniform(3, 9) + rng.uniform(0, 6.28))
        z = rng.uniform(-math.pi, math.pi) + np.concatenate(([0.0], np.cumsum(0.5 * (k[1:] + k[:-1]) * step)))
        x = rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(np.cos(z[:-1]) * step)))
        y = rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(np.sin(z[:-1]) * step)))
        st[b] = np.stack([x, y, z, k, s], axis=1)
    return st


def random_agents(rng, count, box=8.0, horizon=4.0):
    """Agents with 1 .. 8 points, every flag combination, radii 0.1 .. 0.6, walking about the box within the horizon."""
    out = []
    for _ in range(count):
        npts = int(rng.integers(1, 9))
        tt = rng.uniform(-1.0, horizon / 2) + np.concatenate(([0.0], np.cumsum(rng.uniform(0.1, horizon / 8, npts - 1))))
        x = rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(rng.uniform(-2, 2, npts - 1))))
        y = rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(rng.uniform(-2, 2, npts - 1))))
        out.append((rng.uniform(0.1, 0.6), int(rng.integers(0, 4)), list(zip(tt, x, y))))
    return out


def random_case(seed, B, N, per_set=(5, 0, 9), ragged=True, extras=True):
    """Ragged paths, S sets of agents, a set per path, speeds 0 .. 4 m/s, and (extras) a v_cap and a v_limit_in with negative and NaN entries."""
    rng = np.random.default_rng([30, seed])
    st = make_paths(seed, B, N)
    n = rng.integers(0, N + 1, B).astype(np.int32) if ragged else np.full(B, N, dtype=np.int32)
    n[rng.integers(0, B)] = N
    sets = [random_agents(rng, c) for c in per_set]
    c = dict(states=st, v0=rng.uniform(0, 4, B), n_states=n, agents=binding.pack_agents(sets), set_of=rng.integers(0, len(per_set), B).astype(np.int32))
    if extras:
        for key, lo, hi in (("v_cap", 2, 9), ("v_limit_in", 1, 9)):
            a = rng.uniform(lo, hi, (B, N))
            a[rng.random((B, N)) < 0.4] = -1.0
            a[rng.random((B, N)) < 0.1] = np.nan
            c[key] = a
    return c


def ref(oracle, sp=None, **c):
    c = dict(c)
    agents, first = binding.pack_agents(c.pop("agents"))
    return stplan_ref.plan(oracle.default_params(), c.pop("states"), c.pop("v0"), agents, first, sp or params_of(), **c)


def edges_of(r, b=0):
    """(stations, u per edge) of a planned path."""
    nl = int(r["n_layers"][b])
    s = r["station"][b, :nl + 1].astype(int)
    return s, np.diff(s)


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def _scalar_plan(params, st, v0, n, okb, agents, first, ks, cap, lim, sp):
    """The definition as a plain scalar Python loop over ONE path (Python floats are IEEE doubles; every operation rounds once).  st [N, 5]."""
    N, K, U, stride = len(st), int(sp.K), int(sp.U), int(sp.stride)
    dt, margin, a_max, b_max, v_max, w_acc, w_slow = (float(getattr(sp, f)) for f in ("dt", "margin", "a_max", "b_max", "v_max", "w_acc", "w_slow"))
    n = min(max(int(n), 0), N)
    L = [-1.0 if lim is None else float(v) for v in (lim if lim is not None else range(N))]
    out = dict(status=0, ok_out=0, n_layers=0, cost=DBL_MAX, station=[-1] * 17, cells=[[-1] * MAX_M for _ in range(K)], v_limit=list(L))
    fin = lambda v: abs(v) <= DBL_MAX
    mn = lambda a, b: b if b < a else a
    mx = lambda a, b: b if b > a else a
    x, y, z, _, s = ([float(v) for v in st[:n, c]] for c in range(5))
    v0 = float(v0)
    if okb == 0 or n < 2 or not (fin(v0) and v0 >= 0) or not all(fin(v) for v in x + y + z + s):
        return out
    M = min((n - 1) // stride + 1, MAX_M)
    if M < 2:
        return out
    T = select_ref.trig_lib()
    cx, cy, cr = ([float(v) for v in arr] for arr in select_ref.car_circles(params))
    S, Vc, gx, gy = [], [], [], []
    for m in range(M):
        i = m * stride
        S.append(s[i])
        vc = v_max
        if cap is not None and float(cap[i]) >= 0:
            vc = mn(vc, float(cap[i]))
        Vc.append(vc)
        cz, sz = T.po_oracle_pcos(z[i]), T.po_oracle_psin(z[i])
        gx.append([(cx[q] * cz - cy[q] * sz) + x[i] for q in range(6)])
        gy.append([(cx[q] * sz + cy[q] * cz) + y[i] for q in range(6)])
    n_sets, n_agents = len(first) - 1, len(agents)
    cl = lambda v, hi: min(max(int(v), 0), hi)
    ks = cl(ks, n_sets - 1)
    lo, hi = cl(first[ks], n_agents), cl(first[ks + 1], n_agents)
    cells = out["cells"]
    for k in range(K):
        tk, tk1 = float(k) * dt, float(k + 1) * dt
        for m in range(M):
            for a in range(lo, hi):
                if cells[k][m] >= 0:
                    break
                ag = agents[a]
                npts, R, flags = int(ag["n_pts"]), float(ag["radius"]), int(ag["flags"])
                if npts < 1 or npts > 8 or not R >= 0:
                    continue
                AT, AX, AY = ([float(v) for v in ag[f][:npts]] for f in ("t", "x", "y"))
                if not all(fin(v) for v in AT + AX + AY):
                    continue
                for p in ([-1] if flags & 1 else []) + list(range(npts - 1)) + ([npts - 1] if flags & 2 else []):
                    if p < 0:
                        ta, tb = tk, mn(tk1, AT[0])
                        pa = pb = (AX[0], AY[0])
                    elif p == npts - 1:
                        ta, tb = mx(tk, AT[p]), tk1
                        pa = pb = (AX[p], AY[p])
                    else:
                        D = AT[p + 1] - AT[p]
                        if not D > 0:
                            continue
                        ta, tb = mx(tk, AT[p]), mn(tk1, AT[p + 1])
                        wa, wb = (ta - AT[p]) / D, (tb - AT[p]) / D
                        pa = (AX[p] + wa * (AX[p + 1] - AX[p]), AY[p] + wa * (AY[p + 1] - AY[p]))
                        pb = (AX[p] + wb * (AX[p + 1] - AX[p]), AY[p] + wb * (AY[p + 1] - AY[p]))
                    if not ta <= tb:
                        continue
                    for q in range(6):
                        rax, ray, rbx, rby = gx[m][q] - pa[0], gy[m][q] - pa[1], gx[m][q] - pb[0], gy[m][q] - pb[1]
                        dx, dy, px, py = rbx - rax, rby - ray, -rax, -ray
                        L2, dot = dx * dx + dy * dy, px * dx + py * dy
                        u = dot / L2 if L2 > 0 else 0.0
                        u = 0.0 if u < 0 else u
                        u = 1.0 if u > 1 else u
                        qx, qy = px - u * dx, py - u * dy
                        gap = (math.sqrt(qx * qx + qy * qy) - cr[q]) - R
                        if gap < margin and cells[k][m] < 0:
                            cells[k][m] = a
    v = lambda j, u: (S[j] - S[j - u]) / dt

    def c(j, u):
        cc = Vc[j - u]
        for m in range(j - u + 1, j + 1):
            cc = mn(cc, Vc[m])
        return cc

    prev, bp, best = None, {}, (DBL_MAX, 0, 0, 0)
    for k in range(1, K + 1):
        cur = {}
        for j in range(M):
            for u in range(min(U, j) + 1):
                p = j - u
                val, arg = DBL_MAX, 0
                drivable = u == 0 or (v(j, u) > 0 and v(j, u) <= c(j, u))
                clear = all(cells[k - 1][m] < 0 for m in range(p, j + 1))
                for up in ([0] if k == 1 else range(min(U, p) + 1)):
                    if k == 1:
                        if p != 0:
                            continue
                        cp, vp = 0.0, v0
                    else:
                        cp, vp = prev[(p, up)], v(p, up)
                        if up == 0 and u != 0:
                            continue
                    if not cp < DBL_MAX or p == M - 1 or not (drivable and clear):
                        continue
                    acc = (v(j, u) - vp) / dt
                    if not (acc <= a_max and acc >= -b_max):
                        continue
                    dv = c(j, u) - v(j, u)
                    cand = cp + ((w_acc * acc) * acc + (w_slow * dv) * dv)
                    if cand < val:
                        val, arg = cand, up
                cur[(j, u)], bp[(k, j, u)] = val, arg
        for j in (range(M) if k == K else [M - 1]):
            for u in range(min(U, j) + 1):
                if cur[(j, u)] < best[0]:
                    best = (cur[(j, u)], k, j, u)
        prev = cur
    out["cells"] = cells
    if best[1] == 0:
        out["status"] = 3
        return out
    cost, nl, j, u = best
    station = [0] * (nl + 1)
    us = [0] * (nl + 1)
    for k in range(nl, 0, -1):
        station[k], us[k] = j, u
        j, u = j - u, bp[(k, j, u)]
    blocked = any(cells[k][m] >= 0 for k in range(K) for m in range(M))
    out.update(status=2 if blocked else 1, ok_out=1, n_layers=nl, cost=cost, station=station + [-1] * (16 - nl))
    for i in range(n):
        m = i // stride
        if m >= station[nl]:
            if us[nl] == 0:
                out["v_limit"][i] = 0.0
            continue
        k = next(k for k in range(nl) if station[k] <= m < station[k + 1])
        V = v(station[k + 1], us[k + 1])
        out["v_limit"][i] = mn(L[i], V) if L[i] >= 0 else V
    return out


def test_reference_agrees_with_a_scalar_loop_over_the_definition(oracle):
    params = oracle.default_params()
    seen = set()
    for case, (B, N, sp) in enumerate([(10, 21, small()), (8, 30, small(K=3, stride=3, U=2, margin=0.8)), (6, 9, small(K=2, stride=1, U=9, w_acc=0.0))]):
        c = random_case(case, B, N)
        st = c["states"]
        ok = np.ones(B, dtype=np.int32); ok[3] = 0
        agents, first = c["agents"]
        agents[1]["x"][0] = np.nan  # covers nothing
        st[2, 4, 3] = np.nan  # the curvature is not among the triggers of 'not planned'
        c["v0"][1] = 0.0
        got = stplan_ref.plan(params, st, c["v0"], agents, first, sp, n_states=c["n_states"], ok=ok, v_cap=c["v_cap"], set_of=c["set_of"], v_limit_in=c["v_limit_in"])
        for b in range(B):
            want = _scalar_plan(params, st[b], c["v0"][b], c["n_states"][b], ok[b], agents, first, c["set_of"][b], c["v_cap"][b], c["v_limit_in"][b], sp)
            for key in KEYS:
                assert same(got[key][b], np.array(want[key], dtype=got[key].dtype)), (case, b, key, got[key][b], want[key])
        seen |= set(got["status"].tolist())
    assert seen == {0, 1, 2, 3}


# The closed scenes: a straight path of 121 states 0.5 m apart and stride 2, so stations 1 m apart; dt = 1 s, so v(j, u) = u m/s exactly; a cap of 4 m/s on every
# state; a_max = 2, b_max = 3 (the defaults).  Every speed, acceleration and cost is a small integer: the expectations below are exact, there is no tolerance.
def closed(sets, oracle, v0=0.0, **kw):
    st = straight(121, 0.5)
    return ref(oracle, params_of(**dict(dict(stride=2), **kw)), states=st, v0=np.array([v0]), agents=sets, v_cap=np.full((1, 121), 4.0))


def crosser(T0):
    """A disc of 0.4 m that drives up the line x = 12 from y = -8 at T0 with 4 m/s (no hold flags: it exists for 4 s) and is on the path at T0 + 2."""
    return [[(0.4, 0, [(T0, 12.0, -8.0), (T0 + 4.0, 12.0, 8.0)])]]


def test_closed_scene_no_agents_accelerates_to_the_cap(oracle):
    r = closed([[]], oracle, w_acc=0.0)  # nothing but the distance to the cap counts: the fastest plan, 2 m/s then 4 m/s for seven steps
    assert r["status"][0] == 1 and r["ok_out"][0] == 1 and r["n_layers"][0] == 8 and r["cost"][0] == 4.0 and (r["cells"] == -1).all()
    assert r["station"][0].tolist() == [0, 2] + list(range(6, 31, 4)) + [-1] * 8
    want = np.full(121, -1.0); want[:4] = 2.0; want[4:60] = 4.0  # the edge speeds on the states each edge covers; beyond station 30 the plan says nothing
    assert same(r["v_limit"][0], want)
    r = closed([[]], oracle)  # the default weights: speeds never fall, reach the cap and stay there
    s, u = edges_of(r)
    assert r["status"][0] == 1 and (np.diff(u) >= 0).all() and u[-1] == 4 and u.max() == 4 and r["cost"][0] == 11.0  # 2, 3, 4: (4 + 4) + (1 + 1) + (1 + 0)
    for k in range(len(u)):
        assert (r["v_limit"][0, 2 * s[k]:2 * s[k + 1]] == u[k]).all()


def test_closed_scene_a_held_agent_is_stopped_for(oracle):
    """A disc that stays on the path 14 m ahead, and a horizon of 16 steps: 16 steps of at least 1 m/s would reach it, so the plan has to stop before it."""
    r = closed([[disc(14.0, 0.0, 0.4)]], oracle, K=16)
    first_blocked = int(np.flatnonzero(r["cells"][0, 0] >= 0)[0])
    assert 3 < first_blocked <= 14 and (r["cells"][0, :, first_blocked] == 0).all()
    s, u = edges_of(r)
    assert r["status"][0] == 2 and r["n_layers"][0] == 16 and u[-1] == 0 and s[-1] < first_blocked
    stop = 2 * s[-1]
    assert (r["v_limit"][0, stop:] == 0).all() and (r["v_limit"][0, :stop] > 0).all()  # 0 exactly from the stop station's state to n (= N here)
    assert not u[int(np.argmin(u)):].any()  # stopped stays stopped


def test_closed_scene_a_crosser_is_eased_off_behind(oracle):
    """The crosser is on the path during windows 3 and 4, where the fastest plan sweeps stations 10 .. 18: the plan eases off, never stops, and goes on behind it."""
    free, r = closed([[]], oracle), closed(crosser(2.0), oracle)
    s, u = edges_of(r)
    assert r["status"][0] == 2 and (u > 0).all() and r["n_layers"][0] == 8
    assert s[-1] < edges_of(free)[0][-1] and r["cost"][0] > free["cost"][0]
    blocked = np.flatnonzero(r["cells"][0, 3] >= 0)
    assert len(blocked) and same(r["cells"][0, 3], r["cells"][0, 4]) and (r["cells"][0, [0, 1, 2, 5, 6, 7]] == -1).all()
    assert s[5] < blocked.min() and s[-1] > blocked.max()  # short of the crossing until window 4 ends, across it afterwards
    for k in range(8):
        assert (r["cells"][0, k, s[k]:s[k + 1] + 1] == -1).all(), k


def test_closed_scene_an_agent_the_ego_clears_in_front_of(oracle):
    """The same crosser three seconds later blocks windows 6 and 7 at stations the plan has long passed: the plan is the one without agents."""
    free, r = closed([[]], oracle), closed(crosser(5.0), oracle)
    assert r["status"][0] == 2 and (r["cells"][0, 6:] >= 0).any() and (r["cells"][0, :6] == -1).all()
    for key in ("n_layers", "cost", "station", "v_limit", "ok_out"):
        assert same(r[key], free[key]), key
    assert edges_of(r)[0][6] > np.flatnonzero(r["cells"][0, 6] >= 0).max()


def test_closed_scene_a_blocked_first_cell_leaves_no_plan(oracle):
    r = closed([[disc(0.0, 0.0, 0.4)]], oracle)
    assert r["cells"][0, 0, 0] == 0 and r["status"][0] == 3 and r["ok_out"][0] == 0 and r["n_layers"][0] == 0 and r["cost"][0] == DBL_MAX
    assert (r["station"] == -1).all() and (r["v_limit"] == -1).all() and (r["cells"][0, :, :61] >= 0).any()


def check_plan(c, r, sp, b):
    """Every property the definition promises of a planned path, recomputed from the outputs alone."""
    n = int(np.clip(c["n_states"][b], 0, c["states"].shape[1]))
    stride, dt = int(sp.stride), np.float64(sp.dt)
    M = min((n - 1) // stride + 1, MAX_M)
    at = np.arange(M) * stride
    S = c["states"][b, at, 4]
    Vc = np.full(M, np.float64(sp.v_max))
    if c.get("v_cap") is not None:
        e = c["v_cap"][b, at]
        with np.errstate(all="ignore"):
            Vc = np.where(e >= 0, select_ref.vmin(Vc, e), Vc)
    s, u = edges_of(r, b)
    nl = len(u)
    cells = r["cells"][b]
    assert 1 <= nl <= sp.K and s[0] == 0 and (u >= 0).all() and (u <= sp.U).all() and (r["station"][b, nl + 1:] == -1).all() and (cells[:, M:] == -1).all()
    assert nl == sp.K or s[-1] == M - 1  # the arrival rule: a shorter plan ends at the last station
    assert (s[:-1] < M - 1).all()  # and an arrived state has no successor
    assert r["status"][b] == (2 if (cells >= 0).any() else 1) and r["ok_out"][b] == 1
    total, vp = np.float64(0.0), np.float64(c["v0"][b])
    for k in range(nl):
        j, uu = s[k + 1], u[k]
        v = (S[j] - S[j - uu]) / dt
        cc = Vc[j - uu]
        for m in range(j - uu + 1, j + 1):
            cc = select_ref.vmin(cc, Vc[m])
        acc = (v - vp) / dt
        assert uu == 0 or (v > 0 and v <= cc), (b, k)  # drivable
        assert (cells[k, j - uu:j + 1] == -1).all(), (b, k)  # clear
        assert acc <= sp.a_max and acc >= -sp.b_max, (b, k)
        assert k == 0 or u[k - 1] > 0 or uu == 0, (b, k)  # stopped stays stopped
        dv = cc - v
        total = total + ((np.float64(sp.w_acc) * acc) * acc + (np.float64(sp.w_slow) * dv) * dv)
        vp = v
    assert same(np.float64(r["cost"][b]), total)  # the edge costs re-summed in order
    return s, u


def test_properties_of_the_reference(oracle):
    seen = set()
    for seed, sp in ((1, small()), (2, small(K=4, stride=3, U=3, a_max=4.0, margin=0.9)), (3, small(stride=1, U=12, w_slow=0.25))):
        c = random_case(10 + seed, 30, 45, per_set=(7, 0, 12))
        r = ref(oracle, sp, **c)
        n = np.clip(c["n_states"], 0, 45)
        for b in range(30):
            st = r["status"][b]
            if st in (0, 3):
                assert r["ok_out"][b] == 0 and r["n_layers"][b] == 0 and r["cost"][b] == DBL_MAX and (r["station"][b] == -1).all()
                assert same(r["v_limit"][b], c["v_limit_in"][b])
                assert st == 3 or ((r["cells"][b] == -1).all() and (n[b] - 1) // sp.stride + 1 < 2)
                continue
            s, u = check_plan(c, r, sp, b)
            stop = sp.stride * s[-1]
            assert same(r["v_limit"][b, n[b]:], c["v_limit_in"][b, n[b]:])
            tail, lim = r["v_limit"][b, stop:n[b]], c["v_limit_in"][b, stop:n[b]]
            assert (tail == 0).all() if u[-1] == 0 else same(tail, lim)
            assert c["set_of"][b] != 1 or st == 1  # set 1 is empty
        seen |= set(r["status"].tolist())
    assert seen == {0, 1, 2, 3}


def ties_case():
    c = random_case(40, 6, 40, per_set=(6,), ragged=False)
    c["set_of"] = np.zeros(6, dtype=np.int32)
    return c, small(w_acc=0.0, w_slow=0.0, K=4)


def test_all_ties_follow_the_scan_order(oracle):
    """w_acc = w_slow = 0: every edge costs 0, every comparison is a tie, and a strict < keeps the first: among the candidates the first in (k, j, u) order — which
    is an arrived state at the smallest k if there is one, else the smallest reachable (j, u) of layer K — and among predecessors the smallest u'."""
    c, sp = ties_case()
    r = ref(oracle, sp, **c)
    assert set(r["status"].tolist()) <= {1, 2, 3} and (r["status"] != 3).sum() >= 3
    for b in np.flatnonzero(r["status"] != 3):
        want = _scalar_plan(oracle.default_params(), c["states"][b], c["v0"][b], 40, 1, *c["agents"], 0, c["v_cap"][b], c["v_limit_in"][b], sp)
        assert r["cost"][b] == 0 and same(r["station"][b], np.array(want["station"], dtype=np.int32))
        s, u = check_plan(c, r, sp, b)
        if len(u) == sp.K and c["v0"][b] / sp.dt <= sp.b_max and (r["cells"][b, :, 0] == -1).all():  # nothing arrived, station 0 is free and the vehicle can stop in one step: (0, 0) is the first state of layer K
            assert not s.any()


STATUS0_SP = dict(dt=1.0)


def status0_cases(N=12):
    """(tag, keyword change, whether the path is still planned) of every trigger of 'not planned', and inputs that must NOT trigger it."""
    def poke(key, val, row=5, col=None):
        def f(c):
            c[key] = c[key].copy()
            if col is None:
                c[key][1, row] = val
            else:
                c[key][1, row, col] = val
        return f

    def setk(key, val, dtype=np.int32):
        def f(c):
            c[key] = np.array(c[key], dtype=dtype); c[key][1] = val
        return f

    return [("ok", setk("ok", 0), 0), ("n=1", setk("n_states", 1), 0), ("n=0", setk("n_states", 0), 0), ("n<0", setk("n_states", -3), 0),
            ("M=1", setk("n_states", 2), 0),  # stride 2: one station
            ("x nan", poke("states", np.nan, col=0), 0), ("y inf", poke("states", np.inf, col=1), 0), ("z -inf", poke("states", -np.inf, col=2), 0),
            ("s nan", poke("states", np.nan, col=4), 0), ("s inf off a station", poke("states", np.inf, 3, 4), 0),
            ("v0 nan", setk("v0", np.nan, np.float64), 0), ("v0 inf", setk("v0", np.inf, np.float64), 0), ("v0 < 0", setk("v0", -0.5, np.float64), 0),
            ("k nan", poke("states", np.nan, col=3), 1), ("x nan beyond n", poke("states", np.nan, N - 1, 0), 1), ("n = 3", setk("n_states", 3), 1),
            ("v0 = 0", setk("v0", 0.0, np.float64), 1), ("n > N", setk("n_states", N + 40), 1), ("cap nan", poke("v_cap", np.nan), 1)]


def status0_inputs(N=12):
    st = make_paths(30, 3, N, ds=1.0, box=1.0)  # about 11 m, stations 2 m apart: with STATUS0_SP speeds come in steps of 2 m/s
    agents = [[disc(st[b, N - 1, 0], st[b, N - 1, 1], 0.3) for b in range(3)]]  # a held disc at the end of every path: the last stations are blocked
    return dict(states=st, v0=np.array([1.0, 1.5, 2.0]), n_states=np.array([N, N - 1, N], dtype=np.int32), ok=np.ones(3, dtype=np.int32), agents=agents,
                v_cap=np.full((3, N), 5.0), v_limit_in=np.full((3, N), 4.5))


def test_status_zero_triggers_of_the_reference(oracle):
    sp = small(**STATUS0_SP)
    clean = ref(oracle, sp, **status0_inputs())
    assert (clean["status"] == 2).all()
    for tag, change, still in status0_cases():
        c = status0_inputs()
        change(c)
        r = ref(oracle, sp, **c)
        assert (r["status"][1] > 0) == bool(still), tag
        if not still:
            assert r["ok_out"][1] == 0 and r["n_layers"][1] == 0 and r["cost"][1] == DBL_MAX and (r["station"][1] == -1).all() and (r["cells"][1] == -1).all(), tag
            assert (r["v_limit"][1] == 4.5).all(), tag
        for k in KEYS:  # the neighbours do not notice
            assert same(r[k][[0, 2]], clean[k][[0, 2]]), (tag, k)


def no_map(**kw):
    sp = binding.default_speed_params()
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


def closure_case():
    """Three straight paths of 121 states 0.5 m apart, offset sideways by 0, 0.25 and 9 m, against the crosser of the closed scenes, on the path at 2.5 s (the third path is never near it), a
    fourth with ok = 0; v0 = 2 m/s."""
    st = np.concatenate([straight(121, 0.5, y=y) for y in (0.0, 0.25, 9.0, 0.0)])
    return dict(states=st, v0=np.full(4, 2.0), ok=np.array([1, 1, 1, 0], dtype=np.int32)), crosser(0.5)


CLOSURE_SP = dict(stride=2, margin=1.5)
CLOSURE_DP = dict(margin=0.3, stop_distance=2.0)


def closure_on_the_references(oracle):
    params = oracle.default_params()
    c, agents = closure_case()
    sp, spd = params_of(**CLOSURE_SP), no_map()
    dp = binding.default_dynamic_params()
    dp.margin, dp.stop_distance = CLOSURE_DP["margin"], CLOSURE_DP["stop_distance"]
    ag, first = binding.pack_agents(agents)
    p0 = speed_ref.profile(params, c["states"], c["v0"], spd, ok=c["ok"])
    d0 = dynamic_ref.check(params, c["states"], p0["t"], ag, first, dp, ok=c["ok"])
    plan = stplan_ref.plan(params, c["states"], c["v0"], ag, first, sp, ok=c["ok"], v_cap=p0["v"])
    p1 = speed_ref.profile(params, c["states"], c["v0"], spd, ok=c["ok"], v_limit=plan["v_limit"])
    d1 = dynamic_ref.check(params, c["states"], p1["t"], ag, first, dp, ok=c["ok"])
    return p0, d0, plan, p1, d1


def test_closure_on_the_references(oracle):
    """stplan -> speed (v_limit) -> dynamic.  The definition does NOT guarantee that the profiled plan is free: po_speed_batch reaches a limit with its own
    accelerations and lags the plan, and the plan counts the vehicle only at stations.  The condition under which this scene closes, found on the numpy references:
    the planner's margin (1.5 m) lies above the check's (0.3 m) by more than the profile's lag moves the vehicle while the crosser is on the path."""
    p0, d0, plan, p1, d1 = closure_on_the_references(oracle)
    assert d0["status"].tolist() == [2, 2, 1, 0]  # without the plan the first two paths run into the crosser
    assert plan["status"].tolist() == [2, 2, 2, 0]
    assert d1["status"].tolist() == [1, 1, 1, 0]
    for b in (0, 1):
        s, u = edges_of(plan, b)
        assert (u > 0).all() and p1["total_time"][b] > p0["total_time"][b] and (p1["v"][b, :120] > 0).all()  # eased off, never stopped
        assert d1["gap_min"][b] >= CLOSURE_DP["margin"]


def test_new_symbols_and_abi_mirror():
    L = binding.lib()
    for name in NEW_ENTRIES:
        assert hasattr(L, name), name
        assert name in binding.EXPORTS
    fields = {"po_stplan_params": ["dt", "K", "stride", "U", "margin", "a_max", "b_max", "v_max", "w_acc", "w_slow"],
              "po_stplan_in": ["B", "N", "states", "n_states", "ok", "v0", "v_cap", "set_of", "agents", "v_limit_in"],
              "po_stplan_out": ["status", "ok_out", "n_layers", "cost", "station", "cells", "v_limit"]}
    mirror = {"po_stplan_params": abi.PoStplanParams, "po_stplan_in": abi.PoStplanIn, "po_stplan_out": abi.PoStplanOut}
    body = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs) for s, fs in fields.items())
    body += 'printf("%d %d %d %d", PO_ABI_VERSION, PO_ST_MAX_LAYERS, PO_ST_MAX_STEP, PO_ST_MAX_STATIONS);'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "po_hip.h"\nint main(){' + body + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    want = []
    for s, fs in fields.items():
        want.append(ctypes.sizeof(mirror[s]))
        want += [getattr(mirror[s], f).offset for f in fs]
    want += [abi.PO_ABI_VERSION, abi.PO_ST_MAX_LAYERS, abi.PO_ST_MAX_STEP, abi.PO_ST_MAX_STATIONS]
    assert got == want and abi.PO_ABI_VERSION == 7 and want[-3:] == [16, 31, 128]
    assert (stplan_ref.MAX_LAYERS, stplan_ref.MAX_STEP, stplan_ref.MAX_STATIONS) == (16, 31, 128)
    sp = binding.default_stplan_params()
    assert [getattr(sp, f) for f in fields["po_stplan_params"]] == [1.0, 8, 3, 20, 0.5, 2.0, 3.0, 15.0, 1.0, 1.0]


def bad_params():
    """Every parameter out of its range, one at a time."""
    out = []
    for f in ("dt", "a_max", "b_max", "v_max"):
        out += [(f, v) for v in (0.0, -1.0, np.nan, np.inf)]
    for f in ("w_acc", "w_slow"):
        out += [(f, v) for v in (-0.5, np.nan, np.inf)]
    out += [("margin", v) for v in (np.nan, np.inf, -np.inf)]
    out += [("K", 0), ("K", -1), ("K", 17), ("stride", 0), ("stride", -2), ("U", 0), ("U", 32), ("U", -1)]
    return out


def test_null_arguments_and_ranges_are_refused_without_a_device():
    """The argument checks come before the handle is touched, so any non-NULL handle value shows them here."""
    L = binding.lib()
    sp, si, so = binding.default_stplan_params(), abi.PoStplanIn(), abi.PoStplanOut()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))
    for entry in (L.po_stplan_batch, L.po_stplan_batch_device):
        assert entry(None, ctypes.byref(sp), ctypes.byref(si), ctypes.byref(so)) == abi.PO_ERR_INVALID
        assert entry(None, None, None, None) == abi.PO_ERR_INVALID
        assert entry(fake, None, ctypes.byref(si), ctypes.byref(so)) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(sp), None, ctypes.byref(so)) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(sp), ctypes.byref(si), None) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(sp), ctypes.byref(si), ctypes.byref(so)) == abi.PO_OK  # B = 0: nothing to do, and the handle is not looked at
        for f, v in bad_params():
            assert entry(fake, ctypes.byref(params_of(**{f: v})), ctypes.byref(si), ctypes.byref(so)) == abi.PO_ERR_INVALID, (f, v)
        for f, v in (("B", -1), ("N", -1)):
            bad = abi.PoStplanIn(); setattr(bad, f, v)
            assert entry(fake, ctypes.byref(sp), ctypes.byref(bad), ctypes.byref(so)) == abi.PO_ERR_INVALID, f
        one = abi.PoStplanIn(); one.B = 1; one.N = 4  # B > 0 and no states, v0, status or agents
        assert entry(fake, ctypes.byref(sp), ctypes.byref(one), ctypes.byref(so)) == abi.PO_ERR_INVALID
    L.po_default_stplan_params(None)  # a NULL struct is ignored


def test_host_mirror_header_compiles():
    inc = os.path.join(ROOT, "path_optimizer_amd", "host", "include")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "path_optimizer_amd/st_planner.hpp"\nint main() { PathOptimizationNS::StPlanner p; (void)p; return 0; }\n')
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-I", os.path.join(ROOT, "include"), src])


def test_host_mirror_stplan_test_compiles_and_links():
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "stplan_test"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(host, "stplan_test"))
    assert "StPlanner" in open(os.path.join(host, "test", "stplan_test.cpp")).read()


def mirror_case():
    """The seeded case of host/test/stplan_test.cpp, rebuilt with the same integer generator and the same dyadic arithmetic: bit for bit its inputs."""
    state = [24680]

    def u():
        state[0] = (state[0] * 1103515245 + 12345) & 0x7fffffff
        return (((state[0] >> 8) % 257) - 128) / 64.0

    B = 6
    n = np.array([3 + (b * 13) % 47 for b in range(B)], dtype=np.int32)
    N = int(n.max())
    states = np.zeros((B, N, 5))
    for b in range(B):
        for k in range(n[b]):
            x = -6.0 + 0.5 * k + u() / 16; y = u() / 2; z = u() / 8; kk = u() / 8
            states[b, k] = (x, y, z, kk, 0.5 * k)
    sets = []
    for s in range(3):
        agents = []
        for a in range(0 if s == 1 else 5):
            npts = 1 + (a * 3 + s) % 8
            t0, x0, y0 = u(), 6.0 + 4 * u(), u()
            agents.append((0.25 + 0.125 * a, (a + s) % 4, [(t0 + 0.75 * j, x0 + 0.5 * j, y0 + (j % 2) * 0.25) for j in range(npts)]))
        sets.append(agents)
    ok = np.ones(B, dtype=np.int32); ok[4] = 0
    cap, lim = np.full((B, N), -1.0), np.full((B, N), -1.0)
    for b in range(B):
        (cap if b % 2 else lim)[b, :n[b]] = 3.0 if b % 2 else 6.0
    c = dict(states=states, v0=1.0 + 0.5 * np.arange(B), n_states=n, ok=ok, set_of=np.array([b % 3 for b in range(B)], dtype=np.int32), agents=sets, v_cap=cap,
             v_limit_in=lim)
    return c, params_of(dt=0.5, K=6, stride=2, U=6)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0)  # no map: the stage reads none
    yield e
    e.close()


def _dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


OUT_TYPES = {"status": np.int32, "ok_out": np.int32, "n_layers": np.int32, "cost": np.float64, "station": np.int32, "cells": np.int32, "v_limit": np.float64}


def device_inputs(c):
    agents, first = binding.pack_agents(c["agents"])
    t = {"states": _dev(np.asarray(c["states"], dtype=np.float64)), "v0": _dev(np.asarray(c["v0"], dtype=np.float64)), "first": _dev(first),
         "agents": _dev(agents.view(np.uint8)) if len(agents) else None}
    for k in ("n_states", "ok", "set_of"):
        t[k] = None if c.get(k) is None else _dev(np.asarray(c[k], dtype=np.int32))
    for k in ("v_cap", "v_limit_in"):
        t[k] = None if c.get(k) is None else _dev(np.asarray(c[k], dtype=np.float64))
    return t


def device_outputs(B, N, K, want=KEYS):
    """Outputs that start as 7 / 77."""
    shape = {"station": (B, 17), "cells": (B, K, MAX_M), "v_limit": (B, N)}
    return {k: _dev(np.full(shape.get(k, (B,)), 77 if OUT_TYPES[k] == np.int32 else 7.0, dtype=OUT_TYPES[k])) for k in want}


def run_device(e, c, sp=None, want=KEYS):
    sp = sp or params_of()
    B, N = c["states"].shape[0], c["states"].shape[1]
    out = device_outputs(B, N, sp.K, want)
    e.stplan_batch_device(device_inputs(c), out, sp)
    return {k: _host(v) for k, v in out.items()}


def run_host(e, c, sp=None):
    """The host entry on outputs that start as 7 / 77 (Engine.stplan_batch allocates zeros: the sentinel goes through the C entry directly)."""
    sp = sp or params_of()
    c = dict(c)
    ag, first = binding.pack_agents(c.pop("agents"))
    states = np.ascontiguousarray(c["states"], dtype=np.float64)
    B, N = states.shape[0], states.shape[1]
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    f64 = lambda k: None if c.get(k) is None else np.ascontiguousarray(c[k], dtype=np.float64)
    i32 = lambda k: None if c.get(k) is None else np.ascontiguousarray(c[k], dtype=np.int32)
    arrs = dict(v0=f64("v0"), v_cap=f64("v_cap"), v_limit_in=f64("v_limit_in"), n_states=i32("n_states"), ok=i32("ok"), set_of=i32("set_of"))
    lists = abi.PoAgentLists(p(ag) if len(ag) else None, p(first), len(ag), len(first) - 1)
    si = abi.PoStplanIn(B, N, p(states), p(arrs["n_states"]), p(arrs["ok"]), p(arrs["v0"]), p(arrs["v_cap"]), p(arrs["set_of"]), ctypes.pointer(lists), p(arrs["v_limit_in"]))
    shape = {"station": (B, 17), "cells": (B, sp.K, MAX_M), "v_limit": (B, N)}
    r = {k: np.full(shape.get(k, (B,)), 77 if OUT_TYPES[k] == np.int32 else 7.0, dtype=OUT_TYPES[k]) for k in KEYS}
    binding._check(binding.lib().po_stplan_batch(e._h, ctypes.byref(sp), ctypes.byref(si), ctypes.byref(abi.PoStplanOut(*[p(r[k]) for k in KEYS]))))
    return r


def both(e, oracle, sp=None, tag="", **c):
    """Host entry, device entry and the reference: all three bitwise equal, outputs sentinel-filled, cells as well as the plan.  Returns the reference's dict."""
    want = ref(oracle, sp, **c)
    assert_same(run_host(e, c, sp), want, tag=tag + " host")
    assert_same(run_device(e, c, sp), want, tag=tag + " device")
    return want


@pytest.mark.gpu
def test_station_counts_strides_and_short_paths(eng, oracle):
    """M = 2, 3, 63, 64, 65, 128 and a path whose (n - 1) / stride + 1 exceeds 128 (clamped), n = 0, 1, 2, for stride 1, 2 and 3."""
    for stride in (1, 2, 3):
        lengths = [(M - 1) * stride + 1 + (M % stride if M > 3 else 0) for M in (2, 3, 63, 64, 65, 128)] + [130 * stride + 1, 0, 1, 2]
        N = max(lengths)
        c = random_case(60 + stride, len(lengths), N, per_set=(6, 3, 0))
        c["n_states"] = np.array(lengths, dtype=np.int32)
        sp = small(K=3, stride=stride, U=5, dt=0.5 * stride)
        r = both(eng, oracle, sp, tag=f"stride {stride}", **c)
        assert r["status"][7:9].tolist() == [0, 0] and (r["status"][9] > 0) == (stride == 1) and (r["status"][:7] > 0).all()
        assert ((r["cells"][6] >= 0).any(axis=0)[MAX_M - 8:]).any() or (r["status"][:7] >= 2).any()
    c = random_case(64, 3, 130, per_set=(8,), ragged=False, extras=False)  # N itself, no n_states, no set_of, no v_cap, no v_limit_in
    c.pop("n_states"); c.pop("set_of")
    r = both(eng, oracle, small(K=3, stride=1, U=5), tag="N", **c)
    assert (r["status"] > 0).all() and (np.isin(r["v_limit"], [-1.0]) | (r["v_limit"] >= 0)).all()


@pytest.mark.gpu
def test_layer_and_step_counts_at_their_limits(eng, oracle):
    """K = 1, 2, 16 and U = 1, 2, 31, with U far above M on the short paths."""
    c = random_case(65, 4, 40, per_set=(5, 4))
    c["n_states"] = np.array([40, 9, 5, 23], dtype=np.int32)  # M = 20, 5, 3, 12 at stride 2
    seen = set()
    for K, U in ((1, 1), (2, 2), (16, 31), (1, 31), (16, 1), (2, 31), (16, 2)):
        r = both(eng, oracle, small(K=K, U=U), tag=f"K {K} U {U}", **c)
        seen |= set(r["status"].tolist())
        assert (r["n_layers"] <= K).all()
    assert {1, 2} & seen and len(seen) >= 2


@pytest.mark.gpu
def test_every_limit_at_once(eng, oracle):
    """K = 16, U = 31 and 128 stations in one call: the largest LDS the launcher asks for (one workgroup per CU).  States about 0.3 m apart, dt = 0.25 s: speeds in
    steps of 1.2 m/s, so a_max = b_max = 6 lets a step change u by one."""
    c = random_case(68, 2, 140, per_set=(9, 5))
    c["n_states"] = np.array([140, 128], dtype=np.int32)
    sp = small(K=16, U=31, stride=1, dt=0.25, a_max=6.0, b_max=6.0)
    r = both(eng, oracle, sp, tag="limits", **c)
    assert (r["status"] == 2).all() and (r["n_layers"] == 16).all()


@pytest.mark.gpu
def test_agent_counts_around_the_chunk(eng, oracle):
    """Sets of 0, 1, chunk - 1, chunk, chunk + 1 and two chunks + 1 agents, twice: once as they come, and once with every agent but the last moved 100 m away and the
    last one a held disc on the path, so that the blocked cells carry the index of the LAST agent of the set — found in the second or third chunk."""
    counts = [0, 1, ST_CHUNK - 1, ST_CHUNK, ST_CHUNK + 1, 2 * ST_CHUNK + 1]
    S = len(counts)
    c = random_case(62, 2 * S, 40, per_set=counts + counts, ragged=False, extras=False)
    c["set_of"] = np.arange(2 * S, dtype=np.int32)
    agents, first = c["agents"]
    for k in range(S + 1, 2 * S):
        agents["x"][first[k]:first[k + 1] - 1] += 100.0
        last = agents[first[k + 1] - 1]
        last["n_pts"], last["flags"], last["radius"], last["t"][0] = 1, BEFORE | AFTER, 0.3, 0.0
        last["x"][0], last["y"][0] = c["states"][k, 30, 0], c["states"][k, 30, 1]
    r = both(eng, oracle, small(margin=0.1), tag="counts", **c)
    assert (r["cells"][[0, S]] == -1).all() and (r["status"] == 1).any() and (r["status"] >= 2).any()
    for k in range(S + 1, 2 * S):
        hit = r["cells"][k][r["cells"][k] >= 0]
        assert len(hit) and (hit == first[k + 1] - 1).all(), k
    assert first[2 * S] - 1 - first[2 * S - 1] == 2 * ST_CHUNK


@pytest.mark.gpu
def test_batch_sizes_and_position_in_the_batch(eng, oracle):
    for B in (1, 2, 65):
        c = random_case(70 + B, B, 40)
        ok = np.ones(B, dtype=np.int32); ok[B // 3] = 0
        both(eng, oracle, small(), ok=ok, tag=f"B {B}", **c)
    c = random_case(80, 70, 50, per_set=(9, 4, 0))
    c["n_states"][41] = 50; c["set_of"][41] = 0
    big = eng.stplan_batch(params=small(), **c)
    one = eng.stplan_batch(params=small(), **{k: (v if k == "agents" else v[41:42]) for k, v in c.items()})
    assert big["status"][41] > 0
    for k in KEYS:
        assert same(big[k][41:42], one[k]), k


@pytest.mark.gpu
def test_sets(eng, oracle):
    c = random_case(90, 12, 40, per_set=(6, 0, 11))
    c["set_of"] = np.array([0, 1, 2, 2, 1, 0, 0, 2, 1, 1, 2, 0], dtype=np.int32)
    c["n_states"] = np.maximum(c["n_states"], 10)
    r = both(eng, oracle, small(margin=0.6), tag="sets", **c)
    assert (r["status"][c["set_of"] == 1] == 1).all() and (r["cells"][c["set_of"] == 1] == -1).all()
    first = c["agents"][1]
    lo, hi = first[c["set_of"]][:, None, None], first[c["set_of"] + 1][:, None, None]
    assert (r["cells"] >= 0).any() and ((r["cells"] == -1) | ((r["cells"] >= lo) & (r["cells"] < hi))).all()
    c.pop("set_of")  # NULL: every path meets set 0
    r0 = both(eng, oracle, small(margin=0.6), tag="no set_of", **c)
    assert (r0["cells"] < first[1]).all()


def piece_case():
    """dt = 0.25 and agents whose point times are multiples of 0.25, so piece boundaries fall exactly on the window times k * dt; 1 .. 8 points and every flag
    combination, one agent per set so that cells shows every agent on its own, and four paths beside each other."""
    B, N = 4, 41
    st = np.concatenate([straight(N, 0.25, y=y) for y in (0.0, 0.25, -0.5, 6.0)])
    st[:, :, 0] -= 2.0
    sets = []
    for npts in range(1, 9):
        for flags in range(4):
            T0 = 0.25 * ((npts * 5 + flags * 3) % 11)
            pts = [(T0 + 0.5 * j, 1.0 + 0.5 * npts + 0.75 * j, (1.0 - 0.25 * flags) * (-1) ** j) for j in range(npts)]
            sets.append([(0.125 + 0.0625 * flags, flags, pts)])
    return st, sets


@pytest.mark.gpu
def test_agent_pieces_with_boundaries_on_the_window_times(eng, oracle):
    st, sets = piece_case()
    S = len(sets)
    states = np.tile(st, (S, 1, 1))
    c = dict(states=states, v0=np.full(4 * S, 1.0), agents=sets, set_of=np.repeat(np.arange(S, dtype=np.int32), 4))
    sp = params_of(dt=0.25, K=16, stride=2, U=4, margin=0.3, a_max=4.0, b_max=4.0)  # stations 0.5 m apart: speeds in steps of 2 m/s, accelerations of 8 m/s^2; v0 = 1 reaches 0 and 2 m/s
    r = both(eng, oracle, sp, tag="pieces", **c)
    hit = (r["cells"] >= 0).any(axis=(1, 2)).reshape(S, 4)
    assert hit[:, :3].any(axis=1).sum() >= S - 4 and not hit[:, 3].any()  # almost every agent blocks a cell of a path near it; the path 6 m away is never blocked
    windows = (r["cells"].reshape(S, 4, 16, MAX_M) >= 0).any(axis=(1, 3))
    one_point_no_hold = windows[0]
    assert not one_point_no_hold.any()  # one point and no flag: the agent covers no time at all
    assert windows[1, :9].all() and not windows[1, 9:].any() and windows[2].all()  # one point held before T0 = 2.0: windows 0 .. 8 (window 8 touches T0); held after T0 = 0: all
    assert {1, 2, 3} >= set(r["status"].tolist()) and (r["status"] == 2).any()


@pytest.mark.gpu
def test_margin_one_ulp_either_side_of_a_gap(eng, oracle):
    st = straight(21, 0.5)
    sets = [[disc(30.0, 9.0, 0.1), disc(6.0, 2.5, 0.5), disc(6.0, 2.5, 0.5)]]
    c = dict(states=st, v0=np.array([1.0]), agents=sets)
    sp = params_of(stride=2, K=3)
    ag, first = binding.pack_agents(sets)
    _, gaps = stplan_ref.blocked_cells(oracle.default_params(), st[0, ::2], ag, 0, 3, sp, want_gap=True)
    g = gaps.min()
    at = np.argwhere(gaps == g)
    assert 0 < g < 2 and len(at) >= 3  # the nearest station, in every window
    for margin, hit in ((np.nextafter(g, -np.inf), False), (g, False), (np.nextafter(g, np.inf), True)):
        r = both(eng, oracle, params_of(stride=2, K=3, margin=margin), tag=f"margin {margin!r}", **c)
        assert (r["status"][0] == 2) == hit and (r["cells"][0] >= 0).sum() == (len(at) if hit else 0)
        if hit:
            assert all(r["cells"][0, k, m] == 1 for k, m in at)  # of two agents with the same gap the smaller index
    swapped = dict(c, agents=[[disc(6.0, 2.5, 0.5), disc(30.0, 9.0, 0.1), disc(6.0, 2.5, 0.5)]])
    assert both(eng, oracle, params_of(stride=2, K=3, margin=1.5 * g), tag="swapped", **swapped)["cells"].max() == 0


@pytest.mark.gpu
def test_all_ties_and_a_speed_no_braking_absorbs(eng, oracle):
    c, sp = ties_case()
    r = both(eng, oracle, sp, tag="ties", **c)
    assert (r["cost"][r["status"] != 3] == 0).all() and (r["status"] != 3).sum() >= 3
    # v0 = 14 m/s, stations 0.6 m apart, at most 6 stations a step of 0.5 s: the fastest first edge is about 7.2 m/s, a deceleration of 13 m/s^2 against b_max = 3
    fast = dict(c, v0=np.full(6, 14.0))
    r = both(eng, oracle, small(), tag="too fast", **fast)
    assert (r["status"] == 3).all() and (r["station"] == -1).all() and same(r["v_limit"], c["v_limit_in"])


@pytest.mark.gpu
def test_status_zero_triggers(eng, oracle):
    for tag, change, still in status0_cases():
        c = status0_inputs()
        change(c)
        r = both(eng, oracle, small(**STATUS0_SP), tag=tag, **c)
        assert (r["status"][1] > 0) == bool(still), tag


@pytest.mark.gpu
def test_optional_arguments_and_empty_calls(eng, oracle):
    c = random_case(100, 70, 30)
    ok = np.ones(70, dtype=np.int32); ok[::9] = 0
    c["ok"] = ok
    sp = small()
    want = ref(oracle, sp, **c)
    for drop in KEYS[1:]:  # every optional output NULL in turn
        keys = tuple(k for k in KEYS if k != drop)
        assert_same(run_device(eng, c, sp, want=keys), want, keys=keys, tag="without " + drop)
    assert_same(run_device(eng, c, sp, want=("status",)), want, keys=("status",), tag="status alone")
    for drop in ("n_states", "ok", "v_cap", "set_of", "v_limit_in"):  # every optional input NULL in turn
        both(eng, oracle, sp, tag="no " + drop, **{k: v for k, v in c.items() if k != drop})
    r = eng.stplan_batch(want_rows=False, params=sp, **c)
    assert r["cells"] is None and r["v_limit"] is None
    assert_same(r, want, keys=KEYS[:5], tag="host, no rows")
    # B = 0: PO_OK from both entries on this handle, which has no map; nothing is looked at, not even the agents
    L = binding.lib()
    for entry in (L.po_stplan_batch, L.po_stplan_batch_device):
        si = abi.PoStplanIn(); si.N = 5
        assert entry(eng._h, ctypes.byref(sp), ctypes.byref(si), ctypes.byref(abi.PoStplanOut())) == abi.PO_OK
    none = dict(c, agents=[[], []], set_of=np.zeros(70, dtype=np.int32))  # no agents at all: no cell is blocked
    r = both(eng, oracle, sp, tag="no agents", **none)
    assert set(r["status"].tolist()) <= {0, 1, 3} and (r["cells"] == -1).all()


@pytest.mark.gpu
def test_device_lists_are_read_clamped(eng, oracle):
    """What the host entry refuses, the device entry reads as the definition says: set_of and first clamped, an agent with a bad n_pts covers nothing."""
    c = random_case(105, 6, 30, per_set=(5, 5), ragged=False)
    agents, first = c["agents"]
    agents = agents.copy(); agents["n_pts"][2] = 9; agents["n_pts"][7] = -1
    c["agents"] = (agents, np.array([-3, 5, 99], dtype=np.int32))
    c["set_of"] = np.array([0, 1, -2, 7, 1, 0], dtype=np.int32)
    sp = small(margin=0.8)
    want = ref(oracle, sp, **c)
    assert_same(run_device(eng, c, sp), want, tag="clamped")
    assert (want["cells"] >= 0).any() and not np.isin(want["cells"], [2, 7]).any()
    with pytest.raises(binding.PoError):
        eng.stplan_batch(params=sp, **c)


@pytest.mark.gpu
def test_chain_stplan_speed_dynamic_on_one_stream(oracle):
    """speed -> stplan (v_cap = that profile's v) -> speed (v_limit) -> dynamic, device entries only, no synchronisation and no host copy between the four calls;
    equal to the CPU chain of test_closure_on_the_references, which ends free."""
    import torch

    c, agents = closure_case()
    B, N = c["states"].shape[0], c["states"].shape[1]
    sp, spd = params_of(**CLOSURE_SP), no_map()
    dp = binding.default_dynamic_params()
    dp.margin, dp.stop_distance = CLOSURE_DP["margin"], CLOSURE_DP["stop_distance"]
    e = binding.Engine(0)
    f64 = lambda: _dev(np.full((B, N), 7.0))
    speed = [{"v": f64(), "a": f64(), "t": f64(), "total_time": _dev(np.full(B, 7.0)), "status": _dev(np.full(B, 77, dtype=np.int32))} for _ in range(2)]
    plan = device_outputs(B, N, sp.K)
    dkeys = {"status": np.int32, "ok_out": np.int32, "gap_min": np.float64, "first_state": np.int32, "first_agent": np.int32, "stop_state": np.int32,
             "first_time": np.float64, "gap": np.float64, "v_limit": np.float64}
    dyn = {k: _dev(np.full((B, N) if k in ("gap", "v_limit") else (B,), 77 if t == np.int32 else 7.0, dtype=t)) for k, t in dkeys.items()}
    p_in = device_inputs(dict(states=c["states"], v0=c["v0"], ok=c["ok"], agents=agents))
    s_in = {"states": p_in["states"], "ok": p_in["ok"], "v0": p_in["v0"]}
    torch.cuda.synchronize()
    e.speed_batch_device(s_in, speed[0], spd)
    e.stplan_batch_device(dict(p_in, v_cap=speed[0]["v"]), plan, sp)
    e.speed_batch_device(dict(s_in, v_limit=plan["v_limit"]), speed[1], spd)
    e.dynamic_batch_device(dict(p_in, t=speed[1]["t"]), dyn, dp)
    got_s = [{k: _host(v) for k, v in o.items()} for o in speed]
    got_p, got_d = {k: _host(v) for k, v in plan.items()}, {k: _host(v) for k, v in dyn.items()}
    e.close()
    p0, _, want_p, p1, d1 = closure_on_the_references(oracle)
    skeys = ("v", "a", "t", "total_time", "status")
    assert_same(got_s[0], p0, keys=skeys, tag="speed 1"); assert_same(got_p, want_p, tag="stplan")
    assert_same(got_s[1], p1, keys=skeys, tag="speed 2"); assert_same(got_d, d1, keys=tuple(dkeys), tag="dynamic")
    assert got_p["status"].tolist() == [2, 2, 2, 0] and got_d["status"].tolist() == [1, 1, 1, 0]


@pytest.mark.gpu
def test_host_mirror_stplan_program(eng, oracle):
    """StPlanner::plan end to end in its own process: its statuses, layer counts and its checksum of v_limit and station equal the Python call's and the reference's."""
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "stplan_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "stplan_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "stplan_test passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]
    printed = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("status", "layers", "checksum")}
    c, sp = mirror_case()
    got = both(eng, oracle, sp, tag="mirror case", **c)
    assert printed["status"] == got["status"].tolist() and printed["layers"] == got["n_layers"].tolist() and got["status"][4] == 0
    assert {1, 2} <= set(got["status"].tolist())
    total = 0
    for b in range(len(c["n_states"])):
        total += int(got["v_limit"][b, :c["n_states"][b]].view(np.uint64).sum(dtype=np.uint64))
        total += int(got["station"][b, :got["n_layers"][b] + 1].sum()) if got["status"][b] in (1, 2) else 0
    assert printed["checksum"] == [total & 0xffffffffffffffff]


@pytest.mark.gpu
def test_host_validation(eng):
    st = make_paths(120, 4, 8, box=1.0)
    v0 = np.full(4, 1.0)
    good = [[disc(0.0, 0.0, 0.3), (0.2, 3, [(0.0, 1.0, 1.0), (1.0, 2.0, 1.0), (2.5, 2.0, 3.0)])], []]
    sp = small()
    assert (eng.stplan_batch(st, v0, good, params=sp)["status"] > 0).all()
    for f, v in bad_params():
        with pytest.raises(binding.PoError):
            eng.stplan_batch(st, v0, good, params=small(**{f: v}))
    assert (eng.stplan_batch(st, v0, good, params=small(margin=-10.0, w_acc=0.0, w_slow=0.0, K=16, U=31, stride=1))["status"] == 1).all()  # inside the ranges

    def bad_agent(field, val, idx=None):
        ag, first = binding.pack_agents(good)
        if idx is None:
            ag[1][field] = val
        else:
            ag[1][field][idx] = val
        return ag, first

    lists = [bad_agent("n_pts", 0), bad_agent("n_pts", 9), bad_agent("radius", -0.1), bad_agent("radius", np.nan), bad_agent("radius", np.inf),
             bad_agent("t", np.nan, 1), bad_agent("t", 0.0, 1), bad_agent("t", 0.5, 2), bad_agent("t", np.inf, 2), bad_agent("x", np.nan, 0), bad_agent("y", -np.inf, 2),
             bad_agent("flags", 4), bad_agent("flags", -1)]
    ag, first = binding.pack_agents(good)
    lists += [(ag, np.array(f, dtype=np.int32)) for f in ([1, 2, 2], [0, 2, 1], [0, 2, 3], [0, -1, 2])]
    for k, bad in enumerate(lists):
        with pytest.raises(binding.PoError):
            eng.stplan_batch(st, v0, bad, params=sp)
            raise AssertionError(f"list {k} was accepted")
    assert (eng.stplan_batch(st, v0, bad_agent("x", np.nan, 5), params=sp)["status"] > 0).all()  # beyond n_pts: not read
    for so in ([0, 1, 2, 0], [0, -1, 0, 0]):
        with pytest.raises(binding.PoError):
            eng.stplan_batch(st, v0, good, set_of=np.array(so, dtype=np.int32), params=sp)
    L = binding.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    status = np.zeros(4, dtype=np.int32)

    def call(entry, lists_args, in_edit=None, out_status=True, no_lists=False):
        lists_ = abi.PoAgentLists(*lists_args)
        args = [4, 8, p(st), None, None, p(v0), None, None, None if no_lists else ctypes.pointer(lists_), None]
        for k, v in (in_edit or {}).items():
            args[k] = v
        so = abi.PoStplanOut(p(status) if out_status else None, *([None] * 6))
        return entry(eng._h, ctypes.byref(sp), ctypes.byref(abi.PoStplanIn(*args)), ctypes.byref(so))

    full = [p(ag), p(first), len(ag), 2]
    assert call(L.po_stplan_batch, full) == abi.PO_OK
    for entry in (L.po_stplan_batch, L.po_stplan_batch_device):
        for edit in ({2: None}, {5: None}, {0: -1}, {1: -1}):  # states, v0, B, N
            assert call(entry, full, edit) == abi.PO_ERR_INVALID, edit
        assert call(entry, full, out_status=False) == abi.PO_ERR_INVALID
        assert call(entry, full, no_lists=True) == abi.PO_ERR_INVALID
        for bad in ([None, p(first), len(ag), 2], [p(ag), None, len(ag), 2], [p(ag), p(first), -1, 2], [p(ag), p(first), len(ag), -1], [p(ag), p(first), len(ag), 0]):
            assert call(entry, bad) == abi.PO_ERR_INVALID
    assert call(L.po_stplan_batch, [None, p(np.zeros(3, dtype=np.int32)), 0, 2]) == abi.PO_OK and (status == 1).all()  # n_agents = 0 needs no agents pointer
