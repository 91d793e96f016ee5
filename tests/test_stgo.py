"""Station-time plans that resume, sampled in time: po_stgo_batch* (csrc/po_stgo.hip, csrc/po_stsearch.hpp; include/po_hip.h states the definition; DESIGN.md
section 39).

Every cell, cost, station and sample is a fixed sequence of rounded IEEE double operations and integer choices, so every comparison with the device here is BIT
equality on byte views against tests/stgo_ref.py (numpy, one ufunc per operation), with sentinel-filled outputs, through both entries.  There is no tolerance in this
file: the closed scenes are test_stplan.py's grid (stations 1 m apart, dt = 1 s, a cap of 4 m/s), where every speed, acceleration and cost is a small integer.  The
path generators, agents and status-0 cases are test_stplan.py's own (imported, not copied): the two stages share their inputs.

CPU: the reference's search and sampler against a scalar loop over the definition (with resumes among the cases), the two closed scenes where the plan stops, waits
and goes while po_stplan_batch stands still or stops for good, the scenes where both stages agree, exact sample values, properties on random inputs, every status-0
trigger, the closures stgo -> dynamic and stgo -> trajectory -> dynamic on the references, exports and the ABI mirror, argument, range and aliasing checks without a
device, the host mirror compiles and links.  GPU: station counts, strides, layer and step counts at their limits, sample counts around one and two waves, agent
counts around the LDS chunk, batch sizes and position in the batch, both closed scenes, status-0 triggers, NULL optional inputs and outputs, empty calls, lists read
clamped, three chains on one stream, the C++ mirror's program."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dynamic_ref
import select_ref
import speed_ref
import stgo_ref
import stplan_ref
import test_stplan as ts
import trajectory_ref
from path_optimizer_amd import abi, binding

ROOT = ts.ROOT
NEW_ENTRIES = ["po_default_stgo_params", "po_stgo_batch", "po_stgo_batch_device"]
KEYS = ("status", "ok_out", "n_layers", "cost", "station", "cells", "n_resumes", "states", "v", "a", "t", "index", "first_held", "end")
PLAN_KEYS = ("n_layers", "cost", "station")
DBL_MAX = select_ref.DBL_MAX
BEFORE = abi.PO_AGENT_HOLD_BEFORE
MAX_M = abi.PO_ST_MAX_STATIONS
same = ts.same


def assert_same(got, want, keys=KEYS, tag=""):
    ts.assert_same(got, want, keys=keys, tag=tag)


def params_of(**kw):
    gp = binding.default_stgo_params()
    for k, v in kw.items():
        setattr(gp, k, v)
    return gp


def small(**kw):
    """test_stplan.py's knobs for the random cases, sampled four times a window from just before time 0 to just behind the horizon.  Stations are about 0.6 m apart,
    so the slowest moving edge has about 1.2 m/s and pulling away from rest takes about 2.4 m/s^2: a_max = 4 (the default 2 would leave nothing to resume)."""
    return params_of(**dict(dict(dt=0.5, K=5, stride=2, U=6, margin=0.4, a_max=4.0, t0=-0.25, dts=0.125, Q=27), **kw))


def stplan_params(gp):
    sp = binding.default_stplan_params()
    for f, _ in sp._fields_:
        setattr(sp, f, getattr(gp, f))
    return sp


def leaving(rng, st, n, t_leave):
    """A disc held ON a path (at a state in its third quarter and at least 15 states, about 4.5 m, ahead: the vehicle's own station stays free) until t_leave, then gone within 0.25 s:
    what a plan has to wait for."""
    i = int(rng.integers(max(15, n // 2), max(16, (3 * n) // 4)))
    x, y = st[i, 0], st[i, 1]
    return (0.3, BEFORE, [(t_leave, x, y), (t_leave + 0.25, x + 40.0, y + 40.0)])


def random_case(seed, B, N, per_set=(5, 0, 9), ragged=True, extras=True, waits=True):
    """test_stplan.py's random case without v_limit_in and with speeds of 0 .. 2 m/s; with `waits` every third path gets a set of its own that holds a disc on it for a while."""
    c = ts.random_case(seed, B, N, per_set=per_set, ragged=ragged, extras=extras)
    c.pop("v_limit_in", None)
    c["n_states"] = np.maximum(c["n_states"], 6)  # (the paths too short to plan have cases of their own)
    for f in ("x", "y"):  # the agents spread over twice the box: fewer of them stand where a path starts, which no plan survives
        c["agents"][0][f] *= 2.0
    rng = np.random.default_rng([39, seed])
    c["v0"] = rng.uniform(0, 2, B)  # with caps of 2 m/s and more and b_max = 3, a first edge exists: most paths are planned
    if waits:
        agents, first = c["agents"]
        sets = [list(range(first[k], first[k + 1])) for k in range(len(first) - 1)]
        recs = [agents[i] for i in range(len(agents))]
        for b in range(0, B, 3):
            n = int(np.clip(c["n_states"][b], 0, N))
            if n < 24:
                continue
            one = binding.pack_agents([[leaving(rng, c["states"][b], n, float(rng.uniform(0.6, 1.6)))]])[0][0]
            sets.append([len(recs)]); recs.append(one)
            c["set_of"][b] = len(sets) - 1
            c["v0"][b] = float(rng.uniform(0, 1.0))
        order = [i for s in sets for i in s]
        c["agents"] = (np.array([recs[i] for i in order], dtype=agents.dtype), np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32))
    return c


def ref(oracle, gp=None, **c):
    c = dict(c)
    agents, first = binding.pack_agents(c.pop("agents"))
    return stgo_ref.plan(oracle.default_params(), c.pop("states"), c.pop("v0"), agents, first, gp or params_of(), **c)


def ref_stplan(oracle, gp, **c):
    c = dict(c)
    agents, first = binding.pack_agents(c.pop("agents"))
    return stplan_ref.plan(oracle.default_params(), c.pop("states"), c.pop("v0"), agents, first, stplan_params(gp), **c)


def planned_share(r):
    return np.isin(r["status"], (1, 2)).mean()


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def _scalar_stgo(st, cells, v0, cap, gp):
    """Search, choice, n_resumes and samples of the definition as a plain scalar Python loop over ONE planned path (Python floats are IEEE doubles; every operation
    rounds once).  st [n, 5]; cells [K][M] are the blocked cells (stplan_ref.blocked_cells, which test_stplan.py checks against its own scalar loop: the definition
    of the cells is po_stplan_batch's, unchanged)."""
    n, K, U, stride, Q = len(st), int(gp.K), int(gp.U), int(gp.stride), int(gp.Q)
    dt, a_max, b_max, v_max, w_acc, w_slow, t0, dts = (float(getattr(gp, f)) for f in ("dt", "a_max", "b_max", "v_max", "w_acc", "w_slow", "t0", "dts"))
    mn = lambda a, b: b if b < a else a
    x, y, z, kap, s = ([float(v) for v in st[:, c]] for c in range(5))
    v0 = float(v0)
    M = min((n - 1) // stride + 1, MAX_M)
    S = [s[m * stride] for m in range(M)]
    Vc = [mn(v_max, float(cap[m * stride])) if cap is not None and float(cap[m * stride]) >= 0 else v_max for m in range(M)]
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
                for up in ([0] if k == 1 else range(min(U, p) + 1)):  # a predecessor at rest may have any successor
                    if k == 1:
                        if p != 0:
                            continue
                        cp, vp = 0.0, v0
                    else:
                        cp, vp = prev[(p, up)], v(p, up)
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
    if best[1] == 0:
        return None
    cost, nl, j, u = best
    station, us = [0] * (nl + 1), [0] * (nl + 1)
    for k in range(nl, 0, -1):
        station[k], us[k] = j, u
        j, u = j - u, bp[(k, j, u)]
    out = dict(n_layers=nl, cost=cost, station=station + [-1] * (16 - nl), n_resumes=sum(1 for k in range(2, nl + 1) if us[k - 1] == 0 and us[k] > 0))
    V = [v0] + [v(station[k], us[k]) for k in range(1, nl + 1)]
    A = [0.0] + [(V[k] - V[k - 1]) / dt for k in range(1, nl + 1)]
    rows, vs, accs, ts_, idx, first_held = [], [], [], [], [], Q
    for q in range(Q):
        T = t0 + float(q) * dts
        if T < 0:
            row, vv, aa = 0, v0, 0.0
        else:
            kk = max(k for k in range(nl + 1) if float(k) * dt <= T)
            if kk == nl:
                row, vv, aa = station[nl] * stride, V[nl], 0.0
                first_held = min(first_held, q)
            else:
                p, j = station[kk], station[kk + 1]
                tau = T - float(kk) * dt
                if j == p:
                    row, vv, aa = p * stride, 0.0, A[kk + 1]
                else:
                    sig = V[kk + 1] * tau
                    sx = S[p] + sig
                    sx = S[j] if sx > S[j] else sx
                    i = max(i for i in range(p * stride, j * stride) if s[i] <= sx)
                    ds = s[i + 1] - s[i]
                    lam = (sx - s[i]) / ds if ds > 0 else 0.0
                    lam = 0.0 if lam < 0 else lam
                    lam = 1.0 if lam > 1 else lam
                    dz = z[i + 1] - z[i]
                    if dz > 3.141592653589793:
                        dz = dz - 6.283185307179586
                    elif dz < -3.141592653589793:
                        dz = dz + 6.283185307179586
                    rows.append([x[i] + lam * (x[i + 1] - x[i]), y[i] + lam * (y[i + 1] - y[i]), z[i] + lam * dz, kap[i] + lam * (kap[i + 1] - kap[i]), s[i] + lam * ds])
                    vs.append(V[kk + 1]); accs.append(A[kk + 1]); ts_.append(T); idx.append(i)
                    continue
        rows.append([x[row], y[row], z[row], kap[row], s[row]])
        vs.append(vv); accs.append(aa); ts_.append(T); idx.append(row)
    end = 1 if first_held == Q else (2 if station[nl] == M - 1 else (3 if us[nl] == 0 else 4))
    out.update(states=rows, v=vs, a=accs, t=ts_, index=idx, first_held=first_held, end=end)
    return out


def test_reference_agrees_with_a_scalar_loop_over_the_definition(oracle):
    params = oracle.default_params()
    resumes, ends, planned = 0, set(), 0
    for case, (B, N, gp) in enumerate([(12, 31, small()), (9, 30, small(K=4, stride=3, U=2, margin=0.8, t0=0.0, dts=0.5, Q=6)),
                                       (6, 13, small(K=3, stride=1, U=9, w_acc=0.0, dts=0.375, Q=9))]):
        c = random_case(case, B, N)
        c["states"][2, 4, 3] = np.nan  # the curvature is not among the triggers of 'not planned'; it goes through the samples as it is
        agents, first = c["agents"]
        got = stgo_ref.plan(params, c["states"], c["v0"], agents, first, gp, n_states=c["n_states"], v_cap=c["v_cap"], set_of=c["set_of"])
        for b in np.flatnonzero(got["status"] > 0):
            n = int(np.clip(c["n_states"][b], 0, N))
            M = min((n - 1) // gp.stride + 1, MAX_M)
            want = _scalar_stgo(c["states"][b, :n], got["cells"][b, :, :M].tolist(), c["v0"][b], c["v_cap"][b], gp)
            assert (want is None) == (got["status"][b] == 3), (case, b)
            if want is None:
                continue
            planned += 1
            for key in ("n_layers", "cost", "station", "n_resumes", "states", "v", "a", "t", "index", "first_held", "end"):
                assert same(got[key][b], np.array(want[key], dtype=got[key].dtype)), (case, b, key, got[key][b], want[key])
        resumes = max(resumes, int(got["n_resumes"].max()))
        ends |= set(got["end"].tolist())
    assert resumes >= 1 and planned >= 15 and ends >= {0, 2, 3, 4}  # not vacuous: a resume, and samples of every kind of ending a 3.1 s window leaves


# The closed scenes are test_stplan.py's grid: a straight path of 121 states 0.5 m apart and stride 2, so stations 1 m apart; dt = 1 s, so v(j, u) = u m/s exactly;
# a cap of 4 m/s on every state; a_max = 2, b_max = 3 (the defaults).  Every speed, acceleration and cost is a small integer: the expectations are exact.
def closed_case(sets, v0=0.0):
    return dict(states=ts.straight(121, 0.5), v0=np.array([v0]), agents=sets, v_cap=np.full((1, 121), 4.0))


def closed(sets, oracle, v0=0.0, **kw):
    return ref(oracle, params_of(**dict(dict(stride=2), **kw)), **closed_case(sets, v0))


def closed_stplan(sets, oracle, v0=0.0, **kw):
    return ref_stplan(oracle, params_of(**dict(dict(stride=2), **kw)), **closed_case(sets, v0))


def held_until(T, x):
    """A disc of 0.4 m held on the path at x until T (PO_AGENT_HOLD_BEFORE only), which then leaves sideways within half a second."""
    return [[(0.4, BEFORE, [(T, x, 0.0), (T + 0.5, x, 30.0)])]]


SCENE1 = dict(sets=held_until(5.0, 6.0), v0=0.0, K=12)
SCENE2 = dict(sets=held_until(9.0, 9.0), v0=2.0, K=16)
SCENE1_STATION = [0, 0, 0, 0, 0, 0, 0, 2, 5, 9, 13, 17, 21]
SCENE2_STATION = [0, 1, 2, 2, 2, 2, 2, 2, 2, 2, 3, 6, 10, 14, 18, 22, 26]


def test_closed_scene_1_waits_at_the_start_and_goes(oracle):
    """The contrast that shows the feature exists: po_stplan_batch stands at station 0 for the whole horizon (cost 192), this stage waits six windows and drives."""
    r = closed(oracle=oracle, **SCENE1)
    assert r["status"][0] == 2 and r["cost"][0] == 107.0 and r["n_layers"][0] == 12 and r["n_resumes"][0] == 1
    assert r["station"][0].tolist() == SCENE1_STATION + [-1] * 4
    old = closed_stplan(oracle=oracle, **SCENE1)
    assert old["status"][0] == 2 and old["cost"][0] == 192.0 and old["station"][0, :13].tolist() == [0] * 13
    assert same(old["cells"], r["cells"])  # the geometry half is the same text


def test_closed_scene_2_drives_stops_waits_and_goes(oracle):
    r = closed(oracle=oracle, **SCENE2)
    assert r["status"][0] == 2 and r["cost"][0] == 148.0 and r["n_layers"][0] == 16 and r["n_resumes"][0] == 1
    assert r["station"][0].tolist() == SCENE2_STATION
    assert np.count_nonzero(np.diff(SCENE2_STATION) == 0) == 7  # seven windows of waiting
    old = closed_stplan(oracle=oracle, **SCENE2)
    assert old["status"][0] == 2 and old["cost"][0] == 237.0 and old["station"][0].tolist() == [0, 1, 2] + [3] * 14


def test_closed_scenes_where_nothing_has_to_wait_equal_stplan(oracle):
    """No agents, the crosser at 2 s (eased off behind) and at 5 s (cleared in front of): removing the rule changes nothing."""
    for sets in ([[]], ts.crosser(2.0), ts.crosser(5.0)):
        r, old = closed(sets, oracle), closed_stplan(sets, oracle)
        assert r["status"][0] == old["status"][0] and r["n_resumes"][0] == 0
        for key in PLAN_KEYS + ("cells", "ok_out"):
            assert same(r[key], old[key]), key


def test_samples_exact_values(oracle):
    st = ts.straight(121, 0.5)[0]
    r = closed(oracle=oracle, t0=0.0, dts=0.25, Q=53, **SCENE1)
    assert (r["index"][0, :24] == 0).all() and (r["v"][0, :24] == 0).all() and same(r["states"][0, :24], np.tile(st[0], (24, 1)))  # waiting at state 0
    assert (r["a"][0, :20] == 0).all() and (r["a"][0, 20:24] == 0).all()  # (the window before the pull-away is a standing one: A_6 = 0; A_7 = 2 is window 6's)
    assert r["v"][0, 24] == 2.0 and r["a"][0, 24] == 2.0 and r["index"][0, 24] == 0 and same(r["states"][0, 24], st[0])  # T = 6 belongs to window 6, which moves
    assert (np.diff(r["states"][0, :, 4]) >= 0).all()
    assert same(r["t"][0], 0.25 * np.arange(53))
    for k in range(13):  # on a layer time the sample is the station's row exactly
        assert same(r["states"][0, 4 * k], st[2 * SCENE1_STATION[k]]), k
        assert r["v"][0, 4 * k] == (np.diff(SCENE1_STATION)[k] if k < 12 else 4.0)  # ... with the LATER window's speed, and the last edge's when held
    assert r["states"][0, 25, 4] == 0.5 and r["index"][0, 25] == 1 and r["states"][0, 26, 4] == 1.0 and r["states"][0, 29, 4] == 2.75 and r["index"][0, 29] == 5
    assert r["first_held"][0] == 48 and r["end"][0] == 4 and same(r["states"][0, 48:], np.tile(st[42], (5, 1))) and (r["v"][0, 48:] == 4).all() and (r["a"][0, 48:] == 0).all()
    inside = closed(oracle=oracle, t0=0.0, dts=0.25, Q=48, **SCENE1)
    assert inside["first_held"][0] == 48 and inside["end"][0] == 1 and same(inside["states"][0], r["states"][0, :48])
    # a negative t0: the samples before time 0 are state 0 with v0, then the same plan
    neg = closed(oracle=oracle, t0=-0.75, dts=0.25, Q=56, **SCENE2)
    assert (neg["index"][0, :3] == 0).all() and (neg["v"][0, :3] == 2.0).all() and (neg["a"][0, :3] == 0).all() and same(neg["t"][0, :4], np.array([-0.75, -0.5, -0.25, 0.0]))
    assert neg["v"][0, 3] == 1.0 and neg["a"][0, 3] == -1.0 and neg["states"][0, 4, 4] == 0.25
    wait = neg["states"][0, 3 + 8:3 + 36 + 1]
    assert same(wait, np.tile(st[4], (29, 1))) and (neg["v"][0, 3 + 8:3 + 36] == 0).all()  # from T = 2 to T = 9 at station 2
    assert neg["a"][0, 3 + 4] == 0.0 and neg["a"][0, 3 + 8] == -1.0 and neg["a"][0, 3 + 12] == 0.0 and neg["a"][0, 3 + 36] == 1.0  # the window that stops carries the acc its edge was costed with: 1 m/s -> 0
    # arrived: a path of 11 stations is driven to its end; rest: a disc that never leaves is stood before
    short = ref(oracle, params_of(stride=2, t0=0.0, dts=0.5, Q=20), states=ts.straight(21, 0.5), v0=np.array([0.0]), agents=[[]], v_cap=np.full((1, 21), 4.0))
    nl = int(short["n_layers"][0])
    assert short["status"][0] == 1 and nl < 8 and short["station"][0, nl] == 10 and short["first_held"][0] == 2 * nl and short["end"][0] == 2
    rest = closed([[ts.disc(5.5, 0.0, 0.4)]], oracle, K=12, t0=0.0, dts=1.0, Q=16)  # a disc that never leaves and blocks station 1: nothing to do but stand at station 0
    assert rest["first_held"][0] == 12 and rest["end"][0] == 3 and (rest["v"][0] == 0).all() and rest["n_resumes"][0] == 0 and not rest["station"][0, :13].any()
    none = closed([[ts.disc(0.0, 0.0, 0.4)]], oracle, Q=9)  # a blocked first cell: no plan, the samples of a path that is not planned, cells the map
    assert none["status"][0] == 3 and (none["states"] == 0).all() and (none["t"] == 0).all() and (none["index"] == -1).all() and none["first_held"][0] == -1
    assert none["end"][0] == 0 and none["n_resumes"][0] == 0 and (none["cells"][0, :, :61] >= 0).any() and (none["station"] == -1).all()


def check_plan(c, r, gp, b):
    """Every property the definition promises of a planned path, recomputed from the outputs alone."""
    N = c["states"].shape[1]
    n = int(np.clip(c["n_states"][b], 0, N))
    stride, dt = int(gp.stride), np.float64(gp.dt)
    M = min((n - 1) // stride + 1, MAX_M)
    at = np.arange(M) * stride
    S = c["states"][b, at, 4]
    Vc = np.full(M, np.float64(gp.v_max))
    if c.get("v_cap") is not None:
        e = c["v_cap"][b, at]
        with np.errstate(all="ignore"):
            Vc = np.where(e >= 0, select_ref.vmin(Vc, e), Vc)
    s, u = ts.edges_of(r, b)
    nl = len(u)
    cells = r["cells"][b]
    assert 1 <= nl <= gp.K and s[0] == 0 and (u >= 0).all() and (u <= gp.U).all() and (r["station"][b, nl + 1:] == -1).all() and (cells[:, M:] == -1).all()
    assert (nl == gp.K or s[-1] == M - 1) and (s[:-1] < M - 1).all()
    assert r["status"][b] == (2 if (cells >= 0).any() else 1) and r["ok_out"][b] == 1
    assert r["n_resumes"][b] == sum(1 for k in range(1, nl) if u[k - 1] == 0 and u[k] > 0)
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
        assert acc <= gp.a_max and acc >= -gp.b_max, (b, k)
        dv = cc - v
        total = total + ((np.float64(gp.w_acc) * acc) * acc + (np.float64(gp.w_slow) * dv) * dv)
        vp = v
    assert same(np.float64(r["cost"][b]), total)  # the edge costs re-summed in order
    lam, kk, idx = r["lam"][b], r["kk"][b], r["index"][b]
    moving = ~np.isnan(lam)
    assert ((lam[moving] >= 0) & (lam[moving] <= 1)).all()
    for q in np.flatnonzero(moving):
        assert u[kk[q]] > 0 and s[kk[q]] * stride <= idx[q] < s[kk[q] + 1] * stride, (b, q)  # inside its edge's state range
    assert (np.diff(r["states"][b, :, 4]) >= 0).all() and (idx >= 0).all() and (idx < n).all()
    assert same(r["t"][b], stgo_ref.times(gp))
    fh = int(r["first_held"][b])
    assert ((kk == nl) == (np.arange(gp.Q) >= fh)).all() and r["end"][b] == (1 if fh == gp.Q else (2 if s[-1] == M - 1 else (3 if u[-1] == 0 else 4)))
    return s, u


def test_properties_of_the_reference(oracle):
    seen, resumes = set(), 0
    for seed, gp in ((1, small()), (2, small(K=4, stride=3, U=3, a_max=4.0, margin=0.9, dts=0.3, Q=9)), (3, small(stride=1, U=12, w_slow=0.25, t0=0.0, dts=0.5, Q=5))):
        c = random_case(10 + seed, 30, 45, per_set=(7, 0, 12))
        c["ok"] = np.ones(30, dtype=np.int32); c["ok"][7] = 0
        r = ref(oracle, gp, **c)
        for b in range(30):
            st = r["status"][b]
            if st in (0, 3):
                assert r["ok_out"][b] == 0 and r["n_layers"][b] == 0 and r["cost"][b] == DBL_MAX and (r["station"][b] == -1).all() and r["n_resumes"][b] == 0
                assert not r["states"][b].any() and not r["v"][b].any() and not r["a"][b].any() and not r["t"][b].any()
                assert (r["index"][b] == -1).all() and r["first_held"][b] == -1 and r["end"][b] == 0
                assert st == 3 or (r["cells"][b] == -1).all()
                continue
            check_plan(c, r, gp, b)
        seen |= set(r["status"].tolist())
        resumes += int((r["n_resumes"] > 0).sum())
    assert seen == {0, 1, 2, 3} and resumes >= 3


def status0_inputs(N=12):
    c = ts.status0_inputs(N)
    c.pop("v_limit_in")
    return c


def status0_cases(N=12):
    """test_stplan.py's triggers, and the one this stage adds: s going back, by one ulp; equal s is no trigger."""
    def s_of(val):
        def f(c):
            c["states"] = c["states"].copy()
            c["states"][1, 5, 4] = val(c["states"][1, 4, 4])
        return f

    return ts.status0_cases(N) + [("s one ulp back", s_of(lambda s: np.nextafter(s, -np.inf)), 0), ("s equal", s_of(lambda s: s), 1),
                                  ("s back off a station", lambda c: c["states"].__setitem__((1, 3, 4), c["states"][1, 2, 4] - 0.5), 0)]


def test_status_zero_triggers_of_the_reference(oracle):
    gp = small(**ts.STATUS0_SP)
    clean = ref(oracle, gp, **status0_inputs())
    assert (clean["status"] == 2).all()
    for tag, change, still in status0_cases():
        c = status0_inputs()
        c["states"] = c["states"].copy()
        change(c)
        r = ref(oracle, gp, **c)
        assert (r["status"][1] > 0) == bool(still), tag
        if not still:
            assert r["ok_out"][1] == 0 and r["n_layers"][1] == 0 and r["cost"][1] == DBL_MAX and (r["station"][1] == -1).all() and (r["cells"][1] == -1).all(), tag
            assert not r["states"][1].any() and (r["index"][1] == -1).all() and r["first_held"][1] == -1 and r["end"][1] == 0 and r["n_resumes"][1] == 0, tag
        for k in KEYS:  # the neighbours do not notice
            assert same(r[k][[0, 2]], clean[k][[0, 2]]), (tag, k)
    old = ref_stplan(oracle, gp, **dict(status0_inputs(), states=(lambda s: (s.__setitem__((1, 5, 4), np.nextafter(s[1, 4, 4], -np.inf)), s)[1])(status0_inputs()["states"].copy())))
    assert old["status"][1] > 0  # the stated difference: po_stplan_batch plans a path whose s goes back


CLOSURE = dict(margin=1.5, t0=0.0, dts=0.25, Q=65)  # dts <= dt: see test_closure_stgo_trajectory_dynamic_on_the_references
CLOSURE_DP = dict(margin=0.3, stop_distance=2.0)


def dyn_params():
    dp = binding.default_dynamic_params()
    dp.margin, dp.stop_distance = CLOSURE_DP["margin"], CLOSURE_DP["stop_distance"]
    return dp


def closure_plan(oracle):
    c = closed_case(SCENE2["sets"], SCENE2["v0"])
    gp = params_of(stride=2, K=SCENE2["K"], **CLOSURE)
    return c, gp, ref(oracle, gp, **c)


def test_closure_stgo_dynamic_on_the_references(oracle):
    """stgo -> dynamic on the samples (states, t).  The definition does NOT guarantee that the sampled plan is free: the plan counts the vehicle only at stations and
    for whole windows, the check follows it between samples, continuously.  The condition under which scene 2 closes, found on the numpy references: the planner's
    margin (1.5 m) lies above the check's (0.3 m) by more than the ground between two stations (1 m), which is all the plan does not cover."""
    c, gp, r = closure_plan(oracle)
    assert r["status"][0] == 2 and r["n_resumes"][0] == 1
    ag, first = binding.pack_agents(c["agents"])
    d = dynamic_ref.check(oracle.default_params(), r["states"], r["t"], ag, first, dyn_params())
    assert d["status"][0] == 1 and d["gap_min"][0] >= CLOSURE_DP["margin"]
    standing = (r["v"][0] == 0) & (np.arange(gp.Q) < r["first_held"][0])
    assert standing.sum() >= 16  # and the check covered a vehicle that waits: intervals of positive duration and zero displacement


def trajectory_of(gp, D=4, discs=None):
    tp = binding.default_trajectory_params()
    tp.t0, tp.dt, tp.K, tp.n_discs, tp.agent_pts, tp.agent_stride, tp.agent_flags = gp.t0, gp.dts, gp.Q, D, 8, (gp.Q - 1) // 7, 0
    off, rad = discs
    for d in range(D):
        tp.disc_offset[d], tp.disc_radius[d] = off[d], rad
    return tp


def second_vehicle(r, gp):
    """A vehicle that drives across the first one's path through the place where it waits, there in the middle of the wait."""
    wait = np.flatnonzero((r["v"][0] == 0) & (np.arange(gp.Q) < r["first_held"][0]))
    q = int(wait[len(wait) // 2])
    x, T = r["states"][0, q, 0], r["t"][0, q]
    n = 41
    st = np.zeros((1, n, 5))
    st[0, :, 0], st[0, :, 1], st[0, :, 2], st[0, :, 4] = x, -10.0 + 0.5 * np.arange(n), np.pi / 2, 0.5 * np.arange(n)
    t = (T - 4.0) + 0.2 * np.arange(n)[None, :]  # 2.5 m/s; at y = 0 at time T
    return st, t, (r["t"][0, wait[0]], r["t"][0, wait[-1]])


def test_closure_stgo_trajectory_dynamic_on_the_references(oracle):
    """stgo -> trajectory (t0 the same, dt = dts, K = Q, D = 4) -> dynamic for a second vehicle.  The trajectory stage reproduces the sample positions (compared by
    == on values, not bytes: x + 0 * dx turns -0 into +0), and its records make the waiting vehicle an agent.  The chain needs dts <= dt: with samples further apart
    than a window, two standing samples (v == 0) can have ground between them, which is po_trajectory_batch's end-state rule, and the trajectory would freeze there."""
    c, gp, r = closure_plan(oracle)
    params = oracle.default_params()
    tp = trajectory_of(gp, discs=binding.covering_discs(params))
    tr = trajectory_ref.trajectory(r["states"], r["v"], r["t"], tp)
    assert tr["status"][0] in (1, 2, 3) and (tr["states"] == r["states"]).all() and (tr["t"] == r["t"]).all()
    agents, first = tr["agents"], np.array([0, 4], dtype=np.int32)
    st2, t2, (w0, w1) = second_vehicle(r, gp)
    d = dynamic_ref.check(params, st2, t2, agents, first, dyn_params())
    assert d["status"][0] == 2 and w0 <= d["first_time"][0] <= w1 and w1 - w0 >= 6.0  # a conflict it can stop for, while the first vehicle waits
    late = dynamic_ref.check(params, st2, t2 + 12.0, agents, first, dyn_params())
    assert late["status"][0] == 1  # the records carry no hold flags: after the horizon the first vehicle is gone


FIELDS = {"po_stgo_params": ["dt", "K", "stride", "U", "margin", "a_max", "b_max", "v_max", "w_acc", "w_slow", "t0", "dts", "Q"],
          "po_stgo_in": ["B", "N", "states", "n_states", "ok", "v0", "v_cap", "set_of", "agents"],
          "po_stgo_out": ["status", "ok_out", "n_layers", "cost", "station", "cells", "n_resumes", "states", "v", "a", "t", "index", "first_held", "end"]}


def test_new_symbols_and_abi_mirror():
    L = binding.lib()
    for name in NEW_ENTRIES:
        assert hasattr(L, name), name
        assert name in binding.EXPORTS
    mirror = {"po_stgo_params": abi.PoStgoParams, "po_stgo_in": abi.PoStgoIn, "po_stgo_out": abi.PoStgoOut}
    body = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs) for s, fs in FIELDS.items())
    body += 'printf("%d", PO_ABI_VERSION);'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "po_hip.h"\nint main(){' + body + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    want = []
    for s, fs in FIELDS.items():
        want.append(ctypes.sizeof(mirror[s]))
        want += [getattr(mirror[s], f).offset for f in fs]
        assert [f for f, _ in mirror[s]._fields_] == fs
    assert got == want + [7] and abi.PO_ABI_VERSION == 7
    assert tuple(binding.Engine.STGO_KEYS) == KEYS
    gp, sp = binding.default_stgo_params(), binding.default_stplan_params()
    assert [getattr(gp, f) for f in FIELDS["po_stgo_params"]] == [getattr(sp, f) for f, _ in sp._fields_] + [0.0, 0.1, 81]
    assert gp.t0 + (gp.Q - 1) * gp.dts >= gp.K * gp.dt - 1e-9  # the samples span the horizon


def bad_params():
    return ts.bad_params() + [("t0", v) for v in (np.nan, np.inf, -np.inf)] + [("dts", v) for v in (0.0, -0.1, np.nan, np.inf)] + [("Q", 0), ("Q", -3)]


def test_null_arguments_ranges_and_aliasing_are_refused_without_a_device():
    """The argument checks come before the handle is touched, so any non-NULL handle value shows them here."""
    L = binding.lib()
    gp, gi, go = binding.default_stgo_params(), abi.PoStgoIn(), abi.PoStgoOut()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    B, N, Q = 2, 6, 5
    st, v0, cap = np.zeros((B, N, 5)), np.zeros(B), np.zeros((B, N))
    ints = {k: np.zeros(B, dtype=np.int32) for k in ("n_states", "ok", "set_of")}
    ag, first = binding.pack_agents([[ts.disc(0.0, 0.0, 0.3)]])
    lists = abi.PoAgentLists(p(ag), p(first), 1, 1)
    small_gp = params_of(Q=Q, K=2)
    for entry in (L.po_stgo_batch, L.po_stgo_batch_device):
        assert entry(None, ctypes.byref(gp), ctypes.byref(gi), ctypes.byref(go)) == abi.PO_ERR_INVALID
        assert entry(None, None, None, None) == abi.PO_ERR_INVALID
        assert entry(fake, None, ctypes.byref(gi), ctypes.byref(go)) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(gp), None, ctypes.byref(go)) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(gp), ctypes.byref(gi), None) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(gp), ctypes.byref(gi), ctypes.byref(go)) == abi.PO_OK  # B = 0: nothing to do, and the handle is not looked at
        for f, v in bad_params():
            assert entry(fake, ctypes.byref(params_of(**{f: v})), ctypes.byref(gi), ctypes.byref(go)) == abi.PO_ERR_INVALID, (f, v)
        for f, v in (("B", -1), ("N", -1)):
            bad = abi.PoStgoIn(); setattr(bad, f, v)
            assert entry(fake, ctypes.byref(gp), ctypes.byref(bad), ctypes.byref(go)) == abi.PO_ERR_INVALID, f
        # B > 0: each required pointer NULL in turn is refused before the handle is looked at; and each output aliasing an input
        full_in = lambda: abi.PoStgoIn(B, N, p(st), p(ints["n_states"]), p(ints["ok"]), p(v0), p(cap), p(ints["set_of"]), ctypes.pointer(lists))
        status, states = np.zeros(B, dtype=np.int32), np.zeros((B, Q, 5))
        for drop in ("states", "v0", "agents"):
            gin = full_in(); setattr(gin, drop, None)
            assert entry(fake, ctypes.byref(small_gp), ctypes.byref(gin), ctypes.byref(abi.PoStgoOut(status=p(status), states=p(states)))) == abi.PO_ERR_INVALID, drop
        for out in (abi.PoStgoOut(states=p(states)), abi.PoStgoOut(status=p(status))):
            assert entry(fake, ctypes.byref(small_gp), ctypes.byref(full_in()), ctypes.byref(out)) == abi.PO_ERR_INVALID
        ins = {"states": st, "n_states": ints["n_states"], "ok": ints["ok"], "v0": v0, "v_cap": cap, "set_of": ints["set_of"]}
        for okey in FIELDS["po_stgo_out"]:
            for ikey, arr in ins.items():
                out = abi.PoStgoOut(status=p(status), states=p(states))
                setattr(out, okey, ctypes.c_void_p(p(arr).value + arr.nbytes - 4))  # the last bytes of the input: inside its full extent
                assert entry(fake, ctypes.byref(small_gp), ctypes.byref(full_in()), ctypes.byref(out)) == abi.PO_ERR_INVALID, (okey, ikey)
    L.po_default_stgo_params(None)  # a NULL struct is ignored


def test_host_mirror_header_compiles():
    inc = os.path.join(ROOT, "path_optimizer_amd", "host", "include")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "path_optimizer_amd/st_go.hpp"\nint main() { PathOptimizationNS::StGoPlanner p; (void)p; return 0; }\n')
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-I", os.path.join(ROOT, "include"), src])


def test_host_mirror_stgo_test_compiles_and_links():
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "stgo_test"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(host, "stgo_test"))
    assert "StGoPlanner" in open(os.path.join(host, "test", "stgo_test.cpp")).read()


def mirror_case():
    """test_stplan.py's seeded case (host/test/stgo_test.cpp builds the same one with the same integer generator) without v_limit_in, sampled 13 times."""
    c, sp = ts.mirror_case()
    c.pop("v_limit_in")
    gp = params_of(t0=-0.25, dts=0.25, Q=13)
    for f, _ in sp._fields_:
        setattr(gp, f, getattr(sp, f))
    return c, gp


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0)  # no map: the stage reads none
    yield e
    e.close()


_dev, _host = ts._dev, ts._host
# The seeds of the random GPU cases, picked on the CPU (tests/stgo_ref.py) so that the reference plans at least 80 % of the paths each case asks that of
SEEDS = {"stations": (1, 1, 1), "N": 5, "layers": 1, "limits": 3, "samples": 3, "counts": 18, "B": {1: 1, 2: 3, 65: 3}, "position": 2, "optional": 3, "clamped": 3}
OUT_TYPES = {k: (np.float64 if k in ("cost", "states", "v", "a", "t") else np.int32) for k in KEYS}


def out_shapes(B, K, Q):
    return {"station": (B, 17), "cells": (B, K, MAX_M), "states": (B, Q, 5), "v": (B, Q), "a": (B, Q), "t": (B, Q), "index": (B, Q)}


def sentinels(B, K, Q, want=KEYS):
    """Outputs that start as 7 / 77."""
    shape = out_shapes(B, K, Q)
    return {k: np.full(shape.get(k, (B,)), 77 if OUT_TYPES[k] == np.int32 else 7.0, dtype=OUT_TYPES[k]) for k in want}


def device_inputs(c):
    t = ts.device_inputs(dict(c, v_limit_in=None))
    t.pop("v_limit_in")
    return t


def run_device(e, c, gp, want=KEYS):
    B = c["states"].shape[0]
    out = {k: _dev(v) for k, v in sentinels(B, gp.K, gp.Q, want).items()}
    e.stgo_batch_device(device_inputs(c), out, gp)
    return {k: _host(v) for k, v in out.items()}


def run_host(e, c, gp):
    """The host entry on outputs that start as 7 / 77 (Engine.stgo_batch allocates zeros: the sentinel goes through the C entry directly)."""
    c = dict(c)
    ag, first = binding.pack_agents(c.pop("agents"))
    states = np.ascontiguousarray(c["states"], dtype=np.float64)
    B, N = states.shape[0], states.shape[1]
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    f64 = lambda k: None if c.get(k) is None else np.ascontiguousarray(c[k], dtype=np.float64)
    i32 = lambda k: None if c.get(k) is None else np.ascontiguousarray(c[k], dtype=np.int32)
    arrs = dict(v0=f64("v0"), v_cap=f64("v_cap"), n_states=i32("n_states"), ok=i32("ok"), set_of=i32("set_of"))
    lists = abi.PoAgentLists(p(ag) if len(ag) else None, p(first), len(ag), len(first) - 1)
    gi = abi.PoStgoIn(B, N, p(states), p(arrs["n_states"]), p(arrs["ok"]), p(arrs["v0"]), p(arrs["v_cap"]), p(arrs["set_of"]), ctypes.pointer(lists))
    r = sentinels(B, gp.K, gp.Q)
    binding._check(binding.lib().po_stgo_batch(e._h, ctypes.byref(gp), ctypes.byref(gi), ctypes.byref(abi.PoStgoOut(*[p(r[k]) for k in KEYS]))))
    return r


def both(e, oracle, gp, tag="", share=None, **c):
    """Host entry, device entry and the reference: all three bitwise equal, outputs sentinel-filled.  share: the least share of planned paths (the random cases ask
    for 0.8, with seeds picked on the CPU).  Returns the reference's dict."""
    want = ref(oracle, gp, **c)
    if share is not None:
        assert planned_share(want) >= share, (tag, planned_share(want))
    assert_same(run_host(e, c, gp), want, tag=tag + " host")
    assert_same(run_device(e, c, gp), want, tag=tag + " device")
    return want


@pytest.mark.gpu
def test_station_counts_strides_and_short_paths(eng, oracle):
    """M = 2, 3, 63, 64, 65, 128 and a path whose (n - 1) / stride + 1 exceeds 128 (clamped), n = 0, 1, 2, for stride 1, 2 and 3.  The three shortest are what the
    definition does not plan: the share is asked of the others."""
    for stride in (1, 2, 3):
        lengths = [(M - 1) * stride + 1 + (M % stride if M > 3 else 0) for M in (2, 3, 63, 64, 65, 128)] + [130 * stride + 1, 0, 1, 2]
        N = max(lengths)
        c = random_case(SEEDS["stations"][stride - 1], len(lengths), N, per_set=(6, 3, 0))
        c["n_states"] = np.array(lengths, dtype=np.int32)
        gp = small(K=3, stride=stride, U=5, dt=0.5 * stride, dts=0.25 * stride, Q=9)
        r = both(eng, oracle, gp, tag=f"stride {stride}", **c)
        assert r["status"][7:9].tolist() == [0, 0] and (r["status"][9] > 0) == (stride == 1)
        assert np.isin(r["status"][:7], (1, 2)).mean() >= 0.8
    c = random_case(SEEDS["N"], 3, 130, per_set=(8,), ragged=False, extras=False, waits=False)  # N itself, no n_states, no set_of, no v_cap
    c.pop("n_states"); c.pop("set_of")
    both(eng, oracle, small(K=3, stride=1, U=5), tag="N", share=0.8, **c)


@pytest.mark.gpu
def test_layer_and_step_counts_at_their_limits(eng, oracle):
    """K = 1, 2, 16 and U = 1, 2, 31, with U far above M on the short paths."""
    c = random_case(SEEDS["layers"], 4, 40, per_set=(5, 4))
    c["n_states"] = np.array([40, 9, 5, 23], dtype=np.int32)  # M = 20, 5, 3, 12 at stride 2
    for K, U in ((1, 1), (2, 2), (16, 31), (1, 31), (16, 1), (2, 31), (16, 2)):
        r = both(eng, oracle, small(K=K, U=U, Q=4 * K + 3), tag=f"K {K} U {U}", share=0.8, **c)
        assert (r["n_layers"] <= K).all()


@pytest.mark.gpu
def test_every_limit_at_once(eng, oracle):
    """K = 16, U = 31, 128 stations and Q = 129 in one call: the largest LDS the launcher asks for (one workgroup per CU)."""
    c = random_case(SEEDS["limits"], 2, 140, per_set=(9, 5), waits=False)
    c["n_states"] = np.array([140, 128], dtype=np.int32)
    gp = small(K=16, U=31, stride=1, dt=0.25, a_max=6.0, b_max=6.0, t0=0.0, dts=0.03125, Q=129)
    r = both(eng, oracle, gp, tag="limits", share=0.8, **c)
    assert (r["n_layers"] == 16).all()


@pytest.mark.gpu
def test_sample_counts_around_one_and_two_waves(eng, oracle):
    c = random_case(SEEDS["samples"], 5, 40, per_set=(5, 4))
    c["n_states"] = np.maximum(c["n_states"], 12)
    ends = set()
    for Q in (1, 2, 63, 64, 65, 129):
        r = both(eng, oracle, small(Q=Q, dts=3.0 / max(Q - 1, 1)), tag=f"Q {Q}", share=0.8, **c)
        ends |= set(r["end"].tolist())
    assert len(ends) >= 2


@pytest.mark.gpu
def test_agent_counts_around_the_chunk(eng, oracle):
    counts = [0, 1, ts.ST_CHUNK - 1, ts.ST_CHUNK, ts.ST_CHUNK + 1, 2 * ts.ST_CHUNK + 1]
    c = random_case(SEEDS["counts"], len(counts), 40, per_set=counts, ragged=False, extras=False, waits=False)
    c["set_of"] = np.arange(len(counts), dtype=np.int32)
    agents, first = c["agents"]
    for k in range(len(counts)):  # all but the last two agents of every set 100 m away: the ones that matter come in the set's last chunk
        agents["x"][first[k]:max(first[k + 1] - 2, first[k])] += 100.0
    r = both(eng, oracle, small(margin=0.1), tag="counts", share=0.8, **c)
    assert (r["cells"][0] == -1).all() and (r["status"] >= 2).sum() >= 2
    hit = r["cells"][5][r["cells"][5] >= 0]
    assert len(hit) and (hit >= first[6] - 2).all()  # found in the third chunk


@pytest.mark.gpu
def test_batch_sizes_and_position_in_the_batch(eng, oracle):
    for B in (1, 2, 65):
        c = random_case(SEEDS["B"][B], B, 40, ragged=B > 2)
        both(eng, oracle, small(), tag=f"B {B}", share=0.8, **c)
    c = random_case(SEEDS["position"], 70, 50, per_set=(9, 4, 0))
    c["n_states"][41] = 50
    assert planned_share(ref(oracle, small(), **c)) >= 0.8
    big = eng.stgo_batch(params=small(), **c)
    one = eng.stgo_batch(params=small(), **{k: (v if k == "agents" else v[41:42]) for k, v in c.items()})
    assert big["status"][41] > 0 and planned_share(big) >= 0.8
    for k in KEYS:
        assert same(big[k][41:42], one[k]), k


@pytest.mark.gpu
def test_closed_scenes(eng, oracle):
    for scene, station, cost in ((SCENE1, SCENE1_STATION, 107.0), (SCENE2, SCENE2_STATION, 148.0)):
        gp = params_of(stride=2, K=scene["K"], t0=0.0, dts=0.25, Q=4 * scene["K"] + 5)
        r = both(eng, oracle, gp, tag="scene", **closed_case(scene["sets"], scene["v0"]))
        assert r["station"][0, :scene["K"] + 1].tolist() == station and r["cost"][0] == cost and r["n_resumes"][0] == 1 and r["end"][0] == 4


@pytest.mark.gpu
def test_status_zero_triggers(eng, oracle):
    for tag, change, still in status0_cases():
        c = status0_inputs()
        c["states"] = c["states"].copy()
        change(c)
        r = both(eng, oracle, small(**ts.STATUS0_SP), tag=tag, **c)
        assert (r["status"][1] > 0) == bool(still), tag


@pytest.mark.gpu
def test_optional_arguments_and_empty_calls(eng, oracle):
    c = random_case(SEEDS["optional"], 70, 30)
    ok = np.ones(70, dtype=np.int32); ok[::18] = 0
    c["ok"] = ok
    gp = small()
    want = ref(oracle, gp, **c)
    assert planned_share(want) >= 0.8  # of all 70, the four with ok = 0 among them
    for drop in KEYS[1:]:  # every optional output NULL in turn (states is required: the entry refuses)
        keys = tuple(k for k in KEYS if k != drop)
        if drop == "states":
            with pytest.raises(binding.PoError):
                run_device(eng, c, gp, want=keys)
            continue
        assert_same(run_device(eng, c, gp, want=keys), want, keys=keys, tag="without " + drop)
    assert_same(run_device(eng, c, gp, want=("status", "states")), want, keys=("status", "states"), tag="required alone")
    for drop in ("n_states", "ok", "v_cap", "set_of"):  # every optional input NULL in turn
        both(eng, oracle, gp, tag="no " + drop, share=0.8, **{k: v for k, v in c.items() if k != drop})
    r = eng.stgo_batch(want_rows=False, params=gp, **c)
    assert r["cells"] is None
    assert_same(r, want, keys=tuple(k for k in KEYS if k != "cells"), tag="host, no rows")
    # B = 0: PO_OK from both entries, nothing is looked at and nothing written
    L = binding.lib()
    out = sentinels(3, gp.K, gp.Q)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for entry in (L.po_stgo_batch, L.po_stgo_batch_device):
        gi = abi.PoStgoIn(); gi.N = 5
        assert entry(eng._h, ctypes.byref(gp), ctypes.byref(gi), ctypes.byref(abi.PoStgoOut(*[p(out[k]) for k in KEYS]))) == abi.PO_OK
    assert_same(out, sentinels(3, gp.K, gp.Q), tag="B = 0")
    none = dict(c, agents=[[], []], set_of=np.zeros(70, dtype=np.int32))  # no agents at all: no cell is blocked
    r = both(eng, oracle, gp, tag="no agents", share=0.8, **none)
    assert set(r["status"].tolist()) <= {0, 1, 3} and (r["cells"] == -1).all()


@pytest.mark.gpu
def test_device_lists_are_read_clamped(eng, oracle):
    """What the host entry refuses, the device entry reads as the definition says: set_of and first clamped, an agent with a bad n_pts covers nothing."""
    c = random_case(SEEDS["clamped"], 6, 30, per_set=(5, 5), ragged=False, waits=False)
    agents, first = c["agents"]
    agents = agents.copy(); agents["n_pts"][2] = 9; agents["n_pts"][7] = -1
    c["agents"] = (agents, np.array([-3, 5, 99], dtype=np.int32))
    c["set_of"] = np.array([0, 1, -2, 7, 1, 0], dtype=np.int32)
    gp = small(margin=0.8)
    want = ref(oracle, gp, **c)
    assert planned_share(want) >= 0.8
    assert_same(run_device(eng, c, gp), want, tag="clamped")
    assert (want["cells"] >= 0).any() and not np.isin(want["cells"], [2, 7]).any()
    with pytest.raises(binding.PoError):
        eng.stgo_batch(params=gp, **c)


def _dyn_outputs(B, N):
    dkeys = {"status": np.int32, "ok_out": np.int32, "gap_min": np.float64, "first_state": np.int32, "first_agent": np.int32, "stop_state": np.int32,
             "first_time": np.float64, "gap": np.float64, "v_limit": np.float64}
    return {k: _dev(np.full((B, N) if k in ("gap", "v_limit") else (B,), 77 if t == np.int32 else 7.0, dtype=t)) for k, t in dkeys.items()}


@pytest.mark.gpu
def test_chain_speed_stgo_on_one_stream(oracle):
    """speed -> stgo (v_cap = that profile's v), device entries only, no synchronisation and no host copy between the calls; equal to the composed references."""
    import torch

    c0, agents = ts.closure_case()
    agents = [agents[0] + held_until(4.0, 9.0)[0]]
    B, N = c0["states"].shape[0], c0["states"].shape[1]
    gp, spd = params_of(stride=2, margin=1.5, dts=0.25, Q=37), ts.no_map()
    e = binding.Engine(0)
    f64 = lambda: _dev(np.full((B, N), 7.0))
    speed = {"v": f64(), "a": f64(), "t": f64(), "total_time": _dev(np.full(B, 7.0)), "status": _dev(np.full(B, 77, dtype=np.int32))}
    plan = {k: _dev(v) for k, v in sentinels(B, gp.K, gp.Q).items()}
    p_in = device_inputs(dict(states=c0["states"], v0=c0["v0"], ok=c0["ok"], agents=agents))
    torch.cuda.synchronize()
    e.speed_batch_device({"states": p_in["states"], "ok": p_in["ok"], "v0": p_in["v0"]}, speed, spd)
    e.stgo_batch_device(dict(p_in, v_cap=speed["v"]), plan, gp)
    got_s, got_p = {k: _host(v) for k, v in speed.items()}, {k: _host(v) for k, v in plan.items()}
    e.close()
    p0 = speed_ref.profile(oracle.default_params(), c0["states"], c0["v0"], spd, ok=c0["ok"])
    want = ref(oracle, gp, states=c0["states"], v0=c0["v0"], ok=c0["ok"], agents=agents, v_cap=p0["v"])
    assert_same(got_s, p0, keys=("v", "a", "t", "total_time", "status"), tag="speed"); assert_same(got_p, want, tag="stgo")
    assert want["status"].tolist() == [2, 2, 2, 0]


@pytest.mark.gpu
def test_chain_stgo_dynamic_and_stgo_trajectory_dynamic_on_one_stream(oracle):
    """stgo -> dynamic on out->states / out->t, and stgo -> trajectory (D = 4) -> dynamic for a second vehicle against the first one's records: device entries
    only on one stream, no synchronisation and no host copy in between; equal to the chains of the two closure tests on the references."""
    import torch

    c, gp, r = closure_plan(oracle)
    params = oracle.default_params()
    ag, first = binding.pack_agents(c["agents"])
    tp = trajectory_of(gp, discs=binding.covering_discs(params))
    st2, t2, _ = second_vehicle(r, gp)
    e = binding.Engine(0)
    plan = {k: _dev(v) for k, v in sentinels(1, gp.K, gp.Q).items()}
    dyn1, dyn2 = _dyn_outputs(1, gp.Q), _dyn_outputs(1, st2.shape[1])
    i32 = lambda *s: _dev(np.full(s, 77, dtype=np.int32))
    f64 = lambda *s: _dev(np.full(s, 7.0))
    traj = {"status": i32(1), "states": f64(1, gp.Q, 5), "v": f64(1, gp.Q), "a": f64(1, gp.Q), "t": f64(1, gp.Q), "index": i32(1, gp.Q), "first_held": i32(1),
            "agents": _dev(np.full(4 * 208, 7, dtype=np.uint8))}
    p_in = device_inputs(c)
    first2, st2_d, t2_d = _dev(np.array([0, 4], dtype=np.int32)), _dev(st2), _dev(t2)
    torch.cuda.synchronize()
    e.stgo_batch_device(p_in, plan, gp)
    e.dynamic_batch_device({"states": plan["states"], "t": plan["t"], "agents": p_in["agents"], "first": p_in["first"]}, dyn1, dyn_params())
    e.trajectory_batch_device({"states": plan["states"], "v": plan["v"], "t": plan["t"]}, traj, tp)
    e.dynamic_batch_device({"states": st2_d, "t": t2_d, "agents": traj["agents"], "first": first2}, dyn2, dyn_params())
    got = [{k: _host(v) for k, v in o.items()} for o in (plan, dyn1, traj, dyn2)]
    e.close()
    assert_same(got[0], r, tag="stgo")
    dkeys = tuple(dyn1)
    d1 = dynamic_ref.check(params, r["states"], r["t"], ag, first, dyn_params())
    assert_same(got[1], d1, keys=dkeys, tag="dynamic 1"); assert d1["status"][0] == 1
    tr = trajectory_ref.trajectory(r["states"], r["v"], r["t"], tp)
    assert_same(got[2], tr, keys=("status", "states", "v", "a", "t", "index", "first_held"), tag="trajectory")
    assert got[2]["agents"].tobytes() == tr["agents"].tobytes()
    d2 = dynamic_ref.check(params, st2, t2, tr["agents"], np.array([0, 4], dtype=np.int32), dyn_params())
    assert_same(got[3], d2, keys=dkeys, tag="dynamic 2"); assert d2["status"][0] == 2


@pytest.mark.gpu
def test_host_mirror_stgo_program(eng, oracle):
    """StGoPlanner::plan end to end in its own process: its statuses, layer counts, resumes and its checksum of the samples and stations equal the Python call's."""
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "stgo_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "stgo_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "stgo_test passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]
    printed = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("status", "layers", "resumes", "end", "checksum")}
    c, gp = mirror_case()
    got = both(eng, oracle, gp, tag="mirror case", **c)
    assert printed["status"] == got["status"].tolist() and printed["layers"] == got["n_layers"].tolist() and got["status"][4] == 0
    assert printed["resumes"] == got["n_resumes"].tolist() and printed["end"] == got["end"].tolist()
    total = 0
    for b in range(len(c["n_states"])):
        total += int(got["states"][b].view(np.uint64).sum(dtype=np.uint64)) + int(got["v"][b].view(np.uint64).sum(dtype=np.uint64))
        total += int(got["station"][b, :got["n_layers"][b] + 1].sum()) if got["status"][b] in (1, 2) else 0
    assert printed["checksum"] == [total & 0xffffffffffffffff]
