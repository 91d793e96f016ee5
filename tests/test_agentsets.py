"""Agent sets on the device: po_agentsets_batch* (csrc/po_agentsets.hip; include/po_hip.h states the definition).

A kept record is a copy and every decision is a fixed sequence of rounded IEEE double operations and comparisons, so every comparison with the device here is
BIT equality on byte views against tests/agentsets_ref.py (numpy, one ufunc per operation), outputs sentinel-filled so that what is not written shows.  No
tolerance appears anywhere in this file.

CPU: the reference against a scalar loop over the definition; the property the stage exists for (po_dynamic_batch's definition gives the same answer on the
composed sets as on host-built everybody-but-me sets, while fewer than half the records are kept); closed forms at the four box ties and the two time ties;
arguments refused without a device; exports, the ABI mirror, the host mirror.  GPU: pool sizes, path lengths and batch sizes around the wave size, position
independence, the scan's chunk boundary, clipping, every filter, lists read clamped, not-composed egos, optional pointers, the chain speed -> trajectory -> agent
sets -> dynamic on one stream, reuse of a handle, the C++ mirror's program."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import agentsets_ref
import dynamic_ref
import speed_ref
import trajectory_ref
from path_optimizer_amd import abi, binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["po_default_agentsets_params", "po_agentsets_batch", "po_agentsets_batch_device"]
KEYS = ("agents", "first", "count", "status", "set_of", "src_index", "total")
BEFORE, AFTER = abi.PO_AGENT_HOLD_BEFORE, abi.PO_AGENT_HOLD_AFTER
AGENT = binding.AGENT_DTYPE
FILL_BYTE, FILL_INT = 0x77, 77
# the scan's step, read from the source: the batch sizes of the chunk-boundary test sit around it and change with it
SCAN_CHUNK = int(re.search(r"constexpr int kSetsScanChunk = (\d+);", open(os.path.join(ROOT, "path_optimizer_amd", "csrc", "po_agentsets.hip")).read()).group(1))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(got, want, keys=KEYS, tag=""):
    for k in keys:
        if k not in got or got[k] is None:
            continue
        if k == "total":
            assert int(got[k]) == int(want[k]), (tag, k, got[k], want[k])
            continue
        if not same(got[k], want[k]):
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert g.shape == w.shape and g.dtype == w.dtype, (tag, k, g.shape, w.shape, g.dtype, w.dtype)
            bad = np.flatnonzero((g.reshape(-1).view(np.uint8).reshape(len(g), -1) != w.reshape(-1).view(np.uint8).reshape(len(g), -1)).any(axis=1))
            raise AssertionError(f"{tag} {k}: rows {bad[:8]} differ; got {g[bad[0]]} want {w[bad[0]]}")


def params_of(**kw):
    p = binding.default_agentsets_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def random_records(rng, count, area, valid=True):
    """count records: 1 .. 8 points, times sorted inside (-2, 14), centres on a random walk inside and around the area, every flag combination; the words at and
    behind n_pts hold finite garbage (they are copied as they are).  valid = False: one record in four covers nothing, each in another way, and one in four
    has its times shuffled."""
    rec = np.zeros(count, dtype=AGENT)
    for i in range(count):
        g = rec[i]
        g["n_pts"], g["flags"], g["radius"] = rng.integers(1, 9), rng.integers(0, 4), rng.uniform(0, 1.5)
        g["t"] = np.sort(rng.uniform(-2, 14, 8))
        g["x"] = rng.uniform(-area / 2 - 5, area / 2 + 5) + np.cumsum(rng.normal(0, 1.5, 8))
        g["y"] = rng.uniform(-area / 2 - 5, area / 2 + 5) + np.cumsum(rng.normal(0, 1.5, 8))
        if not valid and i % 4 == 1:
            j = int(rng.integers(0, g["n_pts"]))
            how = (i // 4) % 8
            if how == 0: g["n_pts"] = 0
            elif how == 1: g["n_pts"] = 9
            elif how == 2: g["n_pts"] = -3
            elif how == 3: g["radius"] = -0.25
            elif how == 4: g["radius"] = np.nan
            elif how == 5: g["t"][j] = np.inf
            elif how == 6: g["x"][j] = np.nan
            else: g["y"][j] = -np.inf
        if not valid and i % 4 == 3:
            g["t"] = rng.permutation(g["t"])
    return rec


def make_scene(seed, B, N, sizes0=(8,), sizes1=None, valid=True, ragged=True, area=40.0):
    """B ego paths of N rows (0.5 m steps on gently curved paths from random poses, constant speed, t = t_start + s / v) and two source lists in pools of the
    given sizes (sizes1 None: no second source).  pool_of is random over the pools of source 0."""
    rng = np.random.default_rng([77, seed])
    states, t = np.zeros((B, N, 5)), np.zeros((B, N))
    s = 0.5 * np.arange(N)
    for b in range(B):
        k = rng.uniform(-0.05, 0.05)
        z = rng.uniform(-math.pi, math.pi) + k * s
        x = rng.uniform(-area / 2, area / 2) + np.concatenate(([0.0], np.cumsum(0.5 * np.cos(z[:-1]))))
        y = rng.uniform(-area / 2, area / 2) + np.concatenate(([0.0], np.cumsum(0.5 * np.sin(z[:-1]))))
        states[b] = np.stack([x, y, z, np.full(N, k), s], axis=1)
        t[b] = rng.uniform(0, 4) + s / rng.uniform(1, 6)
    n = rng.integers(0, N + 1, B).astype(np.int32) if ragged else np.full(B, N, dtype=np.int32)
    n[rng.integers(0, B)] = N
    c = dict(states=states, t=t, n_states=n, pool_of=rng.integers(0, len(sizes0), B).astype(np.int32))
    first0 = np.concatenate(([0], np.cumsum(sizes0))).astype(np.int32)
    c["sources"] = [(random_records(rng, int(first0[-1]), area, valid), first0)]
    if sizes1 is not None:
        first1 = np.concatenate(([0], np.cumsum(sizes1))).astype(np.int32)
        c["sources"].append((random_records(rng, int(first1[-1]), area, valid), first1))
    return c


def ref(ap, capacity=None, **c):
    return agentsets_ref.compose(c["states"], c.get("t"), c["sources"], ap, n_states=c.get("n_states"), ok=c.get("ok"), pool_of=c.get("pool_of"),
                                 owner=c.get("owner"), capacity=capacity, fill_byte=FILL_BYTE, fill_index=FILL_INT)


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def _scalar_sets(c, ap):
    """The definition as plain scalar Python loops (Python floats are IEEE doubles): per ego the list of kept (source, index)."""
    fin = lambda q: abs(q) <= 1.7976931348623157e308
    mn = lambda a, b: b if b < a else a
    mx = lambda a, b: b if b > a else a
    states, t = c["states"], c.get("t")
    B, N = states.shape[0], states.shape[1]
    out = []
    for b in range(B):
        n = N if c.get("n_states") is None else min(max(int(c["n_states"][b]), 0), N)
        rows = [(float(states[b, i, 0]), float(states[b, i, 1])) for i in range(n)]
        ts = None if t is None else [float(t[b, i]) for i in range(n)]
        if (c.get("ok") is not None and c["ok"][b] == 0) or n < 1 or not all(fin(x) and fin(y) for x, y in rows) or (ts is not None and not all(fin(q) for q in ts)):
            out.append(None)
            continue
        exl = exh = rows[0][0]; eyl = eyh = rows[0][1]
        for x, y in rows:
            exl, exh, eyl, eyh = mn(exl, x), mx(exh, x), mn(eyl, y), mx(eyh, y)
        if ts is None:
            W0, W1 = float(ap.win_lo), float(ap.win_hi)
        else:
            tl = th = ts[0]
            for q in ts:
                tl, th = mn(tl, q), mx(th, q)
            W0, W1 = tl - float(ap.t_before), th + float(ap.t_after)
        kept = []
        for s, src in enumerate(c["sources"]):
            if src is None:
                continue
            agents, first = src
            S, na = len(first) - 1, len(agents)
            if S < 1 or na < 1:
                continue
            k = min(max(int(c["pool_of"][b]) if c.get("pool_of") is not None else 0, 0), S - 1)
            lo, hi = min(max(int(first[k]), 0), na), min(max(int(first[k + 1]), 0), na)
            for a in range(lo, hi):
                g = agents[a]
                np_, R = int(g["n_pts"]), float(g["radius"])
                if np_ < 1 or np_ > 8 or not (R >= 0):
                    continue
                T, X, Y = [float(q) for q in g["t"][:np_]], [float(q) for q in g["x"][:np_]], [float(q) for q in g["y"][:np_]]
                if not all(fin(q) for q in T + X + Y):
                    continue
                if s == 0:
                    if c.get("owner") is not None:
                        if int(c["owner"][a]) == b:
                            continue
                    elif ap.owner_div > 0 and a // int(ap.owner_div) == b:
                        continue
                A0 = A1 = T[0]; axl = axh = X[0]; ayl = ayh = Y[0]
                for j in range(np_):
                    A0, A1, axl, axh, ayl, ayh = mn(A0, T[j]), mx(A1, T[j]), mn(axl, X[j]), mx(axh, X[j]), mn(ayl, Y[j]), mx(ayh, Y[j])
                if int(g["flags"]) & BEFORE: A0 = -math.inf
                if int(g["flags"]) & AFTER: A1 = math.inf
                if not (A0 <= W1 and A1 >= W0):
                    continue
                rr = R + float(ap.reach)
                if axl - rr <= exh and axh + rr >= exl and ayl - rr <= eyh and ayh + rr >= eyl:
                    kept.append((s, a))
        out.append(kept)
    return out


def test_reference_agrees_with_a_scalar_loop_over_the_definition():
    kept_any = dropped_any = 0
    for seed, kw in enumerate((dict(owner_div=2), dict(owner_div=0, t_before=1.5, t_after=0.5), dict(owner_div=3, reach=4.0), dict(owner_div=1, win_lo=2.0, win_hi=3.0))):
        c = make_scene(seed, 20, 30, sizes0=(13, 0, 30), sizes1=(5, 9, 1), valid=False)
        c["ok"] = np.ones(20, dtype=np.int32); c["ok"][5] = 0
        c["states"][3, 1, 0] = np.nan; c["t"][8, 0] = np.inf; c["n_states"][3] = max(c["n_states"][3], 2); c["n_states"][8] = max(c["n_states"][8], 1)
        c["pool_of"][2] = 7; c["pool_of"][4] = -1
        if seed == 1:
            c["owner"] = np.random.default_rng(5).integers(-2, 23, 43).astype(np.int32)
        if seed == 3:
            c["t"] = None
        ap = params_of(**{**dict(reach=8.0), **kw})
        r = ref(ap, **c)
        want = _scalar_sets(c, ap)
        n0 = len(c["sources"][0][0])
        for b in range(20):
            assert (r["status"][b] == 0) == (want[b] is None), (seed, b)
            assert r["kept"][b] == [a if s == 0 else n0 + a for s, a in (want[b] or [])], (seed, b)
            assert r["count"][b] == len(want[b] or [])
        assert r["status"][3] == 0 and r["status"][5] == 0 and (seed == 3 or r["status"][8] == 0)
        F = np.concatenate(([0], np.cumsum(r["count"])))
        assert same(r["first"], F.astype(np.int32)) and r["total"] == F[-1] == len(r["agents"])
        for b in range(20):
            for q, (s, a) in enumerate(want[b] or []):
                assert same(r["agents"][F[b] + q], c["sources"][s][0][a])
        kept_any += r["total"]
        dropped_any += sum(len(x[0]) for x in c["sources"]) * 20 - r["total"]
    assert kept_any > 100 and dropped_any > 100


def fleet_scene(seed, V=12, N=48, D=2):
    """One world of V vehicles: N states 0.5 m apart on gently curved paths from random poses in a 60 m square, constant speeds of 2 .. 6 m/s with
    t = t_start + s / v; D records of 8 points per vehicle, radius 1 m, at offsets 0 and 2 m along the heading, sampled at 8 times across the path's own span,
    with random hold flags."""
    rng = np.random.default_rng([91, seed])
    s = 0.5 * np.arange(N)
    states, t = np.zeros((V, N, 5)), np.zeros((V, N))
    rec = np.zeros(V * D, dtype=AGENT)
    for b in range(V):
        k = rng.uniform(-0.03, 0.03)
        z = rng.uniform(-math.pi, math.pi) + k * s
        x = rng.uniform(-30, 30) + np.concatenate(([0.0], np.cumsum(0.5 * np.cos(z[:-1]))))
        y = rng.uniform(-30, 30) + np.concatenate(([0.0], np.cumsum(0.5 * np.sin(z[:-1]))))
        states[b] = np.stack([x, y, z, np.full(N, k), s], axis=1)
        t[b] = rng.uniform(0, 3) + s / rng.uniform(2, 6)
        at = np.linspace(0, N - 1, 8).round().astype(int)
        for d in range(D):
            g = rec[b * D + d]
            g["n_pts"], g["flags"], g["radius"] = 8, rng.integers(0, 4), 1.0
            g["t"], g["x"], g["y"] = t[b, at], x[at] + 2.0 * d * np.cos(z[at]), y[at] + 2.0 * d * np.sin(z[at])
    return states, t, rec


def test_composed_sets_are_conservative_and_useful(oracle):
    """po_dynamic_batch's definition on the composed sets equals the same on host-built everybody-but-me sets in status, first_state, stop_state, first_time and
    v_limit, bit for bit, and first_agent names the same record through src_index (gap_min and gap may differ: a dropped record's gap is larger than the
    margin, not absent).  So that neither a filter that keeps everything nor an empty scene passes: fewer than half the records are kept overall and at least a
    quarter of the paths are in conflict."""
    op, dp = oracle.default_params(), binding.default_dynamic_params()
    V, D = 12, 2
    ap = params_of(reach=binding.footprint_reach(op, dp.margin), owner_div=D)
    kept = offered = conflicts = paths = 0
    for seed in range(12):
        states, t, rec = fleet_scene(seed, V=V, D=D)
        r = agentsets_ref.compose(states, t, [(rec, np.array([0, V * D], dtype=np.int32))], ap)
        others = [[a for a in range(V * D) if a // D != b] for b in range(V)]
        full = np.concatenate([rec[o] for o in others])
        full_first = np.concatenate(([0], np.cumsum([len(o) for o in others]))).astype(np.int32)
        full_index = np.concatenate(others)
        want = dynamic_ref.check(op, states, t, full, full_first, dp, set_of=np.arange(V))
        got = dynamic_ref.check(op, states, t, r["agents"], r["first"], dp, set_of=r["set_of"])
        for k in ("status", "first_state", "stop_state", "first_time", "v_limit"):
            assert same(got[k], want[k]), (seed, k)
        hit = np.flatnonzero(want["status"] >= 2)
        assert (r["src_index"][got["first_agent"][hit]] == full_index[want["first_agent"][hit]]).all(), seed
        assert (got["first_agent"][want["status"] == 1] == -1).all()
        for b in range(V):
            assert all(a // D != b for a in r["kept"][b]), (seed, b)
        kept += r["total"]; offered += len(full); conflicts += len(hit); paths += V
    print(f"{conflicts} of {paths} paths in conflict, {kept} of {offered} records kept")
    assert kept < offered / 2 and conflicts >= paths / 4, (kept, offered, conflicts, paths)


def line_ego():
    """One ego along +x: 21 states 0.5 m apart from the origin, t_i = 0.5 i — its box is [0, 10] x [0, 0] and its times span [0, 10]."""
    states = np.zeros((1, 21, 5)); states[0, :, 0] = 0.5 * np.arange(21); states[0, :, 4] = states[0, :, 0]
    return states, (0.5 * np.arange(21))[None, :]


def standing(x, y, T=5.0, R=1.0, flags=0):
    return (R, flags, [(T, x, y)])


def test_closed_forms_at_the_box_ties_and_the_time_ties():
    states, t = line_ego()
    ap = params_of(reach=2.0, t_before=0.5, t_after=0.25, owner_div=0)  # rr = 3; W0 = -0.5, W1 = 10.25
    up, down = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    cases = [  # (record, kept)
        (standing(13.0, 0.0), True), (standing(up(13.0), 0.0), False),          # axl - rr <= exh
        (standing(-3.0, 0.0), True), (standing(down(-3.0), 0.0), False),        # axh + rr >= exl
        (standing(5.0, 3.0), True), (standing(5.0, up(3.0)), False),            # ayl - rr <= eyh
        (standing(5.0, -3.0), True), (standing(5.0, down(-3.0)), False),        # ayh + rr >= eyl
        (standing(5.0, 0.0, T=10.25), True), (standing(5.0, 0.0, T=up(10.25)), False),   # A0 <= W1
        (standing(5.0, 0.0, T=-0.5), True), (standing(5.0, 0.0, T=down(-0.5)), False),   # A1 >= W0
        (standing(5.0, 0.0, T=-1.0, flags=AFTER), True), (standing(5.0, 0.0, T=-1.0, flags=BEFORE), False),  # a hold opens its own side only
        (standing(5.0, 0.0, T=20.0, flags=BEFORE), True), (standing(5.0, 0.0, T=20.0, flags=AFTER), False),
        ((1.0, 0, [(20.0, 5.0, 0.0), (5.0, 5.0, 0.0), (30.0, 5.0, 0.0)]), True),      # non-monotone T: the minimum 5 is inside, first and last are not
        ((1.0, 0, [(-9.0, 5.0, 0.0), (-20.0, 5.0, 0.0), (-8.0, 5.0, 0.0)]), False),   # ... and its maximum -8 is before W0
        ((0.0, 0, [(5.0, -4.0, 9.0), (6.0, 14.0, -9.0)]), True),                      # the record's BOX meets the path's, its points do not
    ]
    agents, first = binding.pack_agents([[rec for rec, _ in cases]])
    r = agentsets_ref.compose(states, t, [(agents, first)], ap)
    assert r["kept"][0] == [i for i, (_, keep) in enumerate(cases) if keep], r["kept"][0]
    assert r["status"].tolist() == [1] and r["first"].tolist() == [0, r["total"]] and r["src_index"].tolist() == r["kept"][0]
    # the ego's span is the minimum and maximum of t, not its first and last entries: t = 5, 0, 10, 3 spans [0, 10]
    st4 = states[:, :4].copy()
    src = binding.pack_agents([[standing(1.0, 0.0, T=0.2), standing(1.0, 0.0, T=9.9), standing(1.0, 0.0, T=10.5)]])
    r = agentsets_ref.compose(st4, np.array([[5.0, 0.0, 10.0, 3.0]]), [src], params_of(reach=2.0, owner_div=0))
    assert r["kept"][0] == [0, 1]
    # without t the window is win_lo .. win_hi, ties included
    ap = params_of(reach=2.0, win_lo=1.0, win_hi=4.0, owner_div=0)
    agents, first = binding.pack_agents([[standing(1.0, 0.0, T=4.0), standing(1.0, 0.0, T=up(4.0)), standing(1.0, 0.0, T=1.0), standing(1.0, 0.0, T=down(1.0))]])
    assert agentsets_ref.compose(states, None, [(agents, first)], ap)["kept"][0] == [0, 2]


def test_footprint_reach_covers_every_footprint_circle(oracle):
    import select_ref

    op = oracle.default_params()
    cx, cy, cr = select_ref.car_circles(op)
    far = max(math.hypot(cx[q], cy[q]) + cr[q] for q in range(6))
    assert binding.footprint_reach(op, 0.3) == far + 0.3 + 1e-6 and binding.footprint_reach(binding.default_params(), 0.3) == binding.footprint_reach(op, 0.3)
    assert binding.footprint_reach(op, 0.0) > far


# ---- interface without a device ----
FIELDS = {"po_agentsets_params": ["reach", "t_before", "t_after", "win_lo", "win_hi", "owner_div"],
          "po_agentsets_in": ["B", "N", "states", "n_states", "ok", "t", "src", "pool_of", "owner"],
          "po_agentsets_out": ["capacity", "agents", "first", "count", "status", "set_of", "src_index", "total"]}


def test_new_symbols_and_abi_mirror():
    L = binding.lib()
    for name in NEW_ENTRIES:
        assert hasattr(L, name), name
        assert name in binding.EXPORTS
    mirror = {"po_agentsets_params": abi.PoAgentsetsParams, "po_agentsets_in": abi.PoAgentsetsIn, "po_agentsets_out": abi.PoAgentsetsOut}
    body = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs) for s, fs in FIELDS.items())
    body += 'printf("%zu %d %d", sizeof(po_agent), PO_SETS_SOURCES, PO_ABI_VERSION);'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "po_hip.h"\nint main(){' + body + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    want = []
    for s, fs in FIELDS.items():
        want.append(ctypes.sizeof(mirror[s]))
        want += [getattr(mirror[s], f).offset for f in fs]
    want += [ctypes.sizeof(abi.PoAgent), abi.PO_SETS_SOURCES, abi.PO_ABI_VERSION]
    assert got == want and abi.PO_ABI_VERSION == 7 and abi.PO_SETS_SOURCES == 2 and agentsets_ref.AGENT_DTYPE == AGENT
    assert [f for f, _ in abi.PoAgentsetsOut._fields_][1:] == list(KEYS) == list(binding.Engine.AGENTSETS_KEYS)
    p = binding.default_agentsets_params()
    assert [p.reach, p.t_before, p.t_after, p.win_lo, p.win_hi, p.owner_div] == [5.0, 0.0, 0.0, 0.0, 8.0, 0]


def bad_params():
    out = [(f, v) for f in ("reach", "t_before", "t_after") for v in (-1e-300, np.nan, np.inf, -np.inf)]
    out += [(f, v) for f in ("win_lo", "win_hi") for v in (np.nan, np.inf, -np.inf)]
    return out + [("win_lo", 8.5), ("win_hi", -0.5), ("owner_div", -1)]


def test_null_arguments_ranges_and_aliasing_are_refused_without_a_device():
    """The argument checks come before the handle is touched, so any non-NULL handle value shows them here."""
    L = binding.lib()
    ap, ai, ao = params_of(), abi.PoAgentsetsIn(), abi.PoAgentsetsOut()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))
    buf, ibuf = np.zeros(256), np.zeros(256, dtype=np.int32)
    recs, orecs = np.zeros(8, dtype=AGENT), np.zeros(8, dtype=AGENT)
    first = np.array([0, 8], dtype=np.int32)
    p = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)
    lists = lambda a=recs, n=8, S=1, f=first: abi.PoAgentLists(p(a) if a is not None else None, p(f) if f is not None else None, n, S)
    for entry in (L.po_agentsets_batch, L.po_agentsets_batch_device):
        assert entry(None, ctypes.byref(ap), ctypes.byref(ai), ctypes.byref(ao)) == abi.PO_ERR_INVALID
        assert entry(None, None, None, None) == abi.PO_ERR_INVALID
        assert entry(fake, None, ctypes.byref(ai), ctypes.byref(ao)) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(ap), None, ctypes.byref(ao)) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(ap), ctypes.byref(ai), None) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(ap), ctypes.byref(ai), ctypes.byref(ao)) == abi.PO_OK  # B = 0: nothing to do, and the handle is not looked at
        for f, v in bad_params():  # B = 0 is decided AFTER the checks
            assert entry(fake, ctypes.byref(params_of(**{f: v})), ctypes.byref(ai), ctypes.byref(ao)) == abi.PO_ERR_INVALID, (f, v)
        edge = params_of(reach=0.0, t_before=0.0, t_after=1e308, win_lo=-3.0, win_hi=-3.0, owner_div=2 ** 31 - 1)  # the edges of the ranges are inside
        assert entry(fake, ctypes.byref(edge), ctypes.byref(ai), ctypes.byref(ao)) == abi.PO_OK
        for f in ("B", "N"):
            bad = abi.PoAgentsetsIn(); setattr(bad, f, -1)
            assert entry(fake, ctypes.byref(ap), ctypes.byref(bad), ctypes.byref(ao)) == abi.PO_ERR_INVALID, f
        bad = abi.PoAgentsetsOut(); bad.capacity = -1
        assert entry(fake, ctypes.byref(ap), ctypes.byref(ai), ctypes.byref(bad)) == abi.PO_ERR_INVALID
        for bad_list in (lists(n=-1), lists(S=-1)):  # a list's own negative sizes are refused even with B = 0, in either source
            for s in (0, 1):
                bi = abi.PoAgentsetsIn(); bi.src[s] = ctypes.pointer(bad_list)
                assert entry(fake, ctypes.byref(ap), ctypes.byref(bi), ctypes.byref(ao)) == abi.PO_ERR_INVALID, s

        # B > 0: every required pointer missing in turn is refused before the handle is read
        held = []

        def full(l0=None, l1=None):
            fi = abi.PoAgentsetsIn(1, 2, p(buf), None, None, None)
            held.extend([l0 if l0 is not None else lists(), l1])
            fi.src[0] = ctypes.pointer(held[-2])
            if l1 is not None:
                fi.src[1] = ctypes.pointer(l1)
            fo = abi.PoAgentsetsOut(8, p(orecs), p(ibuf), p(ibuf, 64), p(ibuf, 128), None, None, None)
            return fi, fo

        fi, fo = full(); fi.states = None
        assert entry(fake, ctypes.byref(ap), ctypes.byref(fi), ctypes.byref(fo)) == abi.PO_ERR_INVALID
        fi, fo = full(); fi.src[0] = None
        assert entry(fake, ctypes.byref(ap), ctypes.byref(fi), ctypes.byref(fo)) == abi.PO_ERR_INVALID
        for key in ("first", "count", "status", "agents"):
            fi, fo = full(); setattr(fo, key, None)
            assert entry(fake, ctypes.byref(ap), ctypes.byref(fi), ctypes.byref(fo)) == abi.PO_ERR_INVALID, key
        # lists refused by their shape: no pool, no first, records missing — in source 0, and in a source 1 that is used
        for bad_list in (lists(S=0), lists(f=None), lists(a=None)):
            fi, fo = full(l0=bad_list)
            assert entry(fake, ctypes.byref(ap), ctypes.byref(fi), ctypes.byref(fo)) == abi.PO_ERR_INVALID
        for bad_list in (lists(f=None), lists(a=None)):
            fi, fo = full(l1=bad_list)
            assert entry(fake, ctypes.byref(ap), ctypes.byref(fi), ctypes.byref(fo)) == abi.PO_ERR_INVALID
        # out->agents overlapping a source array, of either source: the same address, and ranges that only overlap at one end
        other = np.zeros(8, dtype=AGENT)
        for s in (0, 1):
            for off in (0, 7 * 208, -7 * 208):
                fi, fo = full(l0=lists(a=other) if s == 1 else None, l1=lists() if s == 1 else lists(a=other))
                fo.agents = ctypes.c_void_p(recs.ctypes.data + off)
                assert entry(fake, ctypes.byref(ap), ctypes.byref(fi), ctypes.byref(fo)) == abi.PO_ERR_INVALID, (s, off)
    L.po_default_agentsets_params(None)  # a NULL struct is ignored


def test_host_mirror_header_compiles():
    inc = os.path.join(ROOT, "path_optimizer_amd", "host", "include")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "path_optimizer_amd/agent_sets.hpp"\nint main() { PathOptimizationNS::AgentSets s; (void)s; return 0; }\n')
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-I", os.path.join(ROOT, "include"), src])


def test_host_mirror_agentsets_test_compiles_and_links():
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "agentsets_test"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(host, "agentsets_test"))
    assert "AgentSets" in open(os.path.join(host, "test", "agentsets_test.cpp")).read()


def mirror_case():
    """The seeded case of host/test/agentsets_test.cpp, rebuilt with the same integer generator and the same dyadic arithmetic: bit for bit its inputs.  Two
    worlds of three vehicles, 1 .. 12 states, two records per vehicle and two perception records per world."""
    state = [13579]

    def u():
        state[0] = (state[0] * 1103515245 + 12345) & 0x7fffffff
        return (((state[0] >> 8) % 257) - 128) / 64.0

    B, D = 6, 2
    n = np.array([1 + (b * 5) % 12 for b in range(B)], dtype=np.int32)
    N = int(n.max())
    states, t = np.zeros((B, N, 5)), np.zeros((B, N))
    fleet = [[], []]
    for b in range(B):
        x0, y0, t0 = 4 * u(), 4 * u(), u()
        for i in range(n[b]):
            states[b, i] = (x0 + 0.5 * i, y0 + u() / 8, 0.0, 0.0, 0.5 * i)
            t[b, i] = t0 + 0.25 * i
        for d in range(D):
            fleet[b // 3].append((0.5 + 0.25 * d, AFTER if d else 0, [(t0 + 0.25 * j * int(n[b]), x0 + 0.5 * j * int(n[b]) + d, y0) for j in range(2)]))
    seen = [[(0.75, BEFORE | AFTER, [(0.0, 4 * u(), 4 * u())]), (0.25, 0, [(u(), 8 * u(), 8 * u()), (5.0 + u(), 8 * u(), 8 * u())])] for _ in range(2)]
    ok = np.ones(B, dtype=np.int32); ok[4] = 0
    ap = params_of(reach=4.0, t_before=0.25, t_after=0.5, owner_div=D)
    return dict(states=states, t=t, n_states=n, ok=ok, pool_of=np.array([0, 0, 0, 1, 1, 1], dtype=np.int32),
                sources=[binding.pack_agents(fleet), binding.pack_agents(seen)]), ap


def test_mirror_case_exercises_the_stage():
    c, ap = mirror_case()
    r = ref(ap, **c)
    assert r["status"][4] == 0 and (np.delete(r["status"], 4) == 1).all() and 0 < r["total"] < 5 * 6
    assert (r["src_index"] >= 12).any() and (r["src_index"] < 12).any()  # both sources contribute
    # (the host entry takes the lists: strictly increasing t)
    for ag, _ in c["sources"]:
        for g in ag:
            assert (np.diff(g["t"][:g["n_pts"]]) > 0).all()


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


def sentinels(B, cap, want=KEYS):
    """Outputs that start as 77 (the records as bytes of 0x77); no agents and no src_index with capacity 0."""
    r = {"first": np.full(B + 1, FILL_INT, dtype=np.int32), "count": np.full(B, FILL_INT, dtype=np.int32), "status": np.full(B, FILL_INT, dtype=np.int32)}
    if "set_of" in want: r["set_of"] = np.full(B, FILL_INT, dtype=np.int32)
    if "total" in want: r["total"] = np.full(1, FILL_INT, dtype=np.int64)
    if cap > 0:
        r["agents"] = np.full(cap * 208, FILL_BYTE, dtype=np.uint8)
        if "src_index" in want: r["src_index"] = np.full(cap, FILL_INT, dtype=np.int32)
    return r


def finish(r):
    if r.get("agents") is not None:
        r["agents"] = np.ascontiguousarray(r["agents"]).view(AGENT).reshape(-1)
    if r.get("total") is not None:
        r["total"] = int(r["total"][0])
    return r


def device_inputs(c):
    t = {"states": _dev(np.asarray(c["states"], dtype=np.float64)), "t": None if c.get("t") is None else _dev(np.asarray(c["t"], dtype=np.float64))}
    for k in ("n_states", "ok", "pool_of", "owner"):
        t[k] = None if c.get(k) is None else _dev(np.asarray(c[k], dtype=np.int32))
    for s, src in enumerate(c["sources"]):
        if src is None:
            continue
        sfx = "" if s == 0 else "1"
        t["agents" + sfx] = _dev(src[0].view(np.uint8)) if len(src[0]) else None
        t["first" + sfx] = _dev(np.asarray(src[1], dtype=np.int32))
    return t


def run_device(e, c, ap, cap, want=KEYS):
    out = {k: _dev(v) for k, v in sentinels(c["states"].shape[0], cap, want).items()}
    e.agentsets_batch_device(device_inputs(c), out, ap)
    return finish({k: _host(v) for k, v in out.items()})


def run_host(e, c, ap, cap, want=KEYS):
    """The host entry on outputs that start as sentinels (Engine.agentsets_batch allocates zeros: the sentinel goes through the C entry directly)."""
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    a = {"states": np.ascontiguousarray(c["states"], dtype=np.float64), "t": None if c.get("t") is None else np.ascontiguousarray(c["t"], dtype=np.float64)}
    a.update({k: None if c.get(k) is None else np.ascontiguousarray(c[k], dtype=np.int32) for k in ("n_states", "ok", "pool_of", "owner")})
    held = [binding._agent_lists(s) for s in c["sources"] if s is not None]
    B, N = a["states"].shape[0], a["states"].shape[1]
    ai = abi.PoAgentsetsIn(B, N, p(a["states"]), p(a["n_states"]), p(a["ok"]), p(a["t"]))
    for s, h in enumerate(held):
        ai.src[s] = ctypes.pointer(h[0])
    ai.pool_of, ai.owner = p(a["pool_of"]), p(a["owner"])
    r = sentinels(B, cap, want)
    binding._check(binding.lib().po_agentsets_batch(e._h, ctypes.byref(ap), ctypes.byref(ai), ctypes.byref(abi.PoAgentsetsOut(cap, *[p(r.get(k)) for k in KEYS]))))
    return finish(r)


def both(e, ap, cap=None, tag="", **c):
    """Host entry, device entry and the reference: all three bitwise equal, outputs sentinel-filled.  cap None: three records more than the total, so that the
    slots behind first[B] show.  Returns the reference's dict."""
    if cap is None:
        cap = ref(ap, **c)["total"] + 3
    want = ref(ap, capacity=cap, **c)
    assert_same(run_host(e, c, ap, cap), want, tag=tag + " host")
    assert_same(run_device(e, c, ap, cap), want, tag=tag + " device")
    return want


POOLS = (0, 1, 31, 32, 33, 63, 64, 65, 129)  # around the wave size (the candidates are judged 64 at a time) and around the LDS chunk of the consumers


@pytest.mark.gpu
@pytest.mark.parametrize("P", POOLS)
def test_pool_sizes_lengths_and_batch_sizes(eng, P):
    kept = dropped = 0
    for N in (1, 2, 63, 64, 65, 130):
        for B in (1, 3, 65):
            c = make_scene(1000 * P + 10 * N + B, B, N, sizes0=(P, 5, P), sizes1=(3, P, 2))
            c["pool_of"][0] = 0
            r = both(eng, params_of(reach=4.0, t_before=0.5, owner_div=3), tag=f"P {P} N {N} B {B}", **c)
            kept += r["total"]
            dropped += sum(sum(len(s[0][s[1][k]:s[1][k + 1]]) for s in c["sources"]) for k in c["pool_of"][r["status"] > 0]) - r["total"]
    assert kept > 0 and dropped > 0


@pytest.mark.gpu
def test_position_independence(eng):
    """The same ego at different positions and in batches of different size gets the same records in the same order."""
    c = make_scene(31, 65, 65, sizes0=(70, 40), sizes1=(9, 20), ragged=False)
    owner_full = (np.arange(110) // 2).astype(np.int32)
    ap = params_of(reach=6.0, t_after=1.0)
    full = both(eng, ap, tag="B 65", owner=owner_full, **c)
    probe = int(np.argmax(full["count"]))
    lo, hi = full["first"][probe], full["first"][probe + 1]
    assert hi - lo >= 3 and (full["src_index"][lo:hi] >= 110).any() and (full["src_index"][lo:hi] < 110).any()
    for B, places in ((1, (0,)), (3, (0, 2)), (65, (0, 33, 64))):
        for at in places:
            idx = np.arange(B) % 65
            idx[at] = probe
            sub = dict(c, **{k: c[k][idx] for k in ("states", "t", "n_states", "pool_of")})
            sub["owner"] = np.where(owner_full == probe, at, -1).astype(np.int32)
            got = run_device(eng, sub, ap, 65 * 150)
            assert_same(got, ref(ap, capacity=65 * 150, **sub), tag=f"B {B} at {at}")
            glo, ghi = got["first"][at], got["first"][at + 1]
            assert same(got["agents"][glo:ghi], full["agents"][lo:hi]) and same(got["src_index"][glo:ghi], full["src_index"][lo:hi]), (B, at)


@pytest.mark.gpu
@pytest.mark.parametrize("B", (SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 2 * SCAN_CHUNK + 1))
def test_scan_chunk_boundary(eng, B):
    c = make_scene(50 + B % 7, B, 2, sizes0=(3, 3, 3, 3), sizes1=(3, 3, 3, 3), area=8.0)
    r = both(eng, params_of(reach=4.0, t_before=5.0, t_after=5.0, owner_div=0), tag=f"B {B}", **c)
    assert len(set(r["count"].tolist())) >= 3 and r["total"] > B  # the counts vary, and the running sum passes every chunk's end loaded


@pytest.mark.gpu
def test_clipping_by_capacity(eng):
    c = make_scene(61, 20, 40, sizes0=(30, 25), sizes1=(6, 6), ragged=False)
    ap = params_of(reach=8.0, t_before=1.0, t_after=1.0, owner_div=3)
    whole = ref(ap, **c)
    total, F = whole["total"], np.concatenate(([0], np.cumsum(whole["count"])))
    mid = int(np.flatnonzero(whole["count"] >= 2)[3])
    assert total > 40 and 0 < F[mid] and F[mid + 1] < total
    for cap in (0, total - 1, total, total + 5, int(F[mid]) + 1, int(F[mid])):
        r = both(eng, ap, cap=cap, tag=f"capacity {cap}", **c)
        assert r["total"] == total and same(r["first"], np.minimum(F, cap).astype(np.int32)) and same(r["count"], whole["count"])
        assert same(r["status"], np.where(F[1:] > cap, 2, 1).astype(np.int32))  # (every ego is composed here) status 2 exactly on the clipped sets
        n = min(cap, total)
        assert same(r["agents"][:n], whole["agents"][:n]) and same(r["src_index"][:n], whole["src_index"][:n])  # a clipped set is a prefix of the full one
        assert (r["agents"][n:].view(np.uint8) == FILL_BYTE).all() and (r["src_index"][n:] == FILL_INT).all()  # slots behind first[B] are not written
    got = eng.agentsets_batch(c["states"], c["t"], c["sources"], pool_of=c["pool_of"], params=ap)  # capacity None: a counting call, then one with room
    assert got["capacity"] == total
    assert_same(got, whole, tag="Engine.agentsets_batch")
    got = eng.agentsets_batch(c["states"], c["t"], c["sources"], pool_of=c["pool_of"], params=ap, capacity=int(F[mid]) + 1)
    assert got["total"] == total and got["status"][mid] == 2 and got["first"][-1] == F[mid] + 1


@pytest.mark.gpu
def test_every_filter(eng):
    c = make_scene(71, 33, 30, sizes0=(40, 26), sizes1=(7, 11))
    # owners: by the array (with values outside [0, B): nobody's), by owner_div, and none at all
    owner = np.random.default_rng(3).integers(-3, 40, 66).astype(np.int32)
    by_array = both(eng, params_of(reach=5.0, owner_div=2), tag="owner array", owner=owner, **c)
    by_div = both(eng, params_of(reach=5.0, owner_div=2), tag="owner_div 2", **c)
    nobody = both(eng, params_of(reach=5.0, owner_div=0), tag="owner_div 0", **c)
    for b in range(33):
        assert all(a >= 66 or owner[a] != b for a in by_array["kept"][b]) and all(a >= 66 or a // 2 != b for a in by_div["kept"][b])
    assert by_array["total"] < nobody["total"] and by_div["total"] < nobody["total"] and by_array["kept"] != by_div["kept"]
    # a source 1 that is NULL, has no pool, or has no record contributes nothing: the same sets as source 0 alone
    alone = dict(c, sources=c["sources"][:1])
    want = both(eng, params_of(reach=5.0, owner_div=2), tag="source 0 alone", **alone)
    assert 0 < want["total"] < by_div["total"] and (want["src_index"][:want["total"]] < 66).all()
    for tag, src1 in (("S = 0", (c["sources"][1][0], np.array([0], dtype=np.int32))), ("n_agents = 0", (np.zeros(0, dtype=AGENT), np.array([0, 0, 0], dtype=np.int32)))):
        got = both(eng, params_of(reach=5.0, owner_div=2), tag=tag, **dict(c, sources=[c["sources"][0], src1]))
        assert_same(got, want, tag=tag)
    # time and space each drop something of their own
    wide = both(eng, params_of(reach=200.0, owner_div=0), tag="reach 200", **c)
    long = both(eng, params_of(reach=5.0, t_before=100.0, t_after=100.0, owner_div=0), tag="windows of 100 s", **c)
    assert nobody["total"] < wide["total"] and nobody["total"] < long["total"]
    no_t = both(eng, params_of(reach=5.0, win_lo=2.0, win_hi=2.5, owner_div=0), tag="t NULL", **dict(c, t=None))
    assert 0 < no_t["total"] and no_t["kept"] != nobody["kept"]


@pytest.mark.gpu
def test_lists_nobody_validated_are_read_clamped(eng):
    """Through the device entry only (the host entry refuses such lists): records that cover nothing in every way, shuffled times, pool_of outside the pools, a
    first table that is out of range and decreasing."""
    c = make_scene(81, 40, 20, sizes0=(50, 30), sizes1=(20, 12), valid=False)
    c["pool_of"][:6] = [-1, 2, 99, -2 ** 31, 2 ** 31 - 1, 1]
    ap = params_of(reach=6.0, t_before=1.0, owner_div=2)
    for tag, f0, f1 in (("bad records", None, None), ("first out of range", [-5, 40, 2 ** 31 - 1], [3, 2 ** 30, 12]), ("first decreasing", [60, 20, 0], [0, 32, 5])):
        if f0 is not None:
            c["sources"] = [(c["sources"][0][0], np.array(f0, dtype=np.int32)), (c["sources"][1][0], np.array(f1, dtype=np.int32))]
        want = ref(ap, **c)
        assert_same(run_device(eng, c, ap, want["total"] + 2), ref(ap, capacity=want["total"] + 2, **c), tag=tag)
        assert want["total"] > 0
    rec = c["sources"][0][0]
    covers_nothing = [a for a in range(80) if dynamic_ref.covers(rec[a]) == 0]
    want = ref(ap, **dict(c, sources=[(rec, np.array([0, 50, 80], dtype=np.int32)), c["sources"][1]]))
    assert len(covers_nothing) >= 8 and not set(covers_nothing) & {a for k in want["kept"] for a in k}
    with pytest.raises(binding.PoError):  # the host entry reads the lists and refuses them
        eng.agentsets_batch(c["states"], c["t"], [(rec, np.array([0, 50, 80], dtype=np.int32))], params=ap)
    with pytest.raises(binding.PoError):
        eng.agentsets_batch(c["states"], c["t"], [make_scene(1, 2, 2)["sources"][0]], pool_of=np.full(40, 1), params=ap)


@pytest.mark.gpu
def test_not_composed_egos_between_composed_ones(eng):
    c = make_scene(91, 12, 10, sizes0=(30,), sizes1=(6,), ragged=False)
    c["ok"] = np.ones(12, dtype=np.int32); c["ok"][2] = 0
    c["n_states"][4] = 0; c["n_states"][5] = -7
    c["states"][7, 9, 0] = np.nan; c["states"][8, 0, 1] = -np.inf; c["t"][10, 3] = np.inf
    c["states"][1, 9, 0] = np.nan; c["n_states"][1] = 9  # a bad value behind n is not read
    c["states"][3, 5, 2:] = np.nan  # heading, curvature and s are not read
    r = both(eng, params_of(reach=30.0, t_before=9.0, t_after=9.0), tag="not composed", **c)
    bad = [2, 4, 5, 7, 8, 10]
    assert np.flatnonzero(r["status"] == 0).tolist() == bad and (r["count"][bad] == 0).all() and (r["first"][1:][bad] == r["first"][:-1][bad]).all()
    assert (np.delete(r["count"], bad) > 0).all()
    r = both(eng, params_of(reach=30.0), tag="t NULL: a bad t is not read", **dict(c, t=None))
    assert np.flatnonzero(r["status"] == 0).tolist() == [2, 4, 5, 7, 8]


@pytest.mark.gpu
def test_optional_arguments_and_empty_calls(eng):
    import torch

    c = make_scene(95, 70, 33, sizes0=(60, 30), sizes1=(9, 9))
    ap = params_of(reach=6.0, owner_div=1)
    want = ref(ap, **c)
    cap = want["total"]
    for drop in ("set_of", "src_index", "total"):  # every optional output NULL in turn
        keys = tuple(k for k in KEYS if k != drop)
        assert_same(run_device(eng, c, ap, cap, want=keys), want, keys=keys, tag="device without " + drop)
        assert_same(run_host(eng, c, ap, cap, want=keys), want, keys=keys, tag="host without " + drop)
    for drop in ("n_states", "ok", "pool_of", "t"):  # every optional input NULL in turn
        both(eng, ap, tag="no " + drop, **{k: v for k, v in c.items() if k != drop})
    # B = 0: PO_OK from both entries, nothing is written: the outputs keep their sentinels
    L = binding.lib()
    out = {k: _dev(v) for k, v in sentinels(2, 4).items()}
    p = lambda d, k: ctypes.c_void_p(d[k].data_ptr())
    for entry in (L.po_agentsets_batch, L.po_agentsets_batch_device):
        ai = abi.PoAgentsetsIn(); ai.N = 5
        ao = abi.PoAgentsetsOut(4, *[p(out, k) for k in KEYS]) if entry is L.po_agentsets_batch_device else abi.PoAgentsetsOut()
        assert entry(eng._h, ctypes.byref(ap), ctypes.byref(ai), ctypes.byref(ao)) == abi.PO_OK
    torch.cuda.synchronize()
    for k, v in sentinels(2, 4).items():
        assert same(_host(out[k]), v), k
    t = device_inputs(c)
    with pytest.raises(binding.PoError):  # out->agents is the fleet's own array
        eng.agentsets_batch_device(t, dict({k: _dev(v) for k, v in sentinels(70, 4).items()}, agents=t["agents"]), ap)
    for f, v in bad_params():
        with pytest.raises(binding.PoError):
            eng.agentsets_batch(c["states"], c["t"], c["sources"], params=params_of(**{f: v}))


def fleet_case():
    """Two worlds of three vehicles, 64 states 0.5 m apart: A along +x from the origin and B along +y from (20, -20) cross at (20, 0) after the same distance; C
    drives along +x sixty metres north of them towards a disc that stands on its path.  The second world is the first one 7 m further east."""
    N = 64
    s = 0.5 * np.arange(N)
    states = np.zeros((6, N, 5))
    for w in range(2):
        a, b, c = states[3 * w], states[3 * w + 1], states[3 * w + 2]
        a[:, 0] = 7.0 * w + s
        b[:, 0] = 7.0 * w + 20.0; b[:, 1] = -20.0 + s; b[:, 2] = 0.5 * math.pi
        c[:, 0] = 7.0 * w + s; c[:, 1] = 60.0
    states[:, :, 4] = s
    seen = binding.pack_agents([[(0.5, BEFORE | AFTER, [(0.0, 7.0 * w + 25.0, 60.0)])] for w in range(2)])
    return states, seen


DYN_KEYS = {"status": np.int32, "ok_out": np.int32, "gap_min": np.float64, "first_state": np.int32, "first_agent": np.int32, "stop_state": np.int32,
            "first_time": np.float64, "gap": np.float64, "v_limit": np.float64}
TRAJ_TYPES = {"status": (np.int32, ()), "states": (np.float64, (64, 5)), "v": (np.float64, (64,)), "a": (np.float64, (64,)), "t": (np.float64, (64,)),
              "index": (np.int32, (64,)), "first_held": (np.int32, ())}


@pytest.mark.gpu
def test_chain_fleet_plans_as_agent_sets_on_one_stream(eng, oracle):
    """speed -> trajectory (D = 4) -> agent sets (owner_div = 4, pool_of = the world, one perception agent per world as source 1) -> po_dynamic_batch_device on
    out->agents, out->first and out->set_of.  Device entries only, no synchronisation and no host copy between the four calls; every stage equals its reference
    on the device output of the stage before it, bit for bit."""
    op = oracle.default_params()
    states, (seen, seen_first) = fleet_case()
    B, N, K, D = 6, 64, 64, 4
    off, rad = binding.covering_discs(binding.default_params())
    tp = binding.default_trajectory_params()
    tp.dt, tp.K, tp.n_discs, tp.agent_pts, tp.agent_stride, tp.agent_flags = 0.125, K, D, 8, 9, AFTER
    for d in range(D):
        tp.disc_offset[d], tp.disc_radius[d] = off[d], rad
    spd, dp = binding.default_speed_params(), binding.default_dynamic_params()
    ap = params_of(reach=binding.footprint_reach(op, dp.margin), owner_div=D)
    cap = B * (2 * D + 1) + 2  # every other vehicle of the world and its perception agent, and two slots nobody writes
    d_states, v0 = _dev(states), _dev(np.full(B, 4.0))
    sp_out = {"v": _dev(np.full((B, N), 7.0)), "a": _dev(np.full((B, N), 7.0)), "t": _dev(np.full((B, N), 7.0)), "total_time": _dev(np.full(B, 7.0)),
              "status": _dev(np.full(B, FILL_INT, dtype=np.int32))}
    tr = {k: _dev(np.full((B,) + shape, FILL_INT if ty == np.int32 else 7.0, dtype=ty)) for k, (ty, shape) in TRAJ_TYPES.items()}
    tr["agents"] = _dev(np.full(B * D * 208, FILL_BYTE, dtype=np.uint8))
    sets = {k: _dev(v) for k, v in sentinels(B, cap).items()}
    dyn = {k: _dev(np.full((B, N) if k in ("gap", "v_limit") else (B,), FILL_INT if ty == np.int32 else 7.0, dtype=ty)) for k, ty in DYN_KEYS.items()}
    fleet_first, pool_of = np.array([0, 3 * D, 6 * D], dtype=np.int32), np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    lists = {"first": _dev(fleet_first), "pool_of": _dev(pool_of), "agents1": _dev(seen.view(np.uint8)), "first1": _dev(seen_first)}
    eng.speed_batch_device({"states": d_states, "v0": v0}, sp_out, spd)
    eng.trajectory_batch_device({"states": d_states, "v": sp_out["v"], "t": sp_out["t"]}, tr, tp)
    eng.agentsets_batch_device(dict(lists, states=d_states, t=sp_out["t"], agents=tr["agents"]), sets, ap)
    eng.dynamic_batch_device({"states": d_states, "t": sp_out["t"], "agents": sets["agents"], "first": sets["first"], "set_of": sets["set_of"]}, dyn, dp)
    got_sp = {k: _host(v) for k, v in sp_out.items()}
    got_tr = {k: _host(v) for k, v in tr.items()}
    got_tr["agents"] = got_tr["agents"].view(AGENT).reshape(-1)
    got_sets, got_dyn = finish({k: _host(v) for k, v in sets.items()}), {k: _host(v) for k, v in dyn.items()}
    want_sp = speed_ref.profile(op, states, np.full(B, 4.0), spd)
    for k in ("v", "a", "t", "total_time", "status"):
        assert same(got_sp[k], want_sp[k]), ("speed", k)
    want_tr = trajectory_ref.trajectory(states, got_sp["v"], got_sp["t"], tp)
    for k in list(TRAJ_TYPES) + ["agents"]:
        assert same(got_tr[k], want_tr[k]), ("trajectory", k)
    c = dict(states=states, t=got_sp["t"], pool_of=pool_of, sources=[(got_tr["agents"], fleet_first), (seen, seen_first)])
    want_sets = ref(ap, capacity=cap, **c)
    assert_same(got_sets, want_sets, tag="agent sets on the stream")
    want_dyn = dynamic_ref.check(op, states, got_sp["t"], got_sets["agents"], got_sets["first"], dp, set_of=got_sets["set_of"])
    for k in DYN_KEYS:
        assert same(got_dyn[k], want_dyn[k]), ("dynamic on the composed sets", k)
    # no ego's set holds one of its own records, nor one of the other world
    first, idx = got_sets["first"], got_sets["src_index"]
    for b in range(B):
        mine = idx[first[b]:first[b + 1]]
        fleet = mine[mine < B * D]
        assert (fleet // D != b).all() and (fleet // (3 * D) == b // 3).all() and ((mine[mine >= B * D] - B * D) == b // 3).all(), b
    assert (got_sets["status"] == 1).all() and got_sets["total"] < B * (2 * D + 1)  # something was dropped: C is sixty metres from A and B
    # the crossing vehicles report each other, C reports the disc on its path: through src_index
    assert (got_dyn["status"] >= 2).all()
    who = idx[got_dyn["first_agent"]]
    for w in range(2):
        assert who[3 * w] // D == 3 * w + 1 and who[3 * w + 1] // D == 3 * w and who[3 * w + 2] == B * D + w, (w, who)


@pytest.mark.gpu
def test_reuse_and_host_mirror_program(eng):
    """Two runs on a reused handle are bitwise equal, and AgentSets::compose end to end in its own process prints what the reference computes."""
    c, ap = mirror_case()
    want = both(eng, ap, tag="mirror case", **c)
    again = run_device(eng, c, ap, want["capacity"])
    assert_same(again, run_device(eng, c, ap, want["capacity"]), tag="second run on the same handle")
    assert_same(again, want, tag="reused handle")
    got = eng.agentsets_batch(c["states"], c["t"], c["sources"], pool_of=c["pool_of"], params=ap, n_states=c["n_states"], ok=c["ok"])
    assert_same(got, ref(ap, **c), tag="Engine.agentsets_batch")
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "agentsets_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "agentsets_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "agentsets_test passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]
    printed = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("status", "count", "first", "src_index", "checksum")}
    exact = ref(ap, **c)
    assert printed["status"] == exact["status"].tolist() and printed["count"] == exact["count"].tolist() and printed["first"] == exact["first"].tolist()
    assert printed["src_index"] == exact["src_index"].tolist()
    ag = exact["agents"]
    total = sum(int(ag[f].view(np.uint64).sum(dtype=np.uint64)) for f in ("t", "x", "y", "radius")) + int(ag["n_pts"].sum()) + int(ag["flags"].sum())
    assert printed["checksum"] == [total & 0xffffffffffffffff]
