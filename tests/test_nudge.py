"""The corridor nudge: po_nudge_batch* (csrc/po_nudge.hip; include/po_hip.h states the definition).

Every hull, touch, side and carved bound is a fixed sequence of rounded IEEE double operations and comparisons, so every comparison with the device here is BIT
equality on byte views against tests/nudge_ref.py (numpy, one ufunc per operation).  The closed scenes sit on a dyadic grid: heading 0 (pcos and psin are exactly
1 and 0), car_length 6, car_width 2 and safety_margin 0 (rad is exactly 1.25), d, radii, margins and positions in multiples of 1 / 8.  Two tolerances appear in
this file and nowhere near the device: the hull property's delta, derived beside it, and the solver tolerance of tests/test_gpu_parity.py, imported.

CPU: the reference against a scalar loop over the definition, the hull property against brute force, the closed scenes (left, right, ties, hints, min_width at
equality, a blocking agent, two agents whose order matters, a crosser out of every window, skip_states, hi == Wl and one ulp beyond), every status-0 trigger, the
closure nudge -> KP solve -> dynamic on the references, exports and the ABI mirror, argument checks without a device, the kernel's constants, the host mirror
compiles and links.  GPU: lane-ownership boundaries of 4 N pairs with ragged n, agent counts around the LDS chunk, batch sizes and position in the batch, sets,
every kind of piece with boundaries on the window ends, W below, at and above the set size, the closed scenes, NULL optional pointers, empty calls, lists read
clamped, the chain bounds -> nudge -> solve -> speed -> dynamic on one stream, the C++ mirror's program against the Python call."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import dynamic_ref
import nudge_ref
import select_ref
import speed_ref
from path_optimizer_amd import abi, binding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["po_default_nudge_params", "po_nudge_batch", "po_nudge_batch_device"]
KEYS = ("status", "ok_out", "bounds", "side", "first_blocked_state", "first_blocked_agent", "width_min")
DBL_MAX = select_ref.DBL_MAX
BEFORE, AFTER = abi.PO_AGENT_HOLD_BEFORE, abi.PO_AGENT_HOLD_AFTER
NDG_CHUNK, NDG_TRIG = 32, 384  # kAgentChunk of po_agents.hpp, kNdgTrig of po_nudge.hip: agents per LDS chunk, states whose cos / sin are kept in LDS
GRID_D = (-0.75, 0.75, 2.25, 3.75)


def test_boundary_cases_follow_the_kernel_constants():
    """The agent counts and the long path below are built from NDG_CHUNK and NDG_TRIG: they must be the kernel's own constants."""
    src = open(os.path.join(ROOT, "path_optimizer_amd", "csrc", "po_nudge.hip")).read()
    agents = open(os.path.join(ROOT, "path_optimizer_amd", "csrc", "po_agents.hpp")).read()
    assert int(re.search(r"constexpr int kAgentChunk = (\d+);", agents).group(1)) == NDG_CHUNK
    assert int(re.search(r"constexpr int kNdgTrig = (\d+);", src).group(1)) == NDG_TRIG


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
    p = binding.default_nudge_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def grid(p):
    """The vehicle of the closed scenes on a parameter struct (the oracle's or the engine's: the same layout): rad = sqrt(0.75^2 + 1) + 0 = 1.25 exactly."""
    p.car_length, p.car_width, p.safety_margin = 6.0, 2.0, 0.0
    for j, v in enumerate(GRID_D):
        p.d[j] = v
    return p


def disc(x, y, r, flags=BEFORE | AFTER, t=0.0):
    return (r, flags, [(t, x, y)])


def ref(params, npar=None, **c):
    c = dict(c)
    agents, first = binding.pack_agents(c.pop("agents"))
    return nudge_ref.nudge(params, c.pop("ref_x"), c.pop("ref_y"), c.pop("ref_z"), c.pop("t"), c.pop("bounds"), agents, first, npar or params_of(), **c)


def make_lines(seed, B, N, ds=0.3, box=4.0):
    """B smooth reference lines of N states around the origin with their times (about 3 m/s) and corridors of 2 .. 6 m: ref_x, ref_y, ref_z, t [B, N],
    bounds [B, N, 4, 2]."""
    rng = np.random.default_rng([31, seed])
    x, y, z, t = (np.zeros((B, N)) for _ in range(4))
    for b in range(B):
        step = ds * rng.uniform(0.7, 1.3, max(N - 1, 0))
        s = np.concatenate(([0.0], np.cumsum(step)))
        k = rng.uniform(0, 0.15) * np.sin(s / rng.uniform(3, 9) + rng.uniform(0, 6.28))
        z[b] = rng.uniform(-math.pi, math.pi) + np.concatenate(([0.0], np.cumsum(0.5 * (k[1:] + k[:-1]) * step)))
        x[b] = rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(np.cos(z[b, :-1]) * step)))
        y[b] = rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(np.sin(z[b, :-1]) * step)))
        t[b] = rng.uniform(0, 1) + s / rng.uniform(2, 4)
    bounds = np.stack([-rng.uniform(1, 3, (B, N, 4)), rng.uniform(1, 3, (B, N, 4))], axis=-1)
    return x, y, z, t, bounds


def random_agents(rng, count, box=8.0, horizon=6.0):
    """Agents with 1 .. 8 points, every flag combination, radii 0.1 .. 0.6, walking about the box within the horizon."""
    out = []
    for _ in range(count):
        npts = int(rng.integers(1, 9))
        tt = rng.uniform(-1.0, horizon / 2) + np.concatenate(([0.0], np.cumsum(rng.uniform(0.1, horizon / 8, npts - 1))))
        x = rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(rng.uniform(-2, 2, npts - 1))))
        y = rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(rng.uniform(-2, 2, npts - 1))))
        out.append((rng.uniform(0.1, 0.6), int(rng.integers(0, 4)), list(zip(tt, x, y))))
    return out


def random_case(seed, B, N, per_set=(5, 0, 9), ragged=True, W=None, hints=True):
    """Ragged lines, S sets of agents, a set per line, and (hints) a side_prev with every value a caller can leave there."""
    rng = np.random.default_rng([32, seed])
    x, y, z, t, bounds = make_lines(seed, B, N)
    n = rng.integers(0, N + 1, B).astype(np.int32) if ragged else np.full(B, N, dtype=np.int32)
    n[rng.integers(0, B)] = N
    W = max(1, max(per_set)) if W is None else W
    c = dict(ref_x=x, ref_y=y, ref_z=z, t=t, bounds=bounds, n_points=n, agents=binding.pack_agents([random_agents(rng, k) for k in per_set]),
             set_of=rng.integers(0, len(per_set), B).astype(np.int32), W=W)
    if hints and W > 0:
        c["side_prev"] = rng.integers(-1, 3, (B, W)).astype(np.int32)
    return c


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def _scalar_nudge(params, x, y, z, t, bnd, n, okb, agents, first, ks, prev, W, npar):
    """The definition as a plain scalar Python loop over ONE path (Python floats are IEEE doubles; every operation rounds once).  bnd [N, 4, 2]."""
    N = len(x)
    margin, t_before, t_after, min_width, skip = float(npar.margin), float(npar.t_before), float(npar.t_after), float(npar.min_width), int(npar.skip_states)
    n = min(max(int(n), 0), N)
    out = dict(status=0, ok_out=0, bounds=[[[float(v) for v in pair] for pair in row] for row in bnd], side=[0] * W, first_blocked_state=-1,
               first_blocked_agent=-1, width_min=DBL_MAX)
    fin = lambda v: abs(v) <= DBL_MAX
    mn = lambda a, b: b if b < a else a
    mx = lambda a, b: b if b > a else a
    x, y, z, t = ([float(v) for v in arr[:n]] for arr in (x, y, z, t))
    Wb = out["bounds"]
    if okb == 0 or n < 1 or not all(fin(v) for v in x + y + z + t) or not all(fin(v) for row in Wb[:n] for pair in row for v in pair):
        return out
    T = select_ref.trig_lib()
    L, Wd = float(params.car_length), float(params.car_width)
    rad = math.sqrt((L / 8) * (L / 8) + (Wd / 2) * (Wd / 2)) + float(params.safety_margin)
    d = [float(params.d[j]) for j in range(4)]
    cl = lambda v, hi: min(max(int(v), 0), hi)
    ks = cl(ks, len(first) - 2)
    lo_a, hi_a = cl(first[ks], len(agents)), cl(first[ks + 1], len(agents))
    carved = False
    for a in range(lo_a, hi_a):
        ag, e = agents[a], a - lo_a
        npts, R, flags = int(ag["n_pts"]), float(ag["radius"]), int(ag["flags"])
        if npts < 1 or npts > 8 or not R >= 0:
            continue
        AT, AX, AY = ([float(v) for v in ag[f][:npts]] for f in ("t", "x", "y"))
        if not all(fin(v) for v in AT + AX + AY):
            continue
        rho = (rad + R) + margin
        hull, touched = {}, []
        for i in range(n):
            cz, sz = T.po_oracle_pcos(z[i]), T.po_oracle_psin(z[i])
            w0, w1 = t[i] - t_before, t[i] + t_after
            for j in range(4):
                cx, cy = x[i] + d[j] * cz, y[i] + d[j] * sz
                lo, hi = DBL_MAX, -DBL_MAX
                for p in ([-1] if flags & 1 else []) + list(range(npts - 1)) + ([npts - 1] if flags & 2 else []):
                    if p < 0:
                        ta, tb = w0, mn(w1, AT[0])
                        pa = pb = (AX[0], AY[0])
                    elif p == npts - 1:
                        ta, tb = mx(w0, AT[p]), w1
                        pa = pb = (AX[p], AY[p])
                    else:
                        D = AT[p + 1] - AT[p]
                        if not D > 0:
                            continue
                        ta, tb = mx(w0, AT[p]), mn(w1, AT[p + 1])
                        wa, wb = (ta - AT[p]) / D, (tb - AT[p]) / D
                        pa = (AX[p] + wa * (AX[p + 1] - AX[p]), AY[p] + wa * (AY[p + 1] - AY[p]))
                        pb = (AX[p] + wb * (AX[p + 1] - AX[p]), AY[p] + wb * (AY[p + 1] - AY[p]))
                    if not ta <= tb:
                        continue
                    ends = []
                    for X, Y in (pa, pb):
                        dx, dy = X - cx, Y - cy
                        ends.append((dx * cz + dy * sz, (-dx) * sz + dy * cz))
                    cands = []
                    for u_, l_ in ends:
                        q = rho * rho - u_ * u_
                        if q >= 0:
                            w = math.sqrt(q)
                            cands += [l_ - w, l_ + w]
                    (ua, la), (ub, lb) = ends
                    du, dl = ub - ua, lb - la
                    L2 = du * du + dl * dl
                    if L2 > 0 and du != 0:
                        ln = math.sqrt(L2)
                        ox, oy = (rho * dl) / ln, (rho * du) / ln
                        tp = (ox - ua) / du
                        if 0 <= tp <= 1:
                            cands.append((la + oy) + tp * dl)
                        tm = (0.0 - (ox + ua)) / du
                        if 0 <= tm <= 1:
                            cands.append((la - oy) + tm * dl)
                    for c in cands:
                        lo, hi = mn(lo, c), mx(hi, c)
                hull[(i, j)] = (lo, hi)
                if i >= skip and lo <= hi and hi > Wb[i][j][0] and lo < Wb[i][j][1]:
                    touched.append((i, j))
        if not touched:
            continue
        rl = min(Wb[i][j][1] - hull[(i, j)][1] for i, j in touched)
        rr = min(hull[(i, j)][0] - Wb[i][j][0] for i, j in touched)
        left, right = rl >= min_width, rr >= min_width
        sp = int(prev[e]) if prev is not None and e < W else 0
        if sp == 1 and left:
            side = 1
        elif sp == -1 and right:
            side = -1
        elif left and right:
            side = 1 if rl >= rr else -1
        elif left or right:
            side = 1 if left else -1
        else:
            side = 2
            if out["first_blocked_agent"] < 0:
                out["first_blocked_agent"], out["first_blocked_state"] = a, min(i for i, _ in touched)
        if e < W:
            out["side"][e] = side
        for i, j in touched if side != 2 else []:
            carved = True
            if side == 1:
                Wb[i][j][0] = hull[(i, j)][1]
            else:
                Wb[i][j][1] = hull[(i, j)][0]
    widths = [Wb[i][j][1] - Wb[i][j][0] for i in range(n) for j in range(4)]
    out["width_min"] = min(0.0 if w == 0 else w for w in widths)
    out["status"] = 3 if out["first_blocked_agent"] >= 0 else (2 if carved else 1)
    out["ok_out"] = 1 if out["status"] != 3 else 0
    return out


def test_reference_agrees_with_a_scalar_loop_over_the_definition(oracle):
    params = oracle.default_params()
    seen, sides = set(), set()
    for case, (B, N, npar) in enumerate([(8, 17, params_of()), (6, 25, params_of(margin=0.0, t_before=0.25, t_after=2.0, min_width=0.6, skip_states=3)),
                                         (6, 9, params_of(margin=-0.1, t_before=0.0, t_after=0.0, min_width=0.0))]):
        c = random_case(case, B, N, W=6)
        ok = np.ones(B, dtype=np.int32); ok[3] = 0
        agents, first = c["agents"]
        agents[1]["x"][0] = np.nan  # covers nothing
        c["bounds"][2, N - 1, 1, 0] = np.nan  # beyond n unless the path is full: copied through or a trigger of 'not processed'
        got = nudge_ref.nudge(params, c["ref_x"], c["ref_y"], c["ref_z"], c["t"], c["bounds"], agents, first, npar, n_points=c["n_points"], ok=ok,
                              set_of=c["set_of"], side_prev=c["side_prev"], W=6)
        for b in range(B):
            want = _scalar_nudge(params, c["ref_x"][b], c["ref_y"][b], c["ref_z"][b], c["t"][b], c["bounds"][b], c["n_points"][b], ok[b], agents, first,
                                 c["set_of"][b], c["side_prev"][b], 6, npar)
            for key in KEYS:
                assert same(got[key][b], np.array(want[key], dtype=got[key].dtype)), (case, b, key, got[key][b], want[key])
        seen |= set(got["status"].tolist())
        sides |= set(got["side"].reshape(-1).tolist())
    assert seen == {0, 1, 2, 3} and sides == {-1, 0, 1, 2}


# The hull property.  Segments with both ends on the grid of 1 / 8 in [-16, 16]^2 (the pair's frame), rho a multiple of 1 / 8 in [1 / 2, 4], so every |coordinate| < 64.
# DELTA, the slack either side of lo and hi: the only ill-conditioned step of the formulas is w = sqrt(q) near q = 0.  q = rho * rho - u * u carries at most three
# roundings of values below 64^2 = 2^12, so |q - q_exact| < 3 * 2^-53 * 2^12 < 2^-39, and a square root moves by at most sqrt of that when q is near 0:
# |w - w_exact| < 2^-19.5.  The side candidates are well conditioned on this grid: du is 0 (then they are not taken) or |du| >= 1 / 8, so tp and tm carry an error
# below 2^-45 / (1 / 8) = 2^-42 and the candidate, times |dl| <= 32, below 2^-37.  DELTA = 2^-17 covers both with room.  The brute-force distance below is exact to
# 2^-45 or so on these magnitudes, while a position DELTA inside (outside) the true interval is nearer (farther) than rho by at least DELTA^2 / (2 * 4) = 2^-37
# at a disc end and DELTA * |du| / len >= 2^-17 * 2^-3 / 46 > 2^-26 at a side, so the comparisons with rho need no slack of their own.
DELTA = 2.0 ** -17


def _dist_to_segment(l, ua, la, ub, lb):
    """The distance of (0, l) from the segment (ua, la) - (ub, lb), the plain way."""
    du, dl = ub - ua, lb - la
    L2 = du * du + dl * dl
    s = 0.0 if L2 == 0 else min(1.0, max(0.0, ((0.0 - ua) * du + (l - la) * dl) / L2))
    return math.hypot(ua + s * du, la + s * dl - l)


def test_hull_is_the_interval_within_rho_of_the_segment():
    rng = np.random.default_rng(3101)
    g = lambda n: rng.integers(-128, 129, n) / 8.0
    n = 400
    ua, la, ub, lb, rho = g(n), g(n), g(n), g(n), rng.integers(4, 33, n) / 8.0
    ub[:60] = ua[:60]                      # du == 0
    lb[40:80] = la[40:80]; ub[40:80] = ua[40:80]  # a zero-length piece
    ua[70:110] = rho[70:110] * np.where(rng.random(40) < 0.5, 1, -1)  # |ua| == rho exactly (with du == 0, a zero length, or a general second end)
    ub[70:80] = ua[70:80]
    near = slice(110, 250)                 # the rest of the forced cases: segments that do come near the line u = 0
    ua[near] = rng.integers(-24, 25, 140) / 8.0
    lo, hi = nudge_ref.hull_piece(ua, la, ub, lb, rho, np.ones(n, dtype=bool), np.full(n, DBL_MAX), np.full(n, -DBL_MAX))
    hit = 0
    for k in range(n):
        seg = (ua[k], la[k], ub[k], lb[k])
        if lo[k] > hi[k]:  # no candidate: no lateral position comes within rho (the nearest ones lie beside the two ends and between them)
            for l in list(np.linspace(min(la[k], lb[k]) - 5, max(la[k], lb[k]) + 5, 41)) + [la[k], lb[k]]:
                assert _dist_to_segment(l, *seg) > rho[k], (k, l)
            continue
        hit += 1
        for l in (lo[k] - DELTA, hi[k] + DELTA, lo[k] - 1.0, hi[k] + 1.0, lo[k] - 40.0, hi[k] + 40.0):
            assert _dist_to_segment(l, *seg) > rho[k], (k, l, lo[k], hi[k])
        if lo[k] + DELTA <= hi[k] - DELTA:
            for l in [lo[k] + DELTA, hi[k] - DELTA] + list(np.linspace(lo[k] + DELTA, hi[k] - DELTA, 9)):
                assert _dist_to_segment(l, *seg) <= rho[k], (k, l, lo[k], hi[k])
    assert hit > 150
    # |ua| == rho with nothing else near: the hull is the one point la
    lo, hi = nudge_ref.hull_piece(np.array([2.0]), np.array([0.5]), np.array([2.0]), np.array([0.5]), np.float64(2.0), np.ones(1, dtype=bool),
                                  np.array([DBL_MAX]), np.array([-DBL_MAX]))
    assert lo[0] == 0.5 and hi[0] == 0.5


# The closed scenes: a reference line of 41 states 0.5 m apart along +x (heading 0), the vehicle there at 4 m/s (t = x / 4), a corridor of 6 m for the circle
# centres (lb = -3, ub = 3), the grid vehicle (rad = 1.25, d = -0.75, 0.75, 2.25, 3.75), agents at x = 10.25, so that the longitudinal coordinate of an agent on
# pair (i, j), 10.25 - 0.5 i - d_j, is a multiple of 0.5 and is 0 on some pairs.  margin 0.25: an agent of radius 0.5 has rho = (1.25 + 0.5) + 0.25 = 2 exactly.
AX = 10.25


def scene(n=41, N=None, lb=-3.0, ub=3.0):
    N = N or n
    x = np.zeros((1, N)); x[0, :n] = 0.5 * np.arange(n)
    bounds = np.zeros((1, N, 4, 2)); bounds[..., 0] = lb; bounds[..., 1] = ub
    return dict(ref_x=x, ref_y=np.zeros((1, N)), ref_z=np.zeros((1, N)), t=x / 4.0, bounds=bounds)


def closed(oracle, sets, npar=None, **kw):
    c = scene()
    c.update(kw)
    return ref(grid(oracle.default_params()), npar or params_of(margin=0.25), agents=sets, **c)


def pairs_within(rho, n=41):
    """{(i, j): ua} of the pairs whose circle centre is longitudinally within rho of x = 10.25."""
    return {(i, j): AX - 0.5 * i - d for i in range(n) for j, d in enumerate(GRID_D) if abs(AX - 0.5 * i - d) <= rho}


def test_closed_scene_a_held_agent_beside_the_reference(oracle):
    """A disc of 0.5 m held 2 m right of the line: the vehicle passes LEFT of it, and exactly the pairs within rho = 2 get lb = -2 + sqrt(4 - ua^2)."""
    r = closed(oracle, [[disc(AX, -2.0, 0.5)]])
    want = np.zeros((41, 4, 2)); want[..., 0] = -3.0; want[..., 1] = 3.0
    near = pairs_within(2.0)
    assert len(near) == 4 * 9 and min(i for i, _ in near) == 9 and max(i for i, _ in near) == 26
    for (i, j), ua in near.items():
        want[i, j, 0] = -2.0 + math.sqrt(4.0 - ua * ua)
    assert same(r["bounds"][0], want)
    assert want[19, 1, 0] == 0.0 and want[15, 1, 0] == -2.0  # ua = 0: the hull ends at -2 + 2; |ua| == rho exactly: at -2 + 0
    assert r["side"].tolist() == [[1]] and r["status"][0] == 2 and r["ok_out"][0] == 1 and r["width_min"][0] == 3.0
    assert r["first_blocked_state"][0] == -1 and r["first_blocked_agent"][0] == -1
    # the mirrored scene: RIGHT of it, ub = 2 - sqrt(4 - ua^2)
    m = closed(oracle, [[disc(AX, 2.0, 0.5)]])
    mirrored = want[..., ::-1] * -1.0
    assert same(m["bounds"][0], mirrored + 0.0) and m["side"].tolist() == [[-1]] and m["status"][0] == 2 and m["width_min"][0] == 3.0


def test_closed_scene_ties_hints_and_min_width(oracle):
    """A disc on the line itself: lo = -2, hi = 2 where ua = 0, so rl = 3 - 2 = 1 = rr = -2 + 3."""
    centre = [[disc(AX, 0.0, 0.5)]]
    assert closed(oracle, centre)["side"].tolist() == [[1]]  # rl == rr: left
    prev = lambda v: np.array([[v]], dtype=np.int32)
    assert closed(oracle, centre, side_prev=prev(-1))["side"].tolist() == [[-1]]  # the hint flips the tie
    assert closed(oracle, centre, side_prev=prev(1))["side"].tolist() == [[1]]
    for v in (0, 2, 7, -3):  # no hint
        assert closed(oracle, centre, side_prev=prev(v))["side"].tolist() == [[1]]
    assert closed(oracle, [[disc(AX, -2.0, 0.5)]], side_prev=prev(-1))["side"].tolist() == [[1]]  # a hint whose side is not passable is ignored
    assert closed(oracle, [[disc(AX, 2.0, 0.5)]], side_prev=prev(1))["side"].tolist() == [[-1]]
    r = closed(oracle, centre, params_of(margin=0.25, min_width=1.0))  # min_width met with equality passes
    assert r["side"].tolist() == [[1]] and r["status"][0] == 2 and r["width_min"][0] == 1.0
    r = closed(oracle, centre, params_of(margin=0.25, min_width=float(np.nextafter(1.0, 2.0))))
    assert r["side"].tolist() == [[2]] and r["status"][0] == 3


def test_closed_scene_an_agent_wider_than_the_corridor_blocks(oracle):
    """Radius 3: rho = 4.5, the hull reaches past both bounds.  side 2, the bounds untouched, and the first touched state reported: the first i with
    10.25 - 0.5 i - 3.75 <= 4.5 is 4, where |ua| == rho exactly."""
    r = closed(oracle, [[disc(AX, 0.0, 3.0)]])
    assert r["side"].tolist() == [[2]] and r["status"][0] == 3 and r["ok_out"][0] == 0
    assert r["first_blocked_state"][0] == 4 and r["first_blocked_agent"][0] == 0 and r["width_min"][0] == 6.0
    assert same(r["bounds"], scene()["bounds"])
    two = closed(oracle, [[], [disc(0.0, 40.0, 0.1), disc(AX, 0.0, 3.0)]], set_of=np.array([1], dtype=np.int32))
    assert two["side"].tolist() == [[0, 2]] and two["first_blocked_agent"][0] == 1  # the index into agents[], not into the set... which is the same here
    three = closed(oracle, [[disc(0.0, 40.0, 0.1)], [disc(0.0, 40.0, 0.1), disc(AX, 0.0, 3.0)]], set_of=np.array([1], dtype=np.int32))
    assert three["side"].tolist() == [[0, 2]] and three["first_blocked_agent"][0] == 2  # index into agents[]: set 1 begins at 1


def test_closed_scene_two_agents_and_their_order(oracle):
    """A (2 m right) leaves lb = 0 where ua = 0; B (2.5 m left, hull 0.5 .. 4.5 there) alone is passed on the right with 3.5 m of room, but behind A only 0.5 m are
    left: with min_width = 1 it blocks.  The other way round B is passed on the right (ub = 0.5) and then A blocks."""
    A, Bg = disc(AX, -2.0, 0.5), disc(AX, 2.5, 0.5)
    npar = params_of(margin=0.25, min_width=1.0)
    alone = closed(oracle, [[Bg]], npar)
    assert alone["side"].tolist() == [[-1]] and alone["status"][0] == 2 and alone["bounds"][0, 19, 1, 1] == 0.5
    ab = closed(oracle, [[A, Bg]], npar)
    assert ab["side"].tolist() == [[1, 2]] and ab["status"][0] == 3 and ab["first_blocked_agent"][0] == 1 and ab["first_blocked_state"][0] == 9
    assert same(ab["bounds"], closed(oracle, [[A]], npar)["bounds"])  # what A carved stays, B changes nothing
    ba = closed(oracle, [[Bg, A]], npar)
    assert ba["side"].tolist() == [[-1, 2]] and ba["first_blocked_agent"][0] == 1 and same(ba["bounds"], alone["bounds"])
    assert not same(ab["bounds"], ba["bounds"])
    free = closed(oracle, [[A, Bg]], params_of(margin=0.25, min_width=0.5))  # 0.5 m are enough: both are passed, lb = 0 and ub = 0.5 where ua = 0
    assert free["side"].tolist() == [[1, -1]] and free["status"][0] == 2 and free["width_min"][0] == 0.5


def test_closed_scene_time_windows_and_skip_states(oracle):
    """The vehicle is on the line from t = 0 to t = 5 and the windows reach 1 s either side.  A crosser that lives from t = 100 to 104 meets no window."""
    late = [[(0.5, 0, [(100.0, AX, -8.0), (104.0, AX, 8.0)])]]
    r = closed(oracle, late)
    assert r["status"][0] == 1 and r["side"].tolist() == [[0]] and same(r["bounds"], scene()["bounds"])
    # the same crosser on time: on the line (y = 0) at t = 2.5625, where the vehicle is at state 20.5; only the states whose window sees it near are touched
    on_time = [[(0.5, 0, [(0.5625, AX, -8.0), (4.5625, AX, 8.0)])]]
    r = closed(oracle, on_time)
    assert r["status"][0] in (2, 3) and r["side"][0, 0] != 0
    # a window of zero width still sees a held agent, and an agent present only at one instant that is a state's time
    z = params_of(margin=0.25, t_before=0.0, t_after=0.0)
    assert closed(oracle, [[disc(AX, -2.0, 0.5)]], z)["side"].tolist() == [[1]]
    # skip_states: the touched states of the held agent are 9 .. 26
    full = closed(oracle, [[disc(AX, -2.0, 0.5)]])
    part = closed(oracle, [[disc(AX, -2.0, 0.5)]], params_of(margin=0.25, skip_states=18))
    assert same(part["bounds"][0, :18], scene()["bounds"][0, :18]) and same(part["bounds"][0, 18:], full["bounds"][0, 18:]) and part["status"][0] == 2
    assert part["width_min"][0] == 3.0  # state 19 is still carved
    for skip in (27, 41, 1000):
        none = closed(oracle, [[disc(AX, -2.0, 0.5)]], params_of(margin=0.25, skip_states=skip))
        assert none["status"][0] == 1 and none["side"].tolist() == [[0]] and same(none["bounds"], scene()["bounds"])
    blocked = closed(oracle, [[disc(AX, 0.0, 3.0)]], params_of(margin=0.25, skip_states=7))
    assert blocked["first_blocked_state"][0] == 7


def test_closed_scene_touching_the_bound_exactly_is_not_touching(oracle):
    """The held agent's hull ends at hi = 0 where ua = 0.  A corridor whose lb is 0 there is not touched (hi > Wl is strict); one ulp lower it is."""
    agent = [[disc(AX, -2.0, 0.5)]]
    at = closed(oracle, agent, bounds=scene(lb=0.0)["bounds"])
    assert at["status"][0] == 1 and at["side"].tolist() == [[0]] and same(at["bounds"], scene(lb=0.0)["bounds"])
    below = float(np.nextafter(0.0, -1.0))
    r = closed(oracle, agent, bounds=scene(lb=below)["bounds"])
    want = scene(lb=below)["bounds"]
    zero = [(i, j) for (i, j), ua in pairs_within(2.0).items() if ua == 0.0]
    assert len(zero) == 4
    for i, j in zero:
        want[0, i, j, 0] = 0.0
    assert r["status"][0] == 2 and r["side"].tolist() == [[1]] and same(r["bounds"], want)
    # and the other bound: lo = 0 where ua = 0 for the mirrored agent
    agent = [[disc(AX, 2.0, 0.5)]]
    assert closed(oracle, agent, bounds=scene(ub=0.0)["bounds"])["status"][0] == 1
    assert closed(oracle, agent, bounds=scene(ub=float(np.nextafter(0.0, 1.0)))["bounds"])["side"].tolist() == [[-1]]


def not_processed_cases():
    """(tag, case, the paths that are not processed): three lines of 12 states with n = 9, a held agent that touches each; one trigger at a time on line 1."""
    out = []

    def base():
        c = scene(n=12, N=12)
        c = {k: np.repeat(v, 3, axis=0) for k, v in c.items()}
        c["n_points"] = np.array([9, 9, 9], dtype=np.int32)
        c["agents"] = [[disc(2.25, -2.0, 0.5)]]
        return c

    c = base(); c["ok"] = np.array([1, 0, 1], dtype=np.int32); out.append(("ok = 0", c, [1]))
    c = base(); c["n_points"] = np.array([9, 0, -4], dtype=np.int32); out.append(("n < 1", c, [1, 2]))
    for key in ("ref_x", "ref_y", "ref_z", "t"):
        for bad in (np.nan, np.inf, -np.inf):
            c = base(); c[key][1, 8] = bad; out.append((f"{key} {bad}", c, [1]))
    for col, bad in ((0, np.nan), (1, np.inf), (0, -np.inf)):
        c = base(); c["bounds"][1, 8, 3, col] = bad; out.append((f"bound {bad}", c, [1]))
    c = base()  # beyond n nothing is looked at, and the rows are copied through bit for bit
    for key in ("ref_x", "ref_y", "ref_z", "t"):
        c[key][1, 9] = np.nan
    c["bounds"][1, 9:, :, 0] = np.nan; c["bounds"][1, 10, 2, 1] = -np.inf
    out.append(("beyond n", c, []))
    return out


def test_paths_that_are_not_processed(oracle):
    params = grid(oracle.default_params())
    for tag, c, bad in not_processed_cases():
        r = ref(params, params_of(margin=0.25), W=2, **c)
        for b in range(3):
            if b in bad:
                assert r["status"][b] == 0 and r["ok_out"][b] == 0 and r["side"][b].tolist() == [0, 0] and r["width_min"][b] == DBL_MAX, (tag, b)
                assert r["first_blocked_state"][b] == -1 and r["first_blocked_agent"][b] == -1 and same(r["bounds"][b], c["bounds"][b]), (tag, b)
            else:
                assert r["status"][b] == 2 and r["side"][b].tolist() == [1, 0] and same(r["bounds"][b, 9:], c["bounds"][b, 9:]), (tag, b)
                assert not same(r["bounds"][b, :9], c["bounds"][b, :9]), (tag, b)


# ---- closure: carved bounds -> KP solve -> dynamic check ----
def closure_case(oracle_params):
    """A reference line of 120 states 0.25 m apart along +x, the grid vehicle, a corridor of +-1.75 m for the circle centres (6 m of road less rad either side
    ... on this grid the road is 6 m wide), the vehicle at 4 m/s, and a parked car — a held disc of 0.75 m, 1.25 m right of the line at x = 15, that covers
    half a metre of the vehicle's swept width.  Returns the synth.Batch of the solve (bounds uncarved), the times, the agents and the parameters."""
    N = 120
    p = grid(oracle_params)
    x = 0.25 * np.arange(N)[None, :]
    zeros = np.zeros((1, N))
    bounds = np.zeros((1, N, 4, 2)); bounds[..., 0] = -1.75; bounds[..., 1] = 1.75
    batch = synth.Batch(synth.PO_KP, 1, N, synth.keep_control_steps(synth.PO_KP, x[0]), x.copy(), zeros.copy(), zeros.copy(), zeros.copy(), x.copy(), bounds,
                        np.zeros((1, 3)), np.zeros(1))
    return batch, x / 4.0, [[disc(15.0, -1.25, 0.75)]], p


CLOSURE_NP = dict(margin=0.5, skip_states=4)  # the QP pins its start: the first keep_control_steps rows are left alone (the agent is 15 m ahead anyway)


def closure_on_the_references(oracle):
    batch, t, agents, p = closure_case(oracle.device_equivalent_params())
    ag, first = binding.pack_agents(agents)
    dp = binding.default_dynamic_params()
    dp.margin, dp.stop_distance = 0.0, 2.0
    st0, info0, _ = oracle.solve_batch(batch, p, want_x=False)
    d0 = dynamic_ref.check(p, st0, t, ag, first, dp)
    nd = nudge_ref.nudge(p, batch.ref_x, batch.ref_y, batch.ref_z, t, batch.bounds, ag, first, params_of(**CLOSURE_NP))
    carved = synth.Batch(**{**batch.__dict__, "bounds": nd["bounds"]})
    st1, info1, _ = oracle.solve_batch(carved, p, want_x=False)
    d1 = dynamic_ref.check(p, st1, t, ag, first, dp)
    return dict(st0=st0, info0=info0, d0=d0, nudge=nd, st1=st1, info1=info1, d1=d1)


def test_closure_on_the_references(oracle):
    """nudge -> KP solve -> dynamic with margin 0.  The definition does NOT guarantee that the solved path is free: the QP linearises the covering circles'
    offsets and the footprint po_dynamic_batch checks has six circles, not the four covering ones.  This scene closes with the nudge margin at 0.5 m: the
    smallest gap of the solved path is 0.33 m, where the un-carved solve overlaps the agent by 0.91 m (measured on the references; with a margin of 0.3 m the
    gap is 0.23 m and with none 0.08 m, so the margin is what buys the room the linearisation and the two extra circles use up)."""
    r = closure_on_the_references(oracle)
    assert r["info0"]["status"][0] == 1 and r["d0"]["status"][0] in (2, 3)  # the un-carved solve stays on the line and runs into the parked car
    assert r["nudge"]["status"][0] == 2 and r["nudge"]["side"].tolist() == [[1]]
    assert r["info1"]["status"][0] == 1 and r["d1"]["status"][0] == 1 and r["d1"]["gap_min"][0] >= 0.0
    assert r["st1"][0, :, 1].max() > 0.5 and abs(r["st0"][0, :, 1]).max() < 1e-6  # it steered left; before, it did not steer at all


# ---- interface without a device ----
def test_new_symbols_and_abi_mirror():
    L = binding.lib()
    for name in NEW_ENTRIES:
        assert hasattr(L, name), name
        assert name in binding.EXPORTS
    fields = {"po_nudge_params": ["margin", "t_before", "t_after", "min_width", "skip_states"],
              "po_nudge_in": ["B", "N", "W", "ref_x", "ref_y", "ref_z", "n_points", "ok", "t", "bounds", "set_of", "agents", "side_prev"],
              "po_nudge_out": ["status", "ok_out", "bounds", "side", "first_blocked_state", "first_blocked_agent", "width_min"]}
    mirror = {"po_nudge_params": abi.PoNudgeParams, "po_nudge_in": abi.PoNudgeIn, "po_nudge_out": abi.PoNudgeOut}
    body = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs) for s, fs in fields.items())
    body += 'printf("%d", PO_ABI_VERSION);'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "po_hip.h"\nint main(){' + body + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    want = []
    for s, fs in fields.items():
        want.append(ctypes.sizeof(mirror[s]))
        want += [getattr(mirror[s], f).offset for f in fs]
    want += [abi.PO_ABI_VERSION]
    assert got == want and abi.PO_ABI_VERSION == 7
    assert [f for f, _ in abi.PoNudgeOut._fields_] == list(KEYS) == list(binding.Engine.NUDGE_KEYS)
    p = binding.default_nudge_params()
    assert [getattr(p, f) for f in fields["po_nudge_params"]] == [0.3, 1.0, 1.0, 0.2, 0]


def bad_params():
    """Every parameter out of its range, one at a time."""
    out = [("margin", v) for v in (np.nan, np.inf, -np.inf)]
    for f in ("t_before", "t_after", "min_width"):
        out += [(f, v) for v in (-0.5, np.nan, np.inf, -np.inf)]
    return out + [("skip_states", -1)]


def test_null_arguments_and_ranges_are_refused_without_a_device():
    """The argument checks come before the handle is touched, so any non-NULL handle value shows them here."""
    L = binding.lib()
    npar, ni, no = binding.default_nudge_params(), abi.PoNudgeIn(), abi.PoNudgeOut()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))
    buf = np.zeros(64)
    ibuf = np.zeros(8, dtype=np.int32)
    p = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)
    lists = abi.PoAgentLists(None, p(ibuf), 0, 1)
    for entry in (L.po_nudge_batch, L.po_nudge_batch_device):
        assert entry(None, ctypes.byref(npar), ctypes.byref(ni), ctypes.byref(no)) == abi.PO_ERR_INVALID
        assert entry(None, None, None, None) == abi.PO_ERR_INVALID
        assert entry(fake, None, ctypes.byref(ni), ctypes.byref(no)) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(npar), None, ctypes.byref(no)) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(npar), ctypes.byref(ni), None) == abi.PO_ERR_INVALID
        assert entry(fake, ctypes.byref(npar), ctypes.byref(ni), ctypes.byref(no)) == abi.PO_OK  # B = 0: nothing to do, and the handle is not looked at
        for f, v in bad_params():
            assert entry(fake, ctypes.byref(params_of(**{f: v})), ctypes.byref(ni), ctypes.byref(no)) == abi.PO_ERR_INVALID, (f, v)
        assert entry(fake, ctypes.byref(params_of(margin=-5.0, t_before=0.0, t_after=0.0, min_width=0.0)), ctypes.byref(ni), ctypes.byref(no)) == abi.PO_OK
        for f, v in (("B", -1), ("N", -1), ("W", -1)):
            bad = abi.PoNudgeIn(); setattr(bad, f, v)
            assert entry(fake, ctypes.byref(npar), ctypes.byref(bad), ctypes.byref(no)) == abi.PO_ERR_INVALID, f
        # B = 0 is decided AFTER the checks: W = 0 with side or side_prev, bounds that alias, negative list sizes
        w0 = abi.PoNudgeIn(); w0.side_prev = p(ibuf)
        assert entry(fake, ctypes.byref(npar), ctypes.byref(w0), ctypes.byref(no)) == abi.PO_ERR_INVALID
        s0 = abi.PoNudgeOut(); s0.side = p(ibuf)
        assert entry(fake, ctypes.byref(npar), ctypes.byref(ni), ctypes.byref(s0)) == abi.PO_ERR_INVALID
        al_in, al_out = abi.PoNudgeIn(), abi.PoNudgeOut()
        al_in.bounds = p(buf); al_out.bounds = p(buf)
        assert entry(fake, ctypes.byref(npar), ctypes.byref(al_in), ctypes.byref(al_out)) == abi.PO_ERR_INVALID
        for neg in (abi.PoAgentLists(None, p(ibuf), -1, 1), abi.PoAgentLists(None, p(ibuf), 0, -1)):
            li = abi.PoNudgeIn(); li.agents = ctypes.pointer(neg)
            assert entry(fake, ctypes.byref(npar), ctypes.byref(li), ctypes.byref(no)) == abi.PO_ERR_INVALID

        # B > 0: every required pointer missing in turn is refused before the handle is read
        def full():
            fi = abi.PoNudgeIn(1, 2, 1, p(buf), p(buf, 16), p(buf, 32), None, None, p(buf, 48), p(buf, 64), None, ctypes.pointer(lists), None)
            fo = abi.PoNudgeOut(p(ibuf), None, p(buf, 256), None, None, None, None)
            return fi, fo

        for key in ("ref_x", "ref_y", "ref_z", "t", "bounds", "agents"):
            fi, fo = full(); setattr(fi, key, None)
            assert entry(fake, ctypes.byref(npar), ctypes.byref(fi), ctypes.byref(fo)) == abi.PO_ERR_INVALID, key
        for key in ("status", "bounds"):
            fi, fo = full(); setattr(fo, key, None)
            assert entry(fake, ctypes.byref(npar), ctypes.byref(fi), ctypes.byref(fo)) == abi.PO_ERR_INVALID, key
        for bad_lists in (abi.PoAgentLists(None, None, 0, 1), abi.PoAgentLists(None, p(ibuf), 0, 0), abi.PoAgentLists(None, p(ibuf), 3, 1)):
            fi, fo = full(); fi.agents = ctypes.pointer(bad_lists)
            assert entry(fake, ctypes.byref(npar), ctypes.byref(fi), ctypes.byref(fo)) == abi.PO_ERR_INVALID
        fi, fo = full(); fo.bounds = fi.bounds
        assert entry(fake, ctypes.byref(npar), ctypes.byref(fi), ctypes.byref(fo)) == abi.PO_ERR_INVALID  # out->bounds == in->bounds
    L.po_default_nudge_params(None)  # a NULL struct is ignored


def test_host_mirror_header_compiles():
    inc = os.path.join(ROOT, "path_optimizer_amd", "host", "include")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "path_optimizer_amd/nudge.hpp"\nint main() { PathOptimizationNS::CorridorNudger n; (void)n; return 0; }\n')
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-I", os.path.join(ROOT, "include"), src])


def test_host_mirror_nudge_test_compiles_and_links():
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "nudge_test"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(host, "nudge_test"))
    assert "CorridorNudger" in open(os.path.join(host, "test", "nudge_test.cpp")).read()


def mirror_case():
    """The seeded case of host/test/nudge_test.cpp, rebuilt with the same integer generator and the same dyadic arithmetic: bit for bit its inputs."""
    state = [13579]

    def u():
        state[0] = (state[0] * 1103515245 + 12345) & 0x7fffffff
        return (((state[0] >> 8) % 257) - 128) / 64.0

    B = 6
    n = np.array([3 + (b * 13) % 47 for b in range(B)], dtype=np.int32)
    N = int(n.max())
    x, y, z, t = (np.zeros((B, N)) for _ in range(4))
    bounds = np.zeros((B, N, 4, 2))
    for b in range(B):
        for i in range(n[b]):
            x[b, i] = -6.0 + 0.5 * i + u() / 16; y[b, i] = u() / 2; z[b, i] = u() / 8
            t[b, i] = 0.125 * i
            for j in range(4):
                bounds[b, i, j] = (-3.5 - 0.25 * (i % 3) - 0.125 * j, 3.5 + 0.5 * (i % 2) + 0.125 * j)
    sets = []
    for s in range(3):
        agents = []
        for a in range(0 if s == 1 else 5):
            npts = 1 + (a * 3 + s) % 8
            t0, x0, y0 = u(), 2.0 + 4 * u(), 2 * u()
            agents.append((0.25 + 0.125 * a, (a + s) % 4, [(t0 + 0.75 * j, x0 + 0.5 * j, y0 + (j % 2) * 0.25) for j in range(npts)]))
        sets.append(agents)
    ok = np.ones(B, dtype=np.int32); ok[4] = 0
    c = dict(ref_x=x, ref_y=y, ref_z=z, t=t, bounds=bounds, n_points=n, ok=ok, set_of=np.array([b % 3 for b in range(B)], dtype=np.int32), agents=sets, W=5)
    return c, params_of(margin=0.125, t_before=0.5, t_after=0.75, min_width=0.75, skip_states=1)


def test_mirror_case_exercises_the_stage(oracle):
    """The case the C++ program prints is not an idle one: on the reference it carves and leaves one line alone."""
    c, npar = mirror_case()
    r = ref(oracle.default_params(), npar, **c)
    assert r["status"][4] == 0 and (r["status"][[1]] == 1).all() and 2 in r["status"].tolist()
    again = ref(oracle.default_params(), npar, **dict(c, side_prev=r["side"]))
    assert_same(again, r, tag="side_prev = the last sides")


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0)  # no map: the stage reads none
    yield e
    e.close()


@pytest.fixture(scope="module")
def grid_eng():
    e = binding.Engine(0, grid(binding.default_params()))
    yield e
    e.close()


def _dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


OUT_TYPES = {"status": np.int32, "ok_out": np.int32, "bounds": np.float64, "side": np.int32, "first_blocked_state": np.int32, "first_blocked_agent": np.int32,
             "width_min": np.float64}
F64_IN, I32_IN = ("ref_x", "ref_y", "ref_z", "t", "bounds"), ("n_points", "ok", "set_of", "side_prev")


def width_of(c):
    if c.get("W") is not None:
        return int(c["W"])
    if c.get("side_prev") is not None:
        return np.asarray(c["side_prev"]).shape[1]
    _, first = binding.pack_agents(c["agents"])
    return max(1, int(np.diff(first).max()))


def sentinels(B, N, W, want=KEYS):
    """Outputs that start as 7 / 77."""
    shape = {"bounds": (B, N, 4, 2), "side": (B, W)}
    return {k: np.full(shape.get(k, (B,)), 77 if OUT_TYPES[k] == np.int32 else 7.0, dtype=OUT_TYPES[k]) for k in want if not (k == "side" and W == 0)}


def run_device(e, c, npar=None, want=KEYS):
    agents, first = binding.pack_agents(c["agents"])
    t = {"first": _dev(first), "agents": _dev(agents.view(np.uint8)) if len(agents) else None}
    for k in F64_IN:
        t[k] = _dev(np.asarray(c[k], dtype=np.float64))
    for k in I32_IN:
        t[k] = None if c.get(k) is None else _dev(np.asarray(c[k], dtype=np.int32))
    B, N = c["ref_x"].shape
    W = width_of(c)
    out = {k: _dev(v) for k, v in sentinels(B, N, W, want).items()}
    if "side" not in out and W > 0 and t["side_prev"] is None:  # the binding reads W off side or side_prev: without both, W = 0 is what the call says
        W = 0
    e.nudge_batch_device(t, out, npar or params_of())
    return {k: _host(v) for k, v in out.items()}


def run_host(e, c, npar=None):
    """The host entry on outputs that start as 7 / 77 (Engine.nudge_batch allocates zeros: the sentinel goes through the C entry directly)."""
    npar = npar or params_of()
    ag, first = binding.pack_agents(c["agents"])
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    a = {k: np.ascontiguousarray(c[k], dtype=np.float64) for k in F64_IN}
    a.update({k: None if c.get(k) is None else np.ascontiguousarray(c[k], dtype=np.int32) for k in I32_IN})
    B, N = a["ref_x"].shape
    W = width_of(c)
    lists = abi.PoAgentLists(p(ag) if len(ag) else None, p(first), len(ag), len(first) - 1)
    ni = abi.PoNudgeIn(B, N, W, p(a["ref_x"]), p(a["ref_y"]), p(a["ref_z"]), p(a["n_points"]), p(a["ok"]), p(a["t"]), p(a["bounds"]), p(a["set_of"]),
                       ctypes.pointer(lists), p(a["side_prev"]))
    r = sentinels(B, N, W)
    binding._check(binding.lib().po_nudge_batch(e._h, ctypes.byref(npar), ctypes.byref(ni), ctypes.byref(abi.PoNudgeOut(*[p(r.get(k)) for k in KEYS]))))
    return r


def both(e, params, npar=None, tag="", **c):
    """Host entry, device entry and the reference: all three bitwise equal, outputs sentinel-filled.  Returns the reference's dict."""
    want = ref(params, npar, **c)
    keys = tuple(k for k in KEYS if not (k == "side" and width_of(c) == 0))
    assert_same(run_host(e, c, npar), want, keys=keys, tag=tag + " host")
    assert_same(run_device(e, c, npar), want, keys=keys, tag=tag + " device")
    return want


@pytest.mark.gpu
def test_lane_ownership_boundaries_and_ragged_lengths(eng, oracle):
    """4 N pairs over 64 lanes: N = 1, 2, 15, 16, 17 (one sweep, 64 pairs exactly, one more), 63, 64, 65, 200, and one line longer than the states whose cos / sin
    the kernel keeps in LDS; ragged n with 0 among them."""
    seen = set()
    for k, N in enumerate((1, 2, 15, 16, 17, 63, 64, 65, 200)):
        c = random_case(200 + k, 7, N, per_set=(6, 0, 3))
        c["n_points"][1] = 0
        seen |= set(both(eng, oracle.default_params(), tag=f"N={N}", **c)["status"].tolist())
    assert seen == {0, 1, 2, 3}
    N = NDG_TRIG + 19
    c = random_case(230, 2, N, per_set=(4,), ragged=False)
    c["n_points"][1] = NDG_TRIG + 1
    for b in range(2):  # an agent parked beside the last states, where the kernel computes cos / sin again
        i = int(c["n_points"][b]) - 1
        c["agents"][0][b]["n_pts"], c["agents"][0][b]["flags"], c["agents"][0][b]["radius"] = 1, 3, 0.3
        c["agents"][0][b]["x"][0], c["agents"][0][b]["y"][0] = c["ref_x"][b, i] + 1.0, c["ref_y"][b, i] + 1.0
    r = both(eng, oracle.default_params(), tag=f"N={N}", **c)
    assert (r["side"][:, :2] != 0).any()


@pytest.mark.gpu
def test_agent_counts_around_the_chunk(eng, oracle):
    """0, 1, 31, 32, 33 and 65 agents in the set: none, one chunk not full, full, one more, three chunks; as they come, and with only the LAST agent near."""
    for k, count in enumerate((0, 1, NDG_CHUNK - 1, NDG_CHUNK, NDG_CHUNK + 1, 2 * NDG_CHUNK + 1)):
        c = random_case(300 + k, 5, 40, per_set=(count,), W=max(count, 1))
        c["set_of"] = None
        r = both(eng, oracle.default_params(), tag=f"{count} agents", **c)
        if count == 0:
            assert set(r["status"].tolist()) <= {0, 1}
            continue
        agents, first = c["agents"]
        far = agents.copy()
        far["x"][:count - 1] += 500.0
        c["agents"] = (far, first)
        c["side_prev"] = None
        r = both(eng, oracle.default_params(), tag=f"the last of {count}", **c)
        assert (r["side"][:, :count - 1] == 0).all()


@pytest.mark.gpu
def test_batch_sizes_and_position_in_the_batch(eng, oracle):
    for B in (1, 2, 65):
        both(eng, oracle.default_params(), tag=f"B={B}", **random_case(400 + B, B, 33))
    c = random_case(410, 70, 33, ragged=False)
    whole = both(eng, oracle.default_params(), tag="70 lines", **c)
    alone = {k: (v[41:42] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    r = both(eng, oracle.default_params(), tag="line 41 alone", **alone)
    for k in KEYS:
        assert same(r[k][0], whole[k][41]), k


@pytest.mark.gpu
def test_sets_and_side_widths(eng, oracle):
    """Three sets with one empty, set_of given and NULL; W below, at and above the size of the largest set, and 0 (no side at all)."""
    c = random_case(500, 12, 50, per_set=(7, 0, 4))
    r = both(eng, oracle.default_params(), tag="three sets", **c)
    assert (r["status"][c["set_of"] == 1] <= 1).all()
    both(eng, oracle.default_params(), tag="set_of NULL", **dict(c, set_of=None))
    for W in (3, 7, 12):
        cw = random_case(500, 12, 50, per_set=(7, 0, 4), W=W)
        r = both(eng, oracle.default_params(), tag=f"W={W}", **cw)
        assert r["side"].shape == (12, W) and (r["side"][:, 7:] == 0).all()
    c0 = dict(random_case(500, 12, 50, per_set=(7, 0, 4), hints=False), W=0)
    want = ref(oracle.default_params(), None, **dict(c0, W=1))
    keys = tuple(k for k in KEYS if k != "side")
    assert_same(run_host(eng, c0), want, keys=keys, tag="W=0 host")
    assert_same(run_device(eng, c0, want=keys), want, keys=keys, tag="W=0 device")


def piece_case():
    """One straight line of 40 states at 2 m/s (t = 0.25 i) with windows of 0.5 s before and 0.75 s after, so that window ends are multiples of 0.25; agents of
    1 .. 8 points with every flag combination whose times are multiples of 0.25 too: piece boundaries fall ON window ends (ta == tb pieces)."""
    N = 40
    x = np.zeros((1, N)); x[0] = 0.5 * np.arange(N)
    bounds = np.zeros((1, N, 4, 2)); bounds[..., 0] = -2.5; bounds[..., 1] = 2.5
    rng = np.random.default_rng(3107)
    agents = []
    for npts in range(1, 9):
        for flags in range(4):
            t0 = 0.25 * int(rng.integers(-4, 30))
            tt = t0 + 0.25 * np.concatenate(([0], np.cumsum(rng.integers(1, 5, npts - 1))))
            xx = 0.125 * rng.integers(0, 160, npts); yy = 0.125 * rng.integers(-40, 41, npts)
            agents.append((0.125 * int(rng.integers(1, 5)), flags, list(zip(tt, xx, yy))))
    return dict(ref_x=x, ref_y=np.zeros((1, N)), ref_z=np.zeros((1, N)), t=x / 2.0, bounds=bounds, agents=[agents]), params_of(margin=0.125, t_before=0.5, t_after=0.75)


@pytest.mark.gpu
def test_agent_pieces_with_boundaries_on_the_window_ends(eng, grid_eng, oracle):
    c, npar = piece_case()
    agents = c["agents"][0]
    seen = set()
    for k in range(0, len(agents), 4):  # the four flag combinations of one point count together, then every agent alone
        seen |= set(both(grid_eng, grid(oracle.default_params()), npar, tag=f"{k // 4 + 1} points", **dict(c, agents=[agents[k:k + 4]]))["side"].reshape(-1).tolist())
    single = dict(c, agents=[[a] for a in agents], set_of=np.zeros(1, dtype=np.int32))
    for s in range(len(agents)):
        single["set_of"][0] = s
        seen |= set(both(grid_eng, grid(oracle.default_params()), npar, tag=f"agent {s}", **single)["side"].reshape(-1).tolist())
    assert seen == {-1, 0, 1, 2}
    both(eng, oracle.default_params(), npar, tag="default vehicle", **c)


@pytest.mark.gpu
def test_closed_scenes_on_the_device(grid_eng, oracle):
    """Every closed scene of the CPU list, ties and ulp cases included, through both entries."""
    params = grid(oracle.default_params())
    m25 = dict(margin=0.25)
    prev = lambda v: np.array([[v]], dtype=np.int32)
    A, Bg, centre = disc(AX, -2.0, 0.5), disc(AX, 2.5, 0.5), disc(AX, 0.0, 0.5)
    below, above = float(np.nextafter(0.0, -1.0)), float(np.nextafter(0.0, 1.0))
    cases = [("left", [[A]], m25, {}), ("right", [[disc(AX, 2.0, 0.5)]], m25, {}), ("tie", [[centre]], m25, {}),
             ("tie, hint right", [[centre]], m25, dict(side_prev=prev(-1))), ("tie, hint left", [[centre]], m25, dict(side_prev=prev(1))),
             ("tie, no hint", [[centre]], m25, dict(side_prev=prev(2))), ("hint not passable", [[A]], m25, dict(side_prev=prev(-1))),
             ("min_width met", [[centre]], dict(margin=0.25, min_width=1.0), {}),
             ("min_width missed by an ulp", [[centre]], dict(margin=0.25, min_width=float(np.nextafter(1.0, 2.0))), {}),
             ("blocks", [[disc(AX, 0.0, 3.0)]], m25, {}), ("A then B", [[A, Bg]], dict(margin=0.25, min_width=1.0), {}),
             ("B then A", [[Bg, A]], dict(margin=0.25, min_width=1.0), {}), ("A and B pass", [[A, Bg]], dict(margin=0.25, min_width=0.5), {}),
             ("late crosser", [[(0.5, 0, [(100.0, AX, -8.0), (104.0, AX, 8.0)])]], m25, {}),
             ("crosser on time", [[(0.5, 0, [(0.5625, AX, -8.0), (4.5625, AX, 8.0)])]], m25, {}),
             ("windows of zero width", [[A]], dict(margin=0.25, t_before=0.0, t_after=0.0), {}), ("skip 18", [[A]], dict(margin=0.25, skip_states=18), {}),
             ("skip 27", [[A]], dict(margin=0.25, skip_states=27), {}), ("skip beyond", [[A]], dict(margin=0.25, skip_states=1000), {}),
             ("hi == Wl", [[A]], m25, dict(bounds=scene(lb=0.0)["bounds"])), ("hi one ulp above Wl", [[A]], m25, dict(bounds=scene(lb=below)["bounds"])),
             ("lo == Wu", [[disc(AX, 2.0, 0.5)]], m25, dict(bounds=scene(ub=0.0)["bounds"])),
             ("lo one ulp below Wu", [[disc(AX, 2.0, 0.5)]], m25, dict(bounds=scene(ub=above)["bounds"]))]
    got = {}
    for tag, sets, kw, extra in cases:
        got[tag] = both(grid_eng, params, params_of(**kw), tag=tag, **dict(scene(), agents=sets, **extra))
    assert got["tie"]["side"].tolist() == [[1]] and got["tie, hint right"]["side"].tolist() == [[-1]] and got["min_width met"]["status"][0] == 2
    assert got["min_width missed by an ulp"]["status"][0] == 3 and got["A then B"]["side"].tolist() == [[1, 2]] and got["B then A"]["side"].tolist() == [[-1, 2]]
    assert got["hi == Wl"]["status"][0] == 1 and got["hi one ulp above Wl"]["status"][0] == 2 and got["lo == Wu"]["status"][0] == 1


@pytest.mark.gpu
def test_paths_that_are_not_processed_on_the_device(grid_eng, oracle):
    params = grid(oracle.default_params())
    for tag, c, bad in not_processed_cases():
        r = both(grid_eng, params, params_of(margin=0.25), tag=tag, W=2, **c)
        assert [b for b in range(3) if r["status"][b] == 0] == bad, tag


@pytest.mark.gpu
def test_optional_arguments_and_empty_calls(eng, oracle):
    c = random_case(600, 70, 30)
    ok = np.ones(70, dtype=np.int32); ok[::9] = 0
    c["ok"] = ok
    want = ref(oracle.default_params(), None, **c)
    for drop in ("ok_out", "side", "first_blocked_state", "first_blocked_agent", "width_min"):  # every optional output NULL in turn
        keys = tuple(k for k in KEYS if k != drop)
        assert_same(run_device(eng, c, want=keys), want, keys=keys, tag="without " + drop)
    assert_same(run_device(eng, c, want=("status", "bounds")), want, keys=("status", "bounds"), tag="status and bounds alone")
    for drop in ("n_points", "ok", "set_of", "side_prev"):  # every optional input NULL in turn
        both(eng, oracle.default_params(), tag="no " + drop, **{k: v for k, v in c.items() if k != drop})
    r = eng.nudge_batch(**{k: v for k, v in c.items()})
    assert_same(r, want, tag="Engine.nudge_batch")
    # B = 0: PO_OK from both entries on this handle, which has no map; nothing is looked at, not even the agents
    L = binding.lib()
    npar = params_of()
    for entry in (L.po_nudge_batch, L.po_nudge_batch_device):
        ni = abi.PoNudgeIn(); ni.N = 5; ni.W = 3
        assert entry(eng._h, ctypes.byref(npar), ctypes.byref(ni), ctypes.byref(abi.PoNudgeOut())) == abi.PO_OK
    none = dict(c, agents=[[], []], set_of=np.zeros(70, dtype=np.int32))  # no agents at all: nothing is touched
    r = both(eng, oracle.default_params(), tag="no agents", **none)
    assert set(r["status"].tolist()) == {0, 1} and same(r["bounds"], c["bounds"]) and (r["side"] == 0).all()
    with pytest.raises(binding.PoError):  # out->bounds == in->bounds
        t = {k: _dev(np.asarray(c[k], dtype=np.float64)) for k in F64_IN}
        t["first"] = _dev(np.zeros(2, dtype=np.int32))
        eng.nudge_batch_device(t, {"status": _dev(np.zeros(70, dtype=np.int32)), "bounds": t["bounds"]})


@pytest.mark.gpu
def test_device_lists_are_read_clamped(eng, oracle):
    """What the host entry refuses, the device entry reads as the definition says: set_of and first clamped, an agent with a bad n_pts covers nothing."""
    c = random_case(605, 6, 30, per_set=(5, 5), ragged=False)
    agents, first = c["agents"]
    agents = agents.copy(); agents["n_pts"][2] = 9; agents["n_pts"][7] = -1
    agents["t"][4][:3] = (2.0, 1.0, 3.0)  # times that go back: the segment of negative duration is skipped
    c["agents"] = (agents, np.array([-3, 5, 99], dtype=np.int32))
    c["set_of"] = np.array([0, 1, -2, 7, 1, 0], dtype=np.int32)
    want = ref(oracle.default_params(), None, **c)
    assert_same(run_device(eng, c), want, tag="clamped")
    assert (want["side"] != 0).any() and (want["side"][[0, 2, 5], 2] == 0).all() and (want["side"][[1, 3, 4], 2] == 0).all()
    with pytest.raises(binding.PoError):
        eng.nudge_batch(**c)
    for bad_first in ([1, 5, 10], [0, 6, 5], [0, 5, 11]):
        with pytest.raises(binding.PoError):
            eng.nudge_batch(**dict(c, agents=(random_case(605, 6, 30, per_set=(5, 5))["agents"][0], np.array(bad_first, dtype=np.int32)), set_of=None))


@pytest.mark.gpu
def test_chain_bounds_nudge_solve_speed_dynamic_on_one_stream(oracle):
    """bounds -> nudge -> po_solve_batch_device -> speed -> dynamic, device entries only, no synchronisation and no host copy between the five calls, on the scene
    of test_closure_on_the_references with the road as a map (walls 3 m either side of the line).  Every stage equals its reference on the device output of the
    stage before it — bit for bit where the stage is defined so, at the solver tolerance of tests/test_gpu_parity.py for the solve — and the chain ends as the CPU
    closure does: free, where the solve on the uncarved bounds ends in conflict."""
    import torch

    from test_gpu_parity import _compare_every_path

    batch, t, agents, op = closure_case(oracle.device_equivalent_params())
    B, N = batch.B, batch.N
    e = binding.Engine(0, grid(binding.default_params()))
    sx, sy, res = 440, 120, 0.1  # 44 m x 12 m around (15, 0): free inside |y| < 3, the distance to the nearer wall
    cy = 0.5 * sy * res - (np.arange(sy) + 0.5) * res
    dist = np.tile(np.maximum(3.0 - np.abs(cy), 0.0).astype(np.float32), (sx, 1))
    e.set_map(dist, res, 15.0, 0.0)
    ks = 1.5 * np.arange(int(math.ceil((N - 1) * 0.25 / 1.5)) + 4)
    paths = dict(ref_x=batch.ref_x, ref_y=batch.ref_y, ref_z=batch.ref_z, ref_s=batch.ref_s, knot_s=ks[None, :], knot_x=ks[None, :], knot_y=np.zeros((1, len(ks))))
    pt = {k: _dev(np.ascontiguousarray(v, dtype=np.float64)) for k, v in paths.items()}
    ag, first = binding.pack_agents(agents)
    lists = {"first": _dev(first), "agents": _dev(ag.view(np.uint8))}
    npar, spd, dp = params_of(**CLOSURE_NP), binding.default_speed_params(), binding.default_dynamic_params()
    dp.margin, dp.stop_distance = 0.0, 2.0
    raw = torch.full((B, N, 4, 2), 7.0, dtype=torch.float64, device="cuda"); nvalid = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    nd = {k: _dev(v) for k, v in sentinels(B, N, 1).items()}
    dev = [binding.DeviceBatch(batch), binding.DeviceBatch(batch)]  # the carved solve and the uncarved one
    dev[0].bounds, dev[1].bounds = nd["bounds"], raw
    dev[0].n_points = dev[1].n_points = nvalid
    f64 = lambda: _dev(np.full((B, N), 7.0))
    speed = [{"v": f64(), "a": f64(), "t": f64(), "total_time": _dev(np.full(B, 7.0)), "status": _dev(np.full(B, 77, dtype=np.int32))} for _ in range(2)]
    dkeys = {"status": np.int32, "ok_out": np.int32, "gap_min": np.float64, "first_state": np.int32, "first_agent": np.int32, "stop_state": np.int32,
             "first_time": np.float64, "gap": np.float64, "v_limit": np.float64}
    dyn = [{k: _dev(np.full((B, N) if k in ("gap", "v_limit") else (B,), 77 if ty == np.int32 else 7.0, dtype=ty)) for k, ty in dkeys.items()} for _ in range(2)]
    v0, tt = _dev(np.full(B, 4.0)), _dev(t)
    torch.cuda.synchronize()
    e.bounds_batch_device(pt, raw, nvalid)
    e.nudge_batch_device(dict(lists, ref_x=pt["ref_x"], ref_y=pt["ref_y"], ref_z=pt["ref_z"], t=tt, bounds=raw, n_points=nvalid), nd, npar)
    for k in range(2):
        e.solve_batch_device(dev[k])
        e.speed_batch_device({"states": dev[k].out_states, "n_states": nvalid, "v0": v0}, speed[k], spd)
        e.dynamic_batch_device(dict(lists, states=dev[k].out_states, n_states=nvalid, t=speed[k]["t"]), dyn[k], dp)
    got_raw, nv = _host(raw), _host(nvalid)
    got_nd = {k: _host(v) for k, v in nd.items()}
    got = [dict(states=_host(dev[k].out_states), info=dev[k].info_numpy(), speed={a: _host(v) for a, v in speed[k].items()},
                dyn={a: _host(v) for a, v in dyn[k].items()}) for k in range(2)]
    e.close()
    n = int(nv[0])
    assert n > 100 and np.abs(got_raw[0, :n, :, 0] + 1.75).max() < 0.11 and np.abs(got_raw[0, :n, :, 1] - 1.75).max() < 0.11  # the road of the closure, to a map cell
    want_nd = nudge_ref.nudge(op, batch.ref_x, batch.ref_y, batch.ref_z, t, got_raw, ag, first, npar, n_points=nv)
    assert_same(got_nd, want_nd, tag="nudge on the stream")
    assert got_nd["status"].tolist() == [2] and got_nd["side"].tolist() == [[1]]
    for k, bnd in enumerate((got_nd["bounds"], got_raw)):
        ob = synth.Batch(**{**batch.__dict__, "bounds": bnd, "n_points": nv})
        ost, oinfo, _ = oracle.solve_batch(ob, op, want_x=False)
        assert got[k]["info"]["status"][0] == 1 and oinfo["status"][0] == 1
        _compare_every_path(got[k]["info"], oinfo, got[k]["states"][:, :n], ost[:, :n], got[k]["states"][:, :n], ost[:, :n], min_same=1)
        sp_ref = speed_ref.profile(op, got[k]["states"], np.full(B, 4.0), spd, n_states=nv)
        assert_same(got[k]["speed"], sp_ref, keys=("v", "a", "t", "total_time", "status"), tag=f"speed {k}")
        d_ref = dynamic_ref.check(op, got[k]["states"], got[k]["speed"]["t"], ag, first, dp, n_states=nv)
        assert_same(got[k]["dyn"], d_ref, keys=tuple(dkeys), tag=f"dynamic {k}")
    assert got[0]["dyn"]["status"].tolist() == [1] and got[1]["dyn"]["status"][0] in (2, 3)  # as the CPU closure: free after the nudge, in conflict without it
    cpu = closure_on_the_references(oracle)
    assert cpu["d1"]["status"].tolist() == [1] and cpu["d0"]["status"][0] == got[1]["dyn"]["status"][0]


@pytest.mark.gpu
def test_host_mirror_nudge_program(eng, oracle):
    """CorridorNudger::nudge end to end in its own process: its statuses, sides and its checksum of the bounds equal the Python call's and the reference's."""
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "nudge_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "nudge_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "nudge_test passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]
    printed = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("status", "sides", "checksum")}
    c, npar = mirror_case()
    got = both(eng, oracle.default_params(), npar, tag="mirror case", **c)
    assert_same(eng.nudge_batch(params=npar, **c), got, tag="Engine.nudge_batch")
    sizes = [len(c["agents"][s]) for s in c["set_of"]]
    assert printed["status"] == got["status"].tolist() and printed["sides"] == [int(v) for b, k in enumerate(sizes) for v in got["side"][b, :k]]
    total = 0
    for b in range(len(c["n_points"])):
        total += int(got["bounds"][b, :c["n_points"][b]].view(np.uint64).sum(dtype=np.uint64))
    assert printed["checksum"] == [total & 0xffffffffffffffff]


@pytest.mark.gpu
def test_host_validation(eng):
    x, y, z, t, bounds = make_lines(700, 4, 8, box=1.0)
    good = [[disc(0.0, 0.0, 0.3), (0.2, 3, [(0.0, 1.0, 1.0), (1.0, 2.0, 1.0), (2.5, 2.0, 3.0)])], []]
    assert (eng.nudge_batch(x, y, z, t, bounds, good)["status"] > 0).all()
    for f, v in bad_params():
        with pytest.raises(binding.PoError):
            eng.nudge_batch(x, y, z, t, bounds, good, params=params_of(**{f: v}))

    def bad_agent(field, val, idx=None):
        ag, first = binding.pack_agents(good)
        if idx is None:
            ag[1][field] = val
        else:
            ag[1][field][idx] = val
        return ag, first

    lists = [bad_agent("n_pts", 0), bad_agent("n_pts", 9), bad_agent("radius", -0.1), bad_agent("radius", np.nan), bad_agent("t", np.nan, 1),
             bad_agent("t", 0.0, 1), bad_agent("x", np.nan, 0), bad_agent("y", -np.inf, 2), bad_agent("flags", 4)]
    ag, first = binding.pack_agents(good)
    lists += [(ag, np.array(f, dtype=np.int32)) for f in ([1, 2, 2], [0, 2, 1], [0, 2, 3])]
    for k, bad in enumerate(lists):
        with pytest.raises(binding.PoError):
            eng.nudge_batch(x, y, z, t, bounds, bad)
            raise AssertionError(f"list {k} was accepted")
    for so in ([0, 1, 2, 0], [0, -1, 0, 0]):
        with pytest.raises(binding.PoError):
            eng.nudge_batch(x, y, z, t, bounds, good, set_of=np.array(so, dtype=np.int32))
