"""The glue stages around the QPs (bSpline, segmentRawReference, the tail of postSmooth, the first half of segmentSmoothedPath) and the orchestration of
po_plan_batch at their edges.

  A. CPU: the restated clamped B-spline (tinyspline is not part of the reference tree) against scipy.interpolate.BSpline on the same knot vector and the same
     accumulated parameters, for the three degrees the spacing rule picks and for the refusals.
  B. GPU: po_bspline / po_segment_raw / po_post_project / po_segment_init_batch_device bit for bit against the oracle's portable-math mode: ragged counts, the
     refusals, capacities that just fit and just do not, knot ties, both extrapolation branches, the 75 degree threshold, the +-pi wrap, the goal trim.
  C. GPU: po_plan_batch with two keep groups in one call, in permuted order, with instances that stop early in between, with one instance over a capacity, through
     the device entry with and without the optional outputs, and with enable_exact_position.
CPU legs: the oracle's two arithmetic modes agree on every input of B and C (the device is compared with the portable mode; this ties it to the mode pinned against the
reference), and that mode against the reference's own segmentRawReference / segmentSmoothedPath (live where the reference tree exists, through tests/golden/glue_ref.npz
everywhere).  Inputs are built here, deterministically; tests/golden/make_glue_golden.py imports them from this file."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from path_optimizer_amd.abi import PO_ERR_UNSUPPORTED, PO_STATUS_UNSOLVED, PoPlanIn, PoPlanOut, PoSplineIn

HAVE_REF = os.path.isdir("/root/reference")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glue_ref.npz")
DEG75 = 75 * np.pi / 180


def _frozen(obj):
    """obj with every numpy array in it read-only: the cached inputs are shared by the tests and by tests/golden/make_glue_golden.py."""
    if isinstance(obj, np.ndarray):
        obj.setflags(write=False)
    elif isinstance(obj, dict):
        for v in obj.values():
            _frozen(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _frozen(v)
    return obj


def _both_modes(oracle, fn):
    """(fn() in the oracle's default mode, fn() in its portable-math mode)"""
    a = fn()
    with oracle.portable_math():
        b = fn()
    return a, b


# ------------------------------------------------------------------ A: the restated B-spline against scipy
def _polyline(ds, n, bend=0.05, x0=-20.0, y0=7.0):
    """n waypoints `ds` apart on a curve whose heading grows by `bend` per waypoint"""
    phi = bend * np.arange(n - 1)
    return x0 + np.concatenate(([0.0], np.cumsum(ds * np.cos(phi)))), y0 + np.concatenate(([0.0], np.cumsum(ds * np.sin(phi))))


def _degree(px, py):
    """bSpline()'s rule on the average waypoint spacing: (degree, polyline length)"""
    length = float(np.hypot(np.diff(px), np.diff(py)).sum())
    avg = length / (len(px) - 1)
    return (3 if avg > 10 else (4 if avg > 5 else 5)), length


def _parameters(length):
    """the accumulated parameter values of bSpline(): t += 1 / length while t < 1, then 1"""
    tt, t, dt = [], 0.0, 1.0 / length
    while t < 1:
        tt.append(t)
        t += dt
    return np.array(tt + [1.0])


@pytest.mark.parametrize("n", (3, 4, 5, 6, 9, 12, 17, 24))
@pytest.mark.parametrize("ds", (3.0, 7.0, 12.0))
def test_oracle_bspline_matches_scipy(oracle, ds, n):
    """Bar 1e-12 on coordinates of up to 300 m: both sides evaluate the same polynomial pieces by a handful of convex combinations per point, the difference measured
    is 1.1e-13 at most."""
    from scipy.interpolate import BSpline

    rng = np.random.default_rng(int(10 * ds) + n)
    px = np.cumsum(rng.uniform(0.9 * ds, 1.1 * ds, n)); py = rng.uniform(-1, 1, n)
    deg, length = _degree(px, py)
    assert deg == {3.0: 5, 7.0: 4, 12.0: 3}[ds]
    cnt, x, y, s = oracle.bspline(px, py)
    if n < 4 or n <= deg:  # "Few reference points." / fewer control points than the order (tinyspline throws)
        assert cnt == -1
        return
    tt = _parameters(length)
    assert cnt == len(tt)
    knots = np.concatenate([np.zeros(deg), np.linspace(0, 1, n - deg + 1), np.ones(deg)])
    ex, ey = np.abs(BSpline(knots, px, deg)(tt) - x).max(), np.abs(BSpline(knots, py, deg)(tt) - y).max()
    print("degree", deg, "n", n, "samples", cnt, "max |oracle - scipy|", ex, ey)
    assert ex < 1e-12 and ey < 1e-12
    chord = np.concatenate(([0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))))
    assert np.abs(chord - s).max() < 1e-12 * max(1.0, s[-1])


# ------------------------------------------------------------------ B: inputs of the four glue kernels
BS_WIDTHS = (24, 70)  # neither a multiple of 64; 70: the staging loop of the 64 lanes wraps


@functools.lru_cache(maxsize=None)
def bspline_inputs(W):
    """way_x, way_y [B, W], n_way [B], tags [B]: degrees 5 / 4 / 3 at n_way = W, 6, 5, 4 (n <= degree is refused), average spacings either side of 5 m and 10 m and
    exactly on them (3-4-5 triangles: every segment length and the average are exact), and the counts a row cannot have."""
    rows = []
    for ds in (3.0, 7.0, 12.0):
        for n in (W, 6, 5, 4):
            rows.append(("ds %g n %d" % (ds, n), *_polyline(ds, n, 0.9 / n), n))
    for ds in (4.999, 5.001, 9.999, 10.001):
        rows.append(("ds %g" % ds, *_polyline(ds, 9), 9))
    for k in (1.0, 2.0):
        rows.append(("exactly %g" % (5 * k), 3.0 * k * np.arange(9) - 11.0, 4.0 * k * np.arange(9) + 2.0, 9))
    full = _polyline(3.0, W, 0.9 / W)
    for n in (3, 0, W + 1):
        rows.append(("n_way %d" % n, *full, n))
    B = len(rows)
    wx = np.zeros((B, W)); wy = np.zeros((B, W)); nw = np.zeros(B, dtype=np.int32)
    for b, (_, x, y, n) in enumerate(rows):
        wx[b, :len(x)] = x; wy[b, :len(y)] = y; nw[b] = n
    return _frozen(dict(way_x=wx, way_y=wy, n_way=nw, tags=[r[0] for r in rows]))


def bspline_expected(oracle, W, M):
    """The oracle (in its current mode) on every row at capacity M: n [B], x, y, s [B, M] zero past the count."""
    inp = bspline_inputs(W)
    B = len(inp["n_way"])
    out = dict(n=np.zeros(B, dtype=np.int32), x=np.zeros((B, M)), y=np.zeros((B, M)), s=np.zeros((B, M)))
    for b in range(B):
        n = int(inp["n_way"][b])
        if n > W:
            out["n"][b] = -1  # more waypoints than the row holds
            continue
        cnt, x, y, s = oracle.bspline(inp["way_x"][b, :n], inp["way_y"][b, :n], cap=M)
        out["n"][b] = cnt
        if cnt > 0:
            out["x"][b, :cnt], out["y"][b, :cnt], out["s"][b, :cnt] = x, y, s
    return out


def bspline_capacities(oracle, W):
    """(generous M, m, m - 1) for m = the sample count of the row 'ds 7 n 5': shorter rows fit all three, longer ones only the first"""
    inp = bspline_inputs(W)
    r = inp["tags"].index("ds 7 n 5")
    full = max(oracle.bspline(inp["way_x"][b, :n], inp["way_y"][b, :n])[0] for b, n in enumerate(inp["n_way"]) if 4 <= n <= W)
    m = oracle.bspline(inp["way_x"][r, :5], inp["way_y"][r, :5])[0]
    return r, (full + 3, m, m - 1)


def _knots(n, ds, seed=None):
    """n knots of a smooth curve x(s), y(s): uniform spacing ds, or (seed given) spacings drawn from [0.5 ds, 1.5 ds]"""
    s = ds * np.arange(n) if seed is None else np.concatenate(([0.0], np.cumsum(np.random.default_rng(seed).uniform(0.5 * ds, 1.5 * ds, n - 1))))
    return s, s - 0.0005 * s * s, 3.0 * np.sin(s / 7.0)


def _pack(rows, K):
    B = len(rows)
    sp = dict(knot_s=np.zeros((B, K)), knot_x=np.zeros((B, K)), knot_y=np.zeros((B, K)))
    for b, (s, x, y) in enumerate(rows):
        sp["knot_s"][b, :len(s)], sp["knot_x"][b, :len(s)], sp["knot_y"][b, :len(s)] = s, x, y
    return sp


RAW_K = 96


@functools.lru_cache(maxsize=None)
def raw_inputs():
    """Splines for segmentRawReference: uniform and jittered knots, ragged counts (3; 2 and K + 1 are refused), a last knot exactly on 40.0 (41 stations), one double
    above (42: the last station lies beyond the last knot) and one below (41, the last beyond)."""
    on = np.linspace(0.0, 40.0, 81)
    up = on.copy(); up[-1] = np.nextafter(40.0, np.inf)
    dn = on.copy(); dn[-1] = np.nextafter(40.0, -np.inf)
    f = lambda s: (s, s - 0.0005 * s * s, 3.0 * np.sin(s / 7.0))
    rows = [_knots(RAW_K, 0.5), _knots(3, 1.25), _knots(RAW_K, 0.5), f(on), f(up), f(dn), _knots(RAW_K, 0.45, seed=5), _knots(50, 0.7, seed=6), _knots(RAW_K, 0.5),
            _knots(3, 0.3, seed=7)]
    nk = np.array([RAW_K, 3, 2, 81, 81, 81, RAW_K, 50, RAW_K + 1, 3], dtype=np.int32)
    return _frozen(dict(sp=_pack(rows, RAW_K), n_knots=nk, on=3, up=4, dn=5))


RAW_KEYS = ("x", "y", "s", "angle", "k")


def raw_expected(mod, sp, n_knots, P):
    """segment_raw of `mod` (the oracle in its current mode, or oracle.ref_py) on every row at capacity P: n [B], x, y, s, angle, k [B, P] zero past the count."""
    B, K = sp["knot_s"].shape
    out = dict(n=np.zeros(B, dtype=np.int32), **{k: np.zeros((B, P)) for k in RAW_KEYS})
    for b in range(B):
        nk = int(n_knots[b])
        if nk < 3 or nk > K:
            out["n"][b] = -1
            continue
        n, lists = mod.segment_raw(sp["knot_s"][b, :nk], sp["knot_x"][b, :nk], sp["knot_y"][b, :nk], cap=P)
        out["n"][b] = n
        for k, v in zip(RAW_KEYS, lists):
            out[k][b, :max(n, 0)] = v
    return out


RAW_CAPS = (64, 41, 40)  # generous; the 41 stations of a last knot at 40.0 fit exactly; one fewer


PROJ_K, PROJ_L = 96, 70


@functools.lru_cache(maxsize=None)
def project_inputs():
    """postSmooth's re-projection: layer arc lengths exactly on knots (the first and the last among them), at 0, slightly negative, beyond the last knot by up to 3 m
    (the pipeline searches up to s.back() + 3), offsets of both signs and 0; layer counts 1, L, 0, L + 1 and ragged ones either side of 64."""
    B, L = 8, PROJ_L
    rows = [_knots(PROJ_K, 0.5), _knots(PROJ_K, 0.45, seed=11), _knots(PROJ_K, 0.5), _knots(PROJ_K, 0.5), _knots(PROJ_K, 0.55, seed=12), _knots(PROJ_K, 0.5),
            _knots(PROJ_K, 0.5, seed=13), _knots(PROJ_K, 0.5)]
    nk = np.array([PROJ_K, PROJ_K, PROJ_K, PROJ_K, PROJ_K, PROJ_K, 50, PROJ_K], dtype=np.int32)
    nl = np.array([L, 1, 0, L + 1, 37, 64, 65, L], dtype=np.int32)
    rng = np.random.default_rng(21)
    ls = np.zeros((B, L)); off = rng.uniform(-1.5, 1.5, (B, L))
    for b, (s, _, _) in enumerate(rows):
        last = s[nk[b] - 1]
        on = s[np.arange(0, nk[b], 5)]  # exactly on knots: the lower_bound tie (the first knot, at == x[0], takes the in-range branch)
        edge = np.array([0.0, -1e-12, -0.3, last, last + 1e-12, last + 0.5, last + 3.0, np.nextafter(last, 0.0)])
        rest = rng.uniform(0.0, last, L - len(on) - len(edge))
        ls[b] = np.concatenate([edge, on, rest])
    off[:, 1] = 0.0; off[:, 9] = 0.0; off[7] = 0.0
    ls[1, 0] = rows[1][0][17]  # the single layer of row 1 sits on a knot
    return _frozen(dict(sp=_pack(rows, PROJ_K), n_knots=nk, n_layers=nl, layer_s=ls, off=off))


def project_expected(oracle, n_layers=None):
    """oracle.post_project row by row: x, y, s [B, L] zero past the count, length [B] (0 for a row without layers)"""
    inp = project_inputs()
    B, L = inp["layer_s"].shape
    out = dict(x=np.zeros((B, L)), y=np.zeros((B, L)), s=np.zeros((B, L)), length=np.zeros(B))
    for b in range(B):
        n = L if n_layers is None else int(n_layers[b])
        nk = int(inp["n_knots"][b])
        if n < 1 or n > L:
            continue
        x, y, s = oracle.post_project(inp["sp"]["knot_s"][b, :nk], inp["sp"]["knot_x"][b, :nk], inp["sp"]["knot_y"][b, :nk], inp["layer_s"][b, :n], inp["off"][b, :n])
        out["x"][b, :n], out["y"][b, :n], out["s"][b, :n], out["length"][b] = x, y, s, s[-1]
    return out


INIT_K = 64


@functools.lru_cache(maxsize=None)
def init_inputs():
    """segmentSmoothedPath's first half.  One path shape (31.5 m), turned and moved per row; per row a start (x, y, heading, curvature), a goal (x, y, heading), the
    length and the knot count.  Points on the path and its heading at s = 0 come from the oracle's portable mode (the very doubles the device computes: a goal
    'exactly on the end' has to be the end, a start 'exactly on the first point' the first point)."""
    from oracle import oracle_py as O

    s0, x0, y0 = _knots(INIT_K, 0.5)
    y0 = 2.0 * np.sin(s0 / 9.0)
    full = s0[-1]
    rows, start, goal, length, nk, tags = [], [], [], [], [], []

    def add(tag, th, heading, side, goal_at, goal_side=0.0, length_=full, n=INIT_K):
        """th: the turn of the path; heading: ('err', e) the start's heading error against the path, or ('abs', z); side: the start's offset along the left normal of
        the path at s = 0; goal_at, goal_side: the goal's arc length on the path and its offset to the left of it"""
        c, sn = np.cos(th), np.sin(th)
        x, y = c * x0 - sn * y0 + 3.0, sn * x0 + c * y0 - 4.0
        at = min(goal_at, full)
        with O.portable_math():
            fz = -O.segment_init(s0, x, y, full, [x[0], y[0], 0.0], [x[-1], y[-1]])[2]  # wrap(0 - heading(0))
            (gx, ax, bx), (gy, ay, by) = (O.spline_eval(s0, v, [at, at - 0.01, at + 0.01]) for v in (x, y))
        gz = np.arctan2(by - ay, bx - ax)
        sz = fz + heading[1] if heading[0] == "err" else heading[1]
        rows.append((s0, x, y))
        start.append([x[0] - side * np.sin(fz), y[0] + side * np.cos(fz), sz, 0.01])
        goal.append([gx - goal_side * np.sin(gz), gy + goal_side * np.cos(gz), gz])
        length.append(length_); nk.append(n); tags.append(tag)

    eps = 1e-9
    add("below +75", 0.3, ("err", DEG75 - eps), 0.0, full)
    add("above +75", 0.3, ("err", DEG75 + eps), 0.0, full)
    add("below -75", 0.3, ("err", -(DEG75 - eps)), 0.0, full)
    add("above -75", 0.3, ("err", -(DEG75 + eps)), 0.0, full)
    add("wrap -3.1 against +3.1", 3.1 - 0.2187, ("abs", -3.1), 0.0, 15.17)
    add("wrap +3.1 against -3.1", -3.1 - 0.2187, ("abs", 3.1), 0.3, 15.17)
    add("start left", -1.2, ("err", 0.1), 0.8, full)
    add("start right", -1.2, ("err", -0.2), -0.8, full)
    add("start on, goal the end", 2.0, ("err", 0.0), 0.0, full)
    add("goal half-way", 2.0, ("err", 0.05), 0.1, 15.17)
    add("goal 0.4 m beside 15.17", 0.7, ("err", 0.0), 0.0, 15.17, 0.4)
    add("goal 0.37 m beside 11.23", 0.7, ("err", 0.0), 0.0, 11.23, -0.37)
    add("goal 20 m aside", 0.7, ("err", 0.0), 0.0, 15.17, 20.0)
    add("goal near the start", 0.7, ("err", 0.0), -0.2, 1.8, 0.1)
    add("length 0", 0.7, ("err", 0.0), 0.0, full, length_=0.0)
    add("two knots", 0.7, ("err", 0.0), 0.0, full, n=2)
    add("shorter length", -2.5, ("err", 0.3), 0.5, 19.4, -0.4, length_=25.3)
    return _frozen(dict(sp=_pack(rows, INIT_K), n_knots=np.array(nk, dtype=np.int32), length=np.array(length), start=np.array(start), goal=np.array(goal), tags=tags))


def init_expected(oracle, exact):
    inp = init_inputs()
    B = len(inp["length"])
    out = dict(ok=np.zeros(B, dtype=np.int32), init=np.zeros((B, 3)))
    for b in range(B):
        nk = int(inp["n_knots"][b])
        r = oracle.segment_init(inp["sp"]["knot_s"][b, :nk], inp["sp"]["knot_x"][b, :nk], inp["sp"]["knot_y"][b, :nk], inp["length"][b], inp["start"][b, :3], inp["goal"][b, :2],
                                exact)
        out["ok"][b], out["init"][b] = r[0], r[1:]
    return out


def glue_expected(oracle):
    """Every part-B output of the oracle in its current mode: {name: array}; integer arrays are counts and flags, the others values."""
    out = {}
    for W in BS_WIDTHS:
        for M in bspline_capacities(oracle, W)[1]:
            for k, v in bspline_expected(oracle, W, M).items():
                out["bs%d_%d_%s" % (W, M, k)] = v
    raw = raw_inputs()
    for P in RAW_CAPS:
        for k, v in raw_expected(oracle, raw["sp"], raw["n_knots"], P).items():
            out["raw%d_%s" % (P, k)] = v
    for tag, nl in (("ragged", project_inputs()["n_layers"]), ("full", None)):
        for k, v in project_expected(oracle, nl).items():
            out["proj_%s_%s" % (tag, k)] = v
    for exact in (0, 1):
        for k, v in init_expected(oracle, exact).items():
            out["init%d_%s" % (exact, k)] = v
    return out


_GLUE = {}


def _glue(oracle, portable):
    if not _GLUE:
        _GLUE[False], _GLUE[True] = _both_modes(oracle, lambda: glue_expected(oracle))
    return _GLUE[portable]


def test_oracle_modes_agree_on_the_glue_inputs(oracle):
    """glibc mode (pinned against the reference) against portable mode (the device's arithmetic) on every part-B input: counts and flags equal, values within 1e-9."""
    a, c = _glue(oracle, False), _glue(oracle, True)
    worst = 0.0
    for k in a:
        if a[k].dtype.kind == "i":
            assert np.array_equal(a[k], c[k]), k
        else:
            worst = max(worst, float(np.abs(a[k] - c[k]).max()))
    print("worst value difference between the oracle's modes on the glue inputs", worst)
    assert worst < 1e-9


def test_glue_inputs_are_not_vacuous(oracle):
    """The inputs do what part B is about."""
    o = _glue(oracle, True)
    for W in BS_WIDTHS:
        inp = bspline_inputs(W)
        tags, nw = inp["tags"], inp["n_way"]
        deg = {t: _degree(inp["way_x"][b, :nw[b]], inp["way_y"][b, :nw[b]])[0] for b, t in enumerate(tags) if 4 <= nw[b] <= W}
        assert {deg["ds 3 n 6"], deg["ds 7 n 6"], deg["ds 12 n 6"]} == {5, 4, 3}
        assert [deg[t] for t in ("ds 4.999", "ds 5.001", "ds 9.999", "ds 10.001", "exactly 5", "exactly 10")] == [5, 4, 4, 3, 5, 4]  # `>`: exactly 5 m is degree 5
        r, (M0, M1, M2) = bspline_capacities(oracle, W)
        n0, n1, n2 = (o["bs%d_%d_n" % (W, M)] for M in (M0, M1, M2))
        want = {"ds 3 n 5": -1, "ds 3 n 4": -1, "ds 7 n 4": -1, "n_way 3": -1, "n_way 0": -1, "n_way %d" % (W + 1): -1}
        for t, v in want.items():
            assert n0[tags.index(t)] == v, t
        assert all(n0[tags.index(t)] > 4 for t in ("ds 7 n 6", "ds 12 n 4", "ds 12 n 5", "ds 3 n %d" % W, "ds 7 n %d" % W, "ds 12 n %d" % W))
        assert n1[r] == M1 and n2[r] == -2 and not o["bs%d_%d_x" % (W, M2)][r].any()  # M = m fits, M = m - 1 does not
        other = np.arange(len(tags)) != r
        assert np.array_equal(n1[other], n2[other]) and (n1 == -2).any() and ((n2 > 0) & (n2 < M2)).any()
    raw = raw_inputs()
    n64, n41, n40 = (o["raw%d_n" % P] for P in RAW_CAPS)
    assert list(n64[[raw["on"], raw["up"], raw["dn"]]]) == [41, 42, 41] and n64[1] == 4 and n64[2] == -1 and n64[8] == -1
    assert o["raw64_s"][raw["up"], 41] == 41.0 and o["raw64_s"][raw["dn"], 40] == 40.0  # stations beyond the last knot
    assert n41[raw["on"]] == 41 and n41[raw["up"]] == -2 and n40[raw["on"]] == -2 and n40[raw["dn"]] == -2 and n40[1] == 4
    p = o["proj_ragged_length"]
    assert p[1] == 0 and p[2] == 0 and p[3] == 0 and (p[[0, 4, 5, 6, 7]] > 0).all()
    i0, i1, tags = o["init0_ok"], o["init1_ok"], init_inputs()["tags"]
    assert np.array_equal(i0, i1)
    assert [int(i0[tags.index(t)]) for t in ("below +75", "above +75", "below -75", "above -75", "length 0", "two knots")] == [1, 0, 1, 0, 0, 0]
    e1 = o["init0_init"][:, 1]
    assert abs(e1[tags.index("wrap -3.1 against +3.1")]) < 0.2 and abs(e1[tags.index("wrap +3.1 against -3.1")]) < 0.2 and i0[4] and i0[5]
    e0 = o["init0_init"][:, 0]
    assert e0[tags.index("start left")] > 0.79 and e0[tags.index("start right")] < -0.79  # a vehicle left of the path has a positive offset
    on = tags.index("start on, goal the end")
    assert e0[on] == 0 and np.signbit(e0[on])  # local_y = 0 is not < 0: the offset is -min_distance = -0.0
    ln0, ln1, full = o["init0_init"][:, 2], o["init1_init"][:, 2], init_inputs()["length"]
    assert ln0[on] == full[on]  # a goal on the end: no trim
    assert ln0[tags.index("goal half-way")] in (15.0, 15.5) and ln0[tags.index("goal 20 m aside")] < full[0] and ln0[tags.index("goal near the start")] < 3
    assert (ln0 != ln1).sum() >= 3  # the 0.1 m search really changes the trim


def _close(a, b, tol):
    return a.shape == b.shape and (a.size == 0 or float(np.abs(a - b).max()) < tol)


def reference_stages(ref_py):
    """What the reference's own classes give on the part-B inputs they can express: segmentRawReference on every row with a valid knot count (no capacity there), and
    segmentSmoothedPath (FLAGS_enable_exact_position as shipped: false) on every row with a spline and a positive length, over an obstacle-free map."""
    from oracle import oracle_py as O

    raw = raw_inputs()
    out = {"raw_" + k: v for k, v in raw_expected(ref_py, raw["sp"], raw["n_knots"], 64).items()}
    m = O.make_map(np.full((700, 700), 30.0, dtype=np.float32), 0.2, 0.0, 0.0)
    inp = init_inputs()
    rows = [b for b in range(len(inp["length"])) if inp["n_knots"][b] >= 3 and inp["length"][b] > 0]
    res = [ref_py.segment_smoothed(m, inp["sp"]["knot_s"][b], inp["sp"]["knot_x"][b], inp["sp"]["knot_y"][b], inp["length"][b], inp["start"][b], inp["goal"][b])[:4] for b in rows]
    out["init_rows"] = np.array(rows, dtype=np.int32)
    out["init_ok"] = np.array([r[0] for r in res], dtype=np.int32)
    out["init_init"] = np.array([r[1:] for r in res])
    return out


def _assert_against_reference(oracle, r):
    """Counts and flags equal, values below 1e-12 (the bar of the live comparisons of tests/test_map_edges.py; the two differ in the order of one elimination)."""
    o = _glue(oracle, False)
    assert np.array_equal(o["raw64_n"], r["raw_n"])
    for k in RAW_KEYS:
        assert _close(o["raw64_" + k], r["raw_" + k], 1e-12), k
    rows = r["init_rows"]
    assert np.array_equal(o["init0_ok"][rows], r["init_ok"])
    good = r["init_ok"] == 1  # a refused start leaves the reference's vehicle state as it was: nothing to compare
    assert good.sum() >= 10 and (~good).sum() >= 2
    assert _close(o["init0_init"][rows][good], r["init_init"][good], 1e-12)
    assert np.array_equal(o["init0_init"][rows][:, 2], r["init_init"][:, 2])  # the trimmed length is one of the search's own arc lengths


@pytest.mark.skipif(not HAVE_REF, reason="reference tree not present: covered by tests/golden/glue_ref.npz instead")
def test_oracle_matches_reference_live_on_the_glue_inputs(oracle):
    from oracle import ref_py

    _assert_against_reference(oracle, reference_stages(ref_py))


def test_oracle_matches_reference_fixture_on_the_glue_inputs(oracle):
    """The same against what the reference's classes returned when tests/golden/make_glue_golden.py ran; the recorded inputs must be the ones built here."""
    g = np.load(GOLD)
    raw, inp = raw_inputs(), init_inputs()
    for k in ("knot_s", "knot_x", "knot_y"):
        assert np.array_equal(g["in_raw_" + k], raw["sp"][k]) and np.array_equal(g["in_init_" + k], inp["sp"][k]), k
    assert np.array_equal(g["in_init_start"], inp["start"]) and np.array_equal(g["in_init_goal"], inp["goal"]) and np.array_equal(g["in_init_length"], inp["length"])
    _assert_against_reference(oracle, {k: g[k] for k in g.files if not k.startswith("in_")})


# ------------------------------------------------------------------ B: the four kernels on the device
@pytest.fixture(scope="module")
def binding():
    from path_optimizer_amd import binding as b

    b.lib()
    return b


@pytest.fixture(scope="module")
def engine(binding):
    return binding.Engine(0)


def _dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.array(a)).cuda()  # (a writable copy: the cached inputs are read-only)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _spline_in(sp, n_knots, length=None):
    """(po_spline_in over device copies, the tensors it points to)"""
    t = [_dev(sp["knot_s"]), _dev(sp["knot_x"]), _dev(sp["knot_y"]), _dev(None if n_knots is None else np.asarray(n_knots, dtype=np.int32)), _dev(length)]
    B, K = sp["knot_s"].shape
    return PoSplineIn(B, K, *[_ptr(x) for x in t]), t


def _dev_bspline(binding, eng, wx, wy, n_way, M):
    B, W = wx.shape
    dx, dy, nw = _dev(wx), _dev(wy), _dev(n_way)
    out = [_dev(np.full((B, M), 7.0)) for _ in range(3)]
    n = _dev(np.full(B, 77, dtype=np.int32))
    binding._check(binding.lib().po_bspline_batch_device(eng._h, B, W, _ptr(nw), _ptr(dx), _ptr(dy), M, *[_ptr(t) for t in out], _ptr(n)))
    return dict(n=_host(n), x=_host(out[0]), y=_host(out[1]), s=_host(out[2]))


def _dev_segment_raw(binding, eng, sp, n_knots, P):
    """(rc, outputs): the outputs start as 7.0 / 77, so a call that is refused without a launch leaves them so"""
    si, keep = _spline_in(sp, n_knots)
    B = si.B
    out = [_dev(np.full((B, P), 7.0)) for _ in range(5)]
    n = _dev(np.full(B, 77, dtype=np.int32))
    rc = binding.lib().po_segment_raw_batch_device(eng._h, C.byref(si), P, *[_ptr(t) for t in out], _ptr(n))
    return rc, dict(n=_host(n), **{k: _host(t) for k, t in zip(RAW_KEYS, out)})


def _dev_post_project(binding, eng, inp, n_layers, want_length):
    si, keep = _spline_in(inp["sp"], inp["n_knots"])
    B, L = inp["layer_s"].shape
    ls, off, nl = _dev(inp["layer_s"]), _dev(inp["off"]), _dev(n_layers)
    out = [_dev(np.full((B, L), 7.0)) for _ in range(3)]
    length = _dev(np.full(B, 7.0)) if want_length else None
    binding._check(binding.lib().po_post_project_batch_device(eng._h, C.byref(si), L, _ptr(nl), _ptr(ls), _ptr(off), *[_ptr(t) for t in out], _ptr(length)))
    return dict(x=_host(out[0]), y=_host(out[1]), s=_host(out[2]), length=None if length is None else _host(length))


def _dev_segment_init(binding, eng, inp, start_stride, goal_stride):
    si, keep = _spline_in(inp["sp"], inp["n_knots"], inp["length"])
    st, gl = _dev(inp["start"][:, :start_stride]), _dev(inp["goal"][:, :goal_stride])
    init, ok = _dev(np.full((si.B, 3), 7.0)), _dev(np.full(si.B, 77, dtype=np.int32))
    binding._check(binding.lib().po_segment_init_batch_device(eng._h, C.byref(si), _ptr(st), start_stride, _ptr(gl), goal_stride, _ptr(init), _ptr(ok)))
    return dict(ok=_host(ok), init=_host(init))


def _assert_identical(got, want, keys, tag):
    """np.array_equal on every output, whole arrays: the expected ones are zero past each row's count, so this is the valid part AND the zero padding."""
    for k in keys:
        if not np.array_equal(got[k], want[k]):
            d = np.abs(got[k].astype(np.float64) - want[k]); b = int(np.argmax(d.reshape(len(d), -1).max(axis=1)))
            raise AssertionError("%s: %s differs, worst %.3e in row %d (%d entries differ)" % (tag, k, d.max(), b, int((got[k] != want[k]).sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("W", BS_WIDTHS)
def test_device_bspline_is_bit_identical_to_the_portable_oracle(binding, engine, oracle, W):
    """bspline_kernel on one batch mixing the three degrees, the refusals and ragged counts, at a generous capacity, at M = m of one row (fits) and M = m - 1 (that row
    alone turns -2 with a zero row)."""
    inp = bspline_inputs(W)
    o = _glue(oracle, True)
    r, caps = bspline_capacities(oracle, W)
    for M in caps:
        got = _dev_bspline(binding, engine, inp["way_x"], inp["way_y"], inp["n_way"], M)
        _assert_identical(got, {k: o["bs%d_%d_%s" % (W, M, k)] for k in ("n", "x", "y", "s")}, ("n", "x", "y", "s"), "W %d M %d" % (W, M))
    rows = [b for b, n in enumerate(inp["n_way"]) if n == W]  # n_way = NULL means W everywhere
    a = _dev_bspline(binding, engine, inp["way_x"][rows], inp["way_y"][rows], None, caps[0])
    c = _dev_bspline(binding, engine, inp["way_x"][rows], inp["way_y"][rows], np.full(len(rows), W, dtype=np.int32), caps[0])
    for k in a:
        assert a[k].tobytes() == c[k].tobytes() and np.array_equal(a[k], o["bs%d_%d_%s" % (W, caps[0], k)][rows]), k


@pytest.mark.gpu
def test_device_segment_raw_is_bit_identical_to_the_portable_oracle(binding, engine, oracle):
    raw = raw_inputs()
    o = _glue(oracle, True)
    for P in RAW_CAPS:
        rc, got = _dev_segment_raw(binding, engine, raw["sp"], raw["n_knots"], P)
        assert rc == 0
        _assert_identical(got, {k: o["raw%d_%s" % (P, k)] for k in ("n",) + RAW_KEYS}, ("n",) + RAW_KEYS, "P %d" % P)


@pytest.mark.gpu
def test_device_segment_raw_at_the_largest_spline_that_fits(binding, engine, oracle):
    """15 K doubles of LDS: K = 546 is the largest the 64 KB check admits (bit-identical to the oracle, uniform and jittered knots), K = 547 is refused
    with PO_ERR_UNSUPPORTED before anything is launched (the outputs keep what they held)."""
    assert 15 * 8 * 546 <= 64 * 1024 < 15 * 8 * 547
    sp = _pack([_knots(546, 0.5), _knots(546, 0.5, seed=31)], 546)
    nk = np.array([546, 546], dtype=np.int32)
    P = 300
    rc, got = _dev_segment_raw(binding, engine, sp, nk, P)
    assert rc == 0
    with oracle.portable_math():
        want = raw_expected(oracle, sp, nk, P)
    assert (want["n"] > 250).all()
    _assert_identical(got, want, ("n",) + RAW_KEYS, "K 546")
    rc, got = _dev_segment_raw(binding, engine, _pack([_knots(547, 0.5)], 547), np.array([547], dtype=np.int32), P)
    assert rc == PO_ERR_UNSUPPORTED and got["n"][0] == 77 and all((got[k] == 7.0).all() for k in RAW_KEYS)


@pytest.mark.gpu
def test_device_post_project_is_bit_identical_to_the_portable_oracle(binding, engine, oracle):
    inp = project_inputs()
    o = _glue(oracle, True)
    got = _dev_post_project(binding, engine, inp, inp["n_layers"], True)
    _assert_identical(got, {k: o["proj_ragged_" + k] for k in got}, ("x", "y", "s", "length"), "ragged")
    got = _dev_post_project(binding, engine, inp, None, False)  # n_layers = NULL: L everywhere; length_out = NULL
    _assert_identical(got, {k: o["proj_full_" + k] for k in got}, ("x", "y", "s"), "full")


@pytest.mark.gpu
@pytest.mark.parametrize("exact", (0, 1))
def test_device_segment_init_is_bit_identical_to_the_portable_oracle(binding, oracle, exact):
    """Offsets, heading errors and trimmed lengths to the bit, the sign of a zero offset included; strides (4, 3) and (3, 2) read the same values."""
    p = binding.default_params()
    p.enable_exact_position = exact
    eng = binding.Engine(0, p)
    inp = init_inputs()
    o = _glue(oracle, True)
    got = _dev_segment_init(binding, eng, inp, 4, 3)
    assert np.array_equal(got["ok"], o["init%d_ok" % exact])
    want = o["init%d_init" % exact]
    assert np.array_equal(got["init"], want)
    assert got["init"].tobytes() == want.tobytes()  # -0.0 is not +0.0 here
    tight = _dev_segment_init(binding, eng, inp, 3, 2)
    assert tight["ok"].tobytes() == got["ok"].tobytes() and tight["init"].tobytes() == got["init"].tobytes()


# ------------------------------------------------------------------ C: po_plan_batch with mixed outcomes in one call
PLAN_W, PLAN_N = 16, 200
PLAN_LONG = 2
PLAN_MAX_LENGTH = 39.0  # an explicit max_length that is too small for the one instance with 16 waypoints (45 m)
PLAN_K0 = (0.1, 0.22, 0.0, 0.23, 0.13, 0.24, 0.16, 0.26, 0.2, 0.3)  # curvature at the start: <= 0.2 gives keep 3, >= 0.22 keep 4
PLAN_NWAY = (14, 13, 16, 14, 12, 12, 13, 13, 14, 12)  # only the straight instance (PLAN_LONG) has 16 waypoints: the one that is too long for PLAN_MAX_LENGTH


@functools.lru_cache(maxsize=None)
def plan_map():
    return _frozen((np.full((700, 700), 30.0, dtype=np.float32), 0.2, 0.0, 0.0))


def _plan_instance(k0, nway, ds=3.0):
    """Waypoints every `ds` on a curve of curvature k0 exp(-s / 12) (midpoint rule on a fine grid), the start on the first with the curve's heading and curvature 0,
    the goal on the last."""
    s = np.linspace(0, ds * (nway - 1), 40 * nway)
    kk = k0 * np.exp(-s / 12.0)
    z = np.concatenate(([0.0], np.cumsum(0.5 * (kk[1:] + kk[:-1]) * np.diff(s))))
    x = np.concatenate(([0.0], np.cumsum(np.cos(0.5 * (z[1:] + z[:-1])) * np.diff(s)))) - 20
    y = np.concatenate(([0.0], np.cumsum(np.sin(0.5 * (z[1:] + z[:-1])) * np.diff(s)))) - 20
    idx = np.searchsorted(s, ds * np.arange(nway)).clip(0, len(s) - 1)
    return x[idx], y[idx], np.array([x[0], y[0], z[0], 0.0]), np.array([x[idx[-1]], y[idx[-1]], z[idx[-1]]])


def _plan_pack(inst):
    """[(wx, wy, start, goal)] -> way_x, way_y [B, W] zero padded, n_way, start [B, 4], goal [B, 3]"""
    B = len(inst)
    wx = np.zeros((B, PLAN_W)); wy = np.zeros((B, PLAN_W)); nw = np.zeros(B, dtype=np.int32)
    for b, (x, y, _, _) in enumerate(inst):
        wx[b, :len(x)] = x; wy[b, :len(y)] = y; nw[b] = len(x)
    return dict(way_x=wx, way_y=wy, n_way=nw, start=np.array([i[2] for i in inst]), goal=np.array([i[3] for i in inst]))


@functools.lru_cache(maxsize=None)
def plan_instances():
    return _frozen([_plan_instance(k0, n) for k0, n in zip(PLAN_K0, PLAN_NWAY)])


def plan_early_stops():
    """The three ways of _variants (tests/test_pipeline.py) to stop early, on instance 4: (instance, stage)"""
    x, y, st, gl = plan_instances()[4]
    turned = st.copy(); turned[2] += 1.6
    far = st.copy(); far[0] += 30 * np.cos(st[2] + 1.5708); far[1] += 30 * np.sin(st[2] + 1.5708)
    return [((x[:3], y[:3], st, gl), 1), ((x, y, turned, gl), 5), ((x, y, far, gl), 3)]


def _oracle_plan(oracle, inst, exact=0):
    """path_optimizer_solve of the oracle in its current mode: dict(ok, path, keep, nv, iters)"""
    p = oracle.default_params()
    p.enable_exact_position = exact
    ok, path, tr = oracle.path_optimizer_solve(p, oracle.make_map(*plan_map()), *inst)
    out = dict(ok=bool(ok), path=path, keep=0, nv=0, iters=-1)
    if "reference" in tr:
        qs, nv = tr["reference"][4], tr["reference"][5]
        out.update(nv=nv, keep=oracle.keep_steps(0, qs[:nv]) if nv >= 2 else 0)
    if "qp" in tr:
        out["iters"] = int(tr["qp"]["iters"])
    return out


_PLAN = {}


def _plan_oracle(oracle, portable=False):
    if portable not in _PLAN:
        if portable:
            with oracle.portable_math():
                _PLAN[portable] = [_oracle_plan(oracle, i) for i in plan_instances()]
        else:
            _PLAN[portable] = [_oracle_plan(oracle, i) for i in plan_instances()]
    return _PLAN[portable]


def test_plan_batch_precondition_two_keep_groups(oracle):
    """What part C rests on, from the oracle's trace: two distinct keeps, at least four solved instances each, unequal n_valid inside each group, and in each group a
    first member that is not the longest (Ng is the maximum over the group, not the first member's count)."""
    o = _plan_oracle(oracle)
    assert all(r["ok"] for r in o)
    groups = {}
    for r in o:
        groups.setdefault(r["keep"], []).append(r["nv"])
    print("keep -> n_valid", groups, "states", [len(r["path"]) for r in o])
    assert sorted(groups) == [3, 4]
    for nv in groups.values():
        assert len(nv) >= 4 and len(set(nv)) > 1 and nv[0] < max(nv)
    n = [len(r["path"]) for r in o]
    assert max(n) <= PLAN_N and n.count(max(n)) == 1


def test_oracle_modes_agree_on_the_plan_inputs(oracle):
    """The two modes on every part-C instance: verdicts, counts, keeps and QP iteration counts equal, states within 1e-9."""
    a, c = _plan_oracle(oracle, False), _plan_oracle(oracle, True)
    worst = 0.0
    for u, v in zip(a, c):
        assert (u["ok"], u["keep"], u["nv"], u["iters"], u["path"].shape) == (v["ok"], v["keep"], v["nv"], v["iters"], v["path"].shape)
        worst = max(worst, float(np.abs(u["path"] - v["path"]).max()))
    print("worst state difference between the oracle's modes on the plan inputs", worst)
    assert worst < 1e-9


@pytest.fixture(scope="module")
def plan_engine(binding):
    e = binding.Engine(0)
    e.set_map(*plan_map())
    return e


def _run(eng, t, N=PLAN_N, max_length=0.0):
    return dict(zip(("states", "n", "ok", "stage", "info"), eng.plan_batch(t["way_x"], t["way_y"], t["start"], t["goal"], N=N, n_way=t["n_way"], max_length=max_length)))


def _rows(t, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in t.items()}


def _same_bytes(a, b, ia, ib, tag):
    for k in ("states", "n", "ok", "stage", "info"):
        assert a[k][ia].tobytes() == b[k][ib].tobytes(), (tag, k)


_BASE = {}


def _base(plan_engine):
    """The batch of plan_instances() through the host entry, computed once and left unchanged."""
    if not _BASE:
        _BASE.update(_frozen(_run(plan_engine, _plan_pack(plan_instances()))))
    return _BASE


@pytest.mark.gpu
def test_device_plan_two_keep_groups_match_the_oracle(plan_engine, oracle):
    """The bars of tests/test_pipeline.py per instance, on a batch whose path QPs run as two launches (keep 3 and keep 4) over ragged groups."""
    o = _plan_oracle(oracle)
    r = _base(plan_engine)
    off = []
    for b, want in enumerate(o):
        assert bool(r["ok"][b]) == want["ok"] and r["n"][b] == len(want["path"]) and r["stage"][b] == 0, (b, r["stage"][b])
        assert not r["states"][b, r["n"][b]:].any()
        err = float(np.abs(r["states"][b, :r["n"][b]] - want["path"]).max())
        same = int(r["info"]["iters"][b]) == want["iters"]
        print("instance", b, "keep", want["keep"], "n", r["n"][b], "iters", int(r["info"]["iters"][b]), want["iters"], "max |device - oracle|", err)
        if same:
            assert err < 1e-6, b
        else:  # a termination check within round-off of eps
            off.append(b)
            assert err < 1e-5, b
    assert len(off) <= 1, off


@pytest.mark.gpu
def test_device_plan_does_not_depend_on_the_order_of_the_batch(plan_engine):
    """Every instance has the same bytes in states, n, ok, stage and info wherever it stands in the batch (a permutation keeps the members of each keep group and so each
    group's Ng), and with instances in between that stop at stages 1, 5 and 3: those come back with their stage, no states and PO_STATUS_UNSOLVED.  Alone, an
    instance's QP has another padded length (Ng), which the class-level scaling depends on: compared at 1e-6."""
    inst = plan_instances()
    base = _base(plan_engine)
    perm = np.array([7, 2, 9, 0, 5, 4, 1, 8, 3, 6])
    r = _run(plan_engine, _plan_pack([inst[i] for i in perm]))
    for j, i in enumerate(perm):
        _same_bytes(r, base, j, i, ("permuted", i))
    stops = plan_early_stops()
    mixed = [inst[0], stops[0][0], inst[1], inst[2], stops[1][0]] + list(inst[3:7]) + [stops[2][0]] + list(inst[7:])
    where = [0, 2, 3, 5, 6, 7, 8, 10, 11, 12]
    r = _run(plan_engine, _plan_pack(mixed))
    for i, j in enumerate(where):
        _same_bytes(r, base, j, i, ("with early stops", i))
    for j, (_, stage) in zip((1, 4, 9), stops):
        assert r["stage"][j] == stage and r["n"][j] == 0 and r["ok"][j] == 0 and not r["states"][j].any() and r["info"]["status"][j] == PO_STATUS_UNSOLVED, (j, r["stage"][j])
    alone = _run(plan_engine, _plan_pack([inst[3]]))
    assert alone["n"][0] == base["n"][3] and alone["ok"][0] == 1 and np.abs(alone["states"][0] - base["states"][3]).max() < 1e-6


@pytest.mark.gpu
def test_device_plan_max_length_too_small_for_one_instance(plan_engine, oracle):
    """max_length = 39 sizes the intermediate rows for 45 samples: the straight 45 m instance overflows them (stage 9, nothing written), every other instance comes
    out as in a batch without it at the same max_length, byte for byte."""
    inst = plan_instances()
    cap = int(np.ceil(PLAN_MAX_LENGTH)) + 6
    counts = np.array([oracle.bspline(i[0], i[1], cap=cap)[0] for i in inst])
    others = np.arange(len(inst)) != PLAN_LONG
    assert counts[PLAN_LONG] == -2 and 0 < counts[others].min() and counts[others].max() < cap - 4  # the B-spline samples of that instance alone do not fit
    full = _run(plan_engine, _plan_pack(inst), max_length=PLAN_MAX_LENGTH)
    rest = _run(plan_engine, _plan_pack([i for b, i in enumerate(inst) if b != PLAN_LONG]), max_length=PLAN_MAX_LENGTH)
    b = PLAN_LONG
    assert full["stage"][b] == 9 and full["n"][b] == 0 and full["ok"][b] == 0 and not full["states"][b].any() and full["info"]["status"][b] == PO_STATUS_UNSOLVED
    assert not full["stage"][others].any() and full["ok"][others].all()
    for j, b in enumerate(np.flatnonzero(others)):
        _same_bytes(full, rest, b, j, ("max_length", b))


@pytest.mark.gpu
def test_device_plan_state_capacity_one_short_for_one_instance(plan_engine):
    """N equal to the longest instance's state count: everything fits.  One less: that instance alone is stage 9 (the host rewrites its stage 6 and uploads the stages
    again), the others are unchanged to the byte."""
    base = _base(plan_engine)
    big = int(np.argmax(base["n"]))
    N = int(base["n"][big])
    t = _plan_pack(plan_instances())
    fit = _run(plan_engine, t, N=N)
    assert not fit["stage"].any() and fit["ok"].all() and np.array_equal(fit["n"], base["n"])
    short = _run(plan_engine, t, N=N - 1)
    others = np.arange(len(base["n"])) != big
    assert short["stage"][big] == 9 and short["n"][big] == 0 and short["ok"][big] == 0 and not short["states"][big].any() and short["info"]["status"][big] == PO_STATUS_UNSOLVED
    assert not short["stage"][others].any() and short["ok"][others].all()
    for b in np.flatnonzero(others):
        assert short["states"][b].tobytes() == fit["states"][b, :N - 1].tobytes() and not fit["states"][b, N - 1:].any(), b
        for k in ("n", "ok", "stage", "info"):
            assert short[k][b].tobytes() == fit[k][b].tobytes(), (b, k)


@pytest.mark.gpu
def test_device_plan_device_entry_and_optional_outputs(binding, plan_engine):
    """po_plan_batch_device on device copies of the batch gives the bytes of the host entry (same explicit max_length); with stage and info NULL it uses slots of its
    own and gives the same states, counts and verdicts."""
    import torch

    t = _plan_pack(plan_instances())
    host = _run(plan_engine, t, max_length=50.0)
    assert host["ok"].all()
    B = len(t["n_way"])
    dt = {k: _dev(v) for k, v in t.items()}
    isz = host["info"].dtype.itemsize

    def outputs():
        return dict(states=_dev(np.full((B, PLAN_N, 5), 7.0)), n_states=_dev(np.full(B, 77, dtype=np.int32)), ok=_dev(np.full(B, 77, dtype=np.int32)),
                    stage=_dev(np.full(B, 77, dtype=np.int32)), info=torch.zeros((B, isz), dtype=torch.uint8, device="cuda"))

    out = outputs()
    plan_engine.plan_batch_device(dt, out, PLAN_N, 50.0)
    got = {k: _host(v) for k, v in out.items()}
    assert got["states"].tobytes() == host["states"].tobytes() and got["n_states"].tobytes() == host["n"].tobytes() and got["ok"].tobytes() == host["ok"].tobytes()
    assert got["stage"].tobytes() == host["stage"].tobytes() and got["info"].tobytes() == host["info"].tobytes()
    out = outputs()
    pi = PoPlanIn(B, PLAN_W, _ptr(dt["n_way"]), _ptr(dt["way_x"]), _ptr(dt["way_y"]), _ptr(dt["start"]), _ptr(dt["goal"]), 50.0, PLAN_N)
    po = PoPlanOut(_ptr(out["states"]), _ptr(out["n_states"]), _ptr(out["ok"]), None, None)
    binding._check(binding.lib().po_plan_batch_device(plan_engine._h, C.byref(pi), C.byref(po)))
    got = {k: _host(v) for k, v in out.items()}
    assert got["states"].tobytes() == host["states"].tobytes() and got["n_states"].tobytes() == host["n"].tobytes() and got["ok"].tobytes() == host["ok"].tobytes()
    assert (got["stage"] == 77).all() and not got["info"].any()  # not passed: not written


EXACT_GOALS = ((2, 0.45, 0.4), (3, 0.5, -0.4), (4, 0.55, 0.4), (8, 0.4, -0.4))  # (instance, fraction of the path, offset to the left): goals 0.4 m off the path half-way


def exact_instances():
    out = []
    for i, frac, side in EXACT_GOALS:
        x, y, st, gl = plan_instances()[i]
        j = int(frac * (len(x) - 1))
        px, py = x[j] + frac * (x[j + 1] - x[j]), y[j] + frac * (y[j + 1] - y[j])
        hz = np.arctan2(y[j + 1] - y[j], x[j + 1] - x[j])
        out.append((x, y, st, np.array([px - side * np.sin(hz), py + side * np.cos(hz), hz])))
    return out


@pytest.mark.gpu
def test_device_plan_with_exact_position(binding, plan_engine, oracle):
    """enable_exact_position = 1 through the whole device pipeline (the 0.1 m goal search of segment_init_kernel): verdicts and counts equal to the oracle's, states within
    1e-6, and the flag changes the count of at least one of the goals against the same batch with the flag off."""
    p = binding.default_params()
    p.enable_exact_position = 1
    eng = binding.Engine(0, p)
    eng.set_map(*plan_map())
    inst = exact_instances()
    t = _plan_pack(inst)
    on, off = _run(eng, t), _run(plan_engine, t)
    for b, i in enumerate(inst):
        want = _oracle_plan(oracle, i, exact=1)
        assert want["ok"] and bool(on["ok"][b]) and on["stage"][b] == 0 and on["n"][b] == len(want["path"]), (b, on["stage"][b], on["n"][b], len(want["path"]))
        err = float(np.abs(on["states"][b, :on["n"][b]] - want["path"]).max())
        print("goal", b, "n with the flag", on["n"][b], "without", off["n"][b], "max |device - oracle|", err)
        assert err < 1e-6, b
    assert off["ok"].all() and (on["n"] != off["n"]).any()
