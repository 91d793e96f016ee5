"""The map-reading stages at the map's edge, on non-square layers, and in both launch variants of the DP lattice search.

Map sampling, the corridor bounds, the DP search, the collision check and the densifying output are held to bit equality with the oracle's portable-math mode
(tests/test_pmath.py).  Here that bar is applied where a wrong extent, stride or border rule shows:
  A. a deterministic lattice of probes on tiny and non-square layers of arbitrary distinct values: every cell centre, corner and edge midpoint, the border ring and
     the four corners moved by one and two ulps, a ring one cell outside;
  B. bounds, search, collision check and densifying output on two small non-square layers (260 x 170 and 170 x 260 cells) that every path leaves;
  C. dp_search_kernel<1>: forced by the switch, picked above 512 instances, and picked because the eight-wave reduction scratch no longer fits in LDS.
CPU legs: the oracle's two arithmetic modes agree on these inputs (so the device, compared with the portable mode, is tied to the mode pinned against the reference),
the oracle against the reference's own classes (live where the reference tree exists, through tests/golden/edge_ref.npz everywhere).  Helpers are local to this file;
tests/golden/make_edge_golden.py imports the scene from here."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from path_optimizer_amd import synth
from path_optimizer_amd.abi import INFO_DTYPE, PO_ERR_UNSUPPORTED

HAVE_REF = os.path.isdir("/root/reference")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_ref.npz")
REF_KEYS = ("ref_x", "ref_y", "ref_z", "ref_s")
KNOT_KEYS = ("knot_s", "knot_x", "knot_y")

# ------------------------------------------------------------------ A: the probe lattice
A_SIZES = ((1, 1), (1, 7), (7, 1), (2, 3), (37, 23), (23, 37))
A_RES = (0.25, 0.2)
A_POS = ((1.3, -0.7), (-2.1, 3.4), (17.35, -40.15))  # layer centres, none a multiple of a resolution; the first is the single map's
A_CASES = [(sx, sy, res) for sx, sy in A_SIZES for res in A_RES]


def _frozen(obj):
    """obj with every numpy array in it marked read-only: the cached scenes below are shared by the tests and by tests/golden/make_edge_golden.py."""
    if isinstance(obj, np.ndarray):
        obj.setflags(write=False)
    elif isinstance(obj, dict):
        for v in obj.values():
            _frozen(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _frozen(v)
    return obj


def _layer_values(seed, sx, sy):
    """Distinct float32 values in no order at all (not a distance field): reading a wrong neighbour changes the result."""
    rng = np.random.default_rng(seed)
    return (0.5 + 0.125 * rng.permutation(sx * sy)).astype(np.float32).reshape(sx, sy)


def _steps(v, k):
    """v moved by k representable doubles (k < 0: downwards)."""
    v = np.asarray(v, dtype=np.float64).copy()
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def _lattice(sx, sy, res, px, py):
    """Half-cell lattice from one cell outside the layer to one cell outside: hx, hy count half cells from the layer's largest x and y (even: a cell boundary,
    odd: a cell centre; 0 and 2 * size: the border).  Returns xs [nx], ys [ny], hx, hy."""
    hx, hy = np.arange(-2, 2 * sx + 3), np.arange(-2, 2 * sy + 3)
    return px + 0.5 * (sx * res) - 0.5 * hx * res, py + 0.5 * (sy * res) - 0.5 * hy * res, hx, hy


def _centres(sx, sy, res, px, py):
    """Cell centres as getPositionFromIndex computes them (the very expression, so that a probe sits ON the centre and not a rounding error beside it)."""
    return ((px + (0.5 * (sx * res) - 0.5 * res)) + res * -np.arange(sx, dtype=np.float64), (py + (0.5 * (sy * res) - 0.5 * res)) + res * -np.arange(sy, dtype=np.float64))


def _probes(sx, sy, res, px, py):
    """[n, 2]: every lattice point (cell centres, corners, edge midpoints, the ring outside), then every point of the border ring (the corners among them) moved by
    -2 .. 2 doubles on each axis, then the cell centres in the library's own arithmetic."""
    xs, ys, hx, hy = _lattice(sx, sy, res, px, py)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    HX, HY = np.meshgrid(hx, hy, indexing="ij")
    CX, CY = np.meshgrid(*_centres(sx, sy, res, px, py), indexing="ij")
    pts = [np.stack([X.ravel(), Y.ravel()], axis=1), np.stack([CX.ravel(), CY.ravel()], axis=1)]
    on = (HX >= 0) & (HX <= 2 * sx) & (HY >= 0) & (HY <= 2 * sy)
    ring = on & ((HX == 0) | (HX == 2 * sx) | (HY == 0) | (HY == 2 * sy))
    rx, ry = X[ring], Y[ring]
    for i in range(-2, 3):
        for j in range(-2, 3):
            if i or j:
                pts.append(np.stack([_steps(rx, i), _steps(ry, j)], axis=1))
    return np.concatenate(pts)


@functools.lru_cache(maxsize=None)
def _a_case(sx, sy, res):
    """Three layers of one geometry with centres A_POS (layer 0 doubles as the single map) and the probes of each."""
    seed = 7000 + 100 * sx + sy
    layers = np.stack([_layer_values(seed + k, sx, sy) for k in range(3)])
    return _frozen((layers, [_probes(sx, sy, res, *A_POS[k]) for k in range(3)]))


_A_ORACLE = {}


def _a_oracle(oracle, sx, sy, res, k):
    """oracle.map_distance of layer k's probes, computed once (map sampling has no trigonometry: the oracle's two modes are one here)."""
    key = (sx, sy, res, k)
    if key not in _A_ORACLE:
        layers, probes = _a_case(sx, sy, res)
        _A_ORACLE[key] = oracle.map_distance(oracle.make_map(layers[k], res, *A_POS[k]), probes[k])
    return _A_ORACLE[key]


@pytest.mark.parametrize("sx,sy,res", A_CASES)
def test_oracle_cell_centres_return_the_stored_cell(oracle, sx, sy, res):
    """Which cell (i, j) a position means: cell (0, 0) at the largest x and y, i along x, j along y, on layers with size_x != size_y.  On a cell centre the bilinear
    weights are 1 and 0 (or the nearest-cell fall-back answers, on the border cells), so the result is the stored value itself.
    The centre has to be the library's own (getPositionFromIndex): grid_map's interpolation picks the neighbour by `position >= centre`, and in the last row or
    column a position one rounding error BELOW the centre selects a neighbour index outside the layer, for which getPosition leaves the centre where it was — the
    weights then swap and the value of linear index + 1 comes back (0 past the buffer).  The oracle restates that (seen here on the 2 x 3 layer at 0.2: cell (1, 1)
    read as cell (0, 2), cell (1, 2) as 0); the half-cell lattice of _probes holds such points and the device is held to the same answers."""
    layers, _ = _a_case(sx, sy, res)
    for k in range(3):
        X, Y = np.meshgrid(*_centres(sx, sy, res, *A_POS[k]), indexing="ij")
        d, ins = oracle.map_distance(oracle.make_map(layers[k], res, *A_POS[k]), np.stack([X.ravel(), Y.ravel()], axis=1))
        assert ins.all()
        assert np.array_equal(d.reshape(sx, sy), layers[k].astype(np.float64))


@pytest.mark.parametrize("sx,sy,res", A_CASES)
def test_oracle_edge_lattice_inside_is_half_open(oracle, sx, sy, res):
    """checkIfPositionWithinMap on the lattice: the border at the largest x / y belongs to the layer, the one at the smallest does not, the ring outside is outside
    and reads 0 (Map.cpp:20-21); two doubles either side of a border decide as their side does."""
    d, ins = _a_oracle(oracle, sx, sy, res, 0)
    xs, ys, hx, hy = _lattice(sx, sy, res, *A_POS[0])
    n = len(hx) * len(hy)
    HX, HY = np.meshgrid(hx, hy, indexing="ij")
    strictly = ((HX > 0) & (HX < 2 * sx) & (HY > 0) & (HY < 2 * sy)).ravel()
    outside = ((HX < 0) | (HX > 2 * sx) | (HY < 0) | (HY > 2 * sy)).ravel()
    assert ins[:n][strictly].all() and not ins[:n][outside].any() and not d[:n][outside].any()
    assert not d[ins == 0].any()
    moved = ins[n + sx * sy:]
    assert 0 < moved.mean() < 1  # the moved border points fall on both sides


@pytest.mark.skipif(not HAVE_REF, reason="reference tree not present")
@pytest.mark.parametrize("sx,sy,res", A_CASES)
def test_oracle_edge_lattice_matches_reference_live(oracle, sx, sy, res):
    """Map::getObstacleDistance of the reference's own Map.cpp on every probe.  The stand-in grid_map of oracle/ref_shim forwards to the oracle's restatement (grid_map
    itself is not part of the reference tree: "parity unpinned"), so what this pins is Map.cpp's logic around it: isInside first, 0 outside."""
    from oracle import ref_py

    layers, probes = _a_case(sx, sy, res)
    m = oracle.make_map(layers[0], res, *A_POS[0])
    d, _ = _a_oracle(oracle, sx, sy, res, 0)
    r = np.array([ref_py.map_distance(m, float(x), float(y)) for x, y in probes[0]])
    assert np.array_equal(d, r)


@pytest.mark.gpu
@pytest.mark.parametrize("sx,sy,res", A_CASES)
def test_device_edge_lattice_matches_oracle(oracle, sx, sy, res):
    """Engine.map_sample on the single map and map_sample_layer on a three-layer stack with per-layer centres: dist and inside bit-identical to the oracle on every
    probe (the bar of test_device_map_sampling_matches_oracle)."""
    from path_optimizer_amd import binding

    layers, probes = _a_case(sx, sy, res)
    eng = binding.Engine(0)
    eng.set_map(layers[0], res, *A_POS[0])
    d, ins = eng.map_sample(probes[0])
    od, oins = _a_oracle(oracle, sx, sy, res, 0)
    assert np.array_equal(ins, oins) and np.array_equal(d, od)
    eng.set_map_stack(layers, res, pos_xy=np.array(A_POS))
    assert eng.debug_get("map_layers") == 3
    for k in range(3):
        d, ins = eng.map_sample_layer(k, probes[k])
        od, oins = _a_oracle(oracle, sx, sy, res, k)
        assert np.array_equal(ins, oins) and np.array_equal(d, od), k


# ------------------------------------------------------------------ B: the stages on small non-square layers that the paths leave
B_RES = 0.2
B_LAYERS = {"wide": dict(size_x=260, size_y=170, pos=(1.3, -0.7), seed=41), "tall": dict(size_x=170, size_y=260, pos=(-2.1, 3.4), seed=42)}
B_SCENES = [(name, fill) for name in B_LAYERS for fill in ("discs", "free")]
B_NB, B_N, B_CAP = 32, 200, 64
B_SEED_PATHS, B_SEED_SEARCH = 900, 901
B_DENSE_M, B_DENSE_SMALL = 200, 30


def _arc_length(states):
    """states[..., 4] = the running arc length exactly as the output map / optimizePath accumulate it"""
    st = states.copy()
    for b in range(st.shape[0]):
        s = 0.0
        for i in range(1, st.shape[1]):
            dx, dy = st[b, i, 0] - st[b, i - 1, 0], st[b, i, 1] - st[b, i - 1, 1]
            s += np.sqrt(dx * dx + dy * dy)
            st[b, i, 4] = s
    return st


def _densify(oracle, p, m, states, status, cap):
    """oracle.densify with the count as the C function reports it (-2: the capacity was met before any collision): (ok, n, out [max(n, 0), 5])."""
    st = np.ascontiguousarray(states, dtype=np.float64)
    out = np.zeros((cap, 5)); n = C.c_int(0)
    ok = oracle.lib().po_oracle_densify(C.byref(p), C.byref(m), st.shape[0], st.ctypes.data_as(C.c_void_p), int(status), cap, out.ctypes.data_as(C.c_void_p), C.byref(n))
    return ok, n.value, out[:max(n.value, 0)]


def _solved(B):
    info = np.zeros(B, dtype=INFO_DTYPE)
    info["status"] = 1
    return info


@functools.lru_cache(maxsize=None)
def edge_layer(name, fill):
    """(dist [size_x, size_y] float32, resolution, pos_x, pos_y) of one part-B layer: a dozen discs, or obstacle-free (every cell 10.0: whatever truncates a path
    there is the border's doing)."""
    kw = B_LAYERS[name]
    if fill == "free":
        return _frozen((np.full((kw["size_x"], kw["size_y"]), 10.0, dtype=np.float32), B_RES, kw["pos"][0], kw["pos"][1]))
    return _frozen(synth.make_distance_map(kw["seed"], size_x=kw["size_x"], size_y=kw["size_y"], resolution=B_RES, pos=kw["pos"], n_obstacles=12, r_range=(0.5, 2.0))[:4])


@functools.lru_cache(maxsize=None)
def edge_inputs(name):
    """Every input of part B on layer `name` (the two fillings share them)."""
    kw = B_LAYERS[name]
    px, py = kw["pos"]
    hx, hy = 0.5 * kw["size_x"] * B_RES, 0.5 * kw["size_y"] * B_RES
    P = synth.make_spline_paths(B_SEED_PATHS, B_NB, B_N)
    npts = np.full(B_NB, B_N, dtype=np.int32)
    npts[::4] = 30  # every fourth path is 8.7 m long: short enough to end inside the layer
    sp, length, start = synth.make_search_inputs(B_SEED_SEARCH, B_NB)
    # collision check: 8 x 64 states over the layer's extent plus 3 m on every side, headings in (-pi, pi]
    rng = np.random.default_rng(4300 + kw["seed"])
    st = np.zeros((8, 64, 5))
    st[..., 0] = rng.uniform(px - hx - 3.0, px + hx + 3.0, (8, 64))
    st[..., 1] = rng.uniform(py - hy - 3.0, py + hy + 3.0, (8, 64))
    st[..., 2] = -rng.uniform(-np.pi, np.pi, (8, 64))
    # batch 7 runs along the border at the largest x, from 2.6 m inside (under the bounding radius sqrt(2.45^2 + 1) = 2.646) to 0.4 m outside, heading along the
    # border, out of the layer and into it in turn
    t = np.arange(64)
    st[7, :, 0] = px + hx - np.linspace(2.6, -0.4, 64)
    st[7, :, 1] = py - hy + 1.0 + (2 * hy - 2.0) * t / 63.0
    st[7, :, 2] = np.array([np.pi / 2, 0.0, np.pi, -np.pi / 2])[t % 4]
    st = _arc_length(st)
    post_npts = np.array([64, 40, 64, 1, 64, 17, 64, 50], dtype=np.int32)
    post_info = _solved(8); post_info["status"][2] = -2; post_info["status"][6] = 0
    # densifying output: solved paths from near the centre across the border in eight directions (the border is 17 .. 26 m away), one of them unsolved
    nd = 60
    u = np.linspace(0.0, 1.0, nd)
    dn = np.zeros((8, nd, 5))
    for k in range(8):
        th = 0.2 + k * np.pi / 4
        along = 42.0 * u
        side = 0.6 * np.sin(3.0 * u + k)
        dn[k, :, 0] = px + 0.7 * np.cos(k) + along * np.cos(th) - side * np.sin(th)
        dn[k, :, 1] = py + 0.7 * np.sin(k) + along * np.sin(th) + side * np.cos(th)
    dn = _arc_length(dn)
    dn_info = _solved(8); dn_info["status"][5] = -3
    return _frozen(dict(P=P, npts=npts, sp=sp, length=length, start=start, post=st, post_npts=post_npts, post_info=post_info, dense=dn, dense_info=dn_info))


def edge_stages(mod, m, inp, nb=B_NB, post=True):
    """Every part-B stage of the first nb instances through `mod` (oracle.oracle_py in its current mode, or oracle.ref_py): dict of arrays padded like the device's
    outputs.  The reference has no entry for ragged / unsolved collision checks and none for the densifying branch: those keys come from the oracle only."""
    is_ref = mod.__name__.endswith("ref_py")
    p = None if is_ref else mod.default_params()
    a = (m,) if is_ref else (p, m)
    P, npts, sp = inp["P"], inp["npts"], inp["sp"]
    out = dict(bounds=np.zeros((nb, B_N, 4, 2)), n_valid=np.zeros(nb, dtype=np.int32), n_layers=np.zeros(nb, dtype=np.int32), l0=np.zeros(nb),
               layer_s=np.zeros((nb, B_CAP)), lb=np.zeros((nb, B_CAP)), ub=np.zeros((nb, B_CAP)))
    for b in range(nb):
        n = npts[b]
        bd, out["n_valid"][b] = mod.bounds_path(*a, *[P[k][b, :n] for k in REF_KEYS], *[P[k][b] for k in KNOT_KEYS])
        out["bounds"][b, :n] = bd
        nl, ls, lb, ub, out["l0"][b] = mod.dp_search(*a, *[sp[k][b] for k in KNOT_KEYS], inp["length"][b], inp["start"][b], **({} if is_ref else {"cap": B_CAP}))
        out["n_layers"][b] = nl
        if nl > 0:
            out["layer_s"][b, :nl], out["lb"][b, :nl], out["ub"][b, :nl] = ls, lb, ub
    if not post:
        return out
    st = inp["post"]
    out["free"] = np.array([[mod.collision_free(*a, *st[b, i, :3]) for i in range(st.shape[1])] for b in range(st.shape[0])], dtype=np.int8)
    if is_ref:
        r = [mod.postcheck(m, st[b]) for b in range(st.shape[0])]
        out["post_ok"] = np.array([x[0] for x in r], dtype=np.int32); out["post_nv"] = np.array([x[1] for x in r], dtype=np.int32)
        return out
    out["post_nv"], out["post_ok"] = mod.postcheck_batch(p, m, st, _solved(st.shape[0]))
    out["post2_nv"], out["post2_ok"] = mod.postcheck_batch(p, m, st, inp["post_info"], inp["post_npts"])
    for tag, cap in (("dense", B_DENSE_M), ("dense_small", B_DENSE_SMALL)):
        r = [_densify(mod, p, m, inp["dense"][k], inp["dense_info"]["status"][k], cap) for k in range(inp["dense"].shape[0])]
        out[tag + "_ok"] = np.array([x[0] for x in r], dtype=np.int32)
        out[tag + "_n"] = np.array([x[1] for x in r], dtype=np.int32)
        out[tag] = [x[2] for x in r]
    # ... and at every capacity that equals some path's own length: M samples kept and sample M colliding is a complete answer (n_out = M), one sample fewer room is -2
    n = out["dense_n"]
    out["dense_caps"] = sorted(set(int(v) for v in n[n > 0]))
    r = [[_densify(mod, p, m, inp["dense"][k], inp["dense_info"]["status"][k], cap)[:2] for k in range(inp["dense"].shape[0])] for cap in out["dense_caps"]]
    out["dense_cap_ok"] = np.array([[x[0] for x in row] for row in r], dtype=np.int32)
    out["dense_cap_n"] = np.array([[x[1] for x in row] for row in r], dtype=np.int32)
    return out


_B_ORACLE = {}


def _b_oracle(oracle, name, fill, portable):
    key = (name, fill, portable)
    if key not in _B_ORACLE:
        m = oracle.make_map(*edge_layer(name, fill))
        if portable:
            with oracle.portable_math():
                _B_ORACLE[key] = edge_stages(oracle, m, edge_inputs(name))
        else:
            _B_ORACLE[key] = edge_stages(oracle, m, edge_inputs(name))
    return _B_ORACLE[key]


INDEX_KEYS = ("n_valid", "n_layers", "free", "post_nv", "post_ok")
VALUE_KEYS = ("bounds", "l0", "layer_s", "lb", "ub")


@pytest.mark.parametrize("name,fill", B_SCENES)
def test_oracle_modes_agree_on_the_edge_scenes(oracle, name, fill):
    """glibc mode (the one pinned against the reference) against portable mode (the device's arithmetic) on every input of part B: every index output equal, values
    within 1e-9 (measured: 5.4e-15).  The GPU tests below compare the device with the portable mode; this ties them to the other."""
    a, c = _b_oracle(oracle, name, fill, False), _b_oracle(oracle, name, fill, True)
    for k in INDEX_KEYS + ("post2_nv", "post2_ok", "dense_ok", "dense_n", "dense_small_ok", "dense_small_n", "dense_cap_ok", "dense_cap_n"):
        assert np.array_equal(a[k], c[k]), k
    assert a["dense_caps"] == c["dense_caps"]
    worst = max(float(np.abs(a[k] - c[k]).max()) for k in VALUE_KEYS)
    worst = max([worst] + [float(np.abs(u - v).max()) for u, v in zip(a["dense"], c["dense"]) if len(u)])
    print(name, fill, "worst value difference between the oracle's modes", worst)
    assert worst < 1e-9


@pytest.mark.parametrize("name,fill", B_SCENES)
def test_edge_scenes_are_not_vacuous(oracle, name, fill):
    """The inputs do what part B is about: paths leave the layer, searches end early, collision checks are cut short after a free start."""
    o, inp = _b_oracle(oracle, name, fill, True), edge_inputs(name)
    nv, npts = o["n_valid"], inp["npts"]
    kw = B_LAYERS[name]
    d, res, px, py = edge_layer(name, fill)
    out = lambda x, y: (np.abs(x - px) > 0.5 * kw["size_x"] * res) | (np.abs(y - py) > 0.5 * kw["size_y"] * res)
    assert out(inp["P"]["ref_x"], inp["P"]["ref_y"])[npts == B_N].any(axis=1).all()  # every full-length path leaves the layer
    assert out(inp["sp"]["knot_x"], inp["sp"]["knot_y"]).any(axis=1).all()
    assert (nv < npts).any() and (nv[npts == B_N] < B_N).all()
    if fill == "free":
        assert (nv < npts).mean() >= 0.5 and (nv == npts).any()  # only the border truncates here
    else:
        assert (nv == npts).any()
    nl = o["n_layers"]
    last = o["layer_s"][np.arange(B_NB), np.maximum(nl, 1) - 1]
    assert (nl > 0).all() and (last < inp["length"]).any()  # at least one search ends before the reference's last layer
    assert ((o["post_nv"] > 0) & (o["post_nv"] < 64)).any()  # truncated at first > 0
    assert 0 < o["free"].mean() < 1 and 0 < o["free"][7].mean() < 1
    solved = inp["dense_info"]["status"] == 1
    n, ok, ns = o["dense_n"], o["dense_ok"], o["dense_small_n"]
    assert (n[solved] < 141).all()  # 42 m at 0.3 m would be 141 samples: every solved path is cut, at the border or at a disc
    assert ((n > 0) & (ok == 0)).any() and (ok[solved] == 1).any()  # ... some before 20 m, some after
    assert not n[~solved].any() and not ok[~solved].any()
    # the small capacity: met before any collision on some paths (-2), the shorter ones complete
    assert (ns[n > B_DENSE_SMALL] == -2).all() and (n > B_DENSE_SMALL).any()
    assert np.array_equal(ns[n <= B_DENSE_SMALL], n[n <= B_DENSE_SMALL]) and not o["dense_small_ok"][n > B_DENSE_SMALL].any()
    # a capacity equal to a path's own length is enough for that path (the walk tests sample M for collision before it needs room for it) and -2 for every longer one
    assert len(o["dense_caps"]) >= 3
    for cap, cn, cok in zip(o["dense_caps"], o["dense_cap_n"], o["dense_cap_ok"]):
        assert (n == cap).any() and np.array_equal(cn[n <= cap], n[n <= cap]) and np.array_equal(cok[n <= cap], ok[n <= cap]) and (cn[n > cap] == -2).all()


def _assert_against_reference(o, r, nb):
    """The bars of the live tests of test_bounds.py / test_plan_stages.py / test_post_step.py: indices equal, values below 1e-12."""
    for k in INDEX_KEYS:
        assert np.array_equal(o[k][:nb] if k in ("n_valid", "n_layers") else o[k], r[k]), k
    for k in VALUE_KEYS:
        assert np.abs(o[k][:nb] - r[k]).max() < 1e-12, k


@pytest.mark.skipif(not HAVE_REF, reason="reference tree not present: covered by tests/golden/edge_ref.npz instead")
@pytest.mark.parametrize("name,fill", B_SCENES)
def test_oracle_matches_reference_live_on_the_edge_scenes(oracle, name, fill):
    from oracle import ref_py

    m = oracle.make_map(*edge_layer(name, fill))
    _assert_against_reference(_b_oracle(oracle, name, fill, False), edge_stages(ref_py, m, edge_inputs(name)), B_NB)


@pytest.mark.parametrize("name,fill", B_SCENES)
def test_oracle_matches_reference_fixture_on_the_edge_scenes(oracle, name, fill):
    """The same comparison against what the reference's own classes returned for the first 16 instances (tests/golden/make_edge_golden.py)."""
    g = np.load(GOLD)
    nb = int(g["nb"])
    _assert_against_reference(_b_oracle(oracle, name, fill, False), {k: g[f"{name}_{fill}_{k}"] for k in INDEX_KEYS + VALUE_KEYS}, nb)


@pytest.fixture(scope="module")
def binding():
    from path_optimizer_amd import binding as b

    b.lib()
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("name,fill", B_SCENES)
def test_device_stages_on_the_edge_scenes_are_bit_identical_to_the_portable_oracle(binding, oracle, name, fill):
    o, inp = _b_oracle(oracle, name, fill, True), edge_inputs(name)
    eng = binding.Engine(0)
    eng.set_map(*edge_layer(name, fill))
    bd, nv = eng.bounds_batch(inp["P"], inp["npts"])
    assert np.array_equal(nv, o["n_valid"]) and np.array_equal(bd, o["bounds"])  # every bound of every covering circle of every path
    assert all(not bd[b, nv[b]:].any() for b in range(B_NB))
    ls, lb, ub, l0, nl = eng.dp_search_batch(inp["sp"], inp["length"], inp["start"], B_CAP)
    assert np.array_equal(nl, o["n_layers"]) and np.array_equal(l0, o["l0"])
    assert np.array_equal(ls, o["layer_s"]) and np.array_equal(lb, o["lb"]) and np.array_equal(ub, o["ub"])
    assert all(not (ls[b, nl[b]:].any() or lb[b, nl[b]:].any() or ub[b, nl[b]:].any()) for b in range(B_NB))
    pnv, pok = eng.postcheck_batch(inp["post"], _solved(8))
    assert np.array_equal(pnv, o["post_nv"]) and np.array_equal(pok, o["post_ok"])
    pnv, pok = eng.postcheck_batch(inp["post"], inp["post_info"], inp["post_npts"])
    assert np.array_equal(pnv, o["post2_nv"]) and np.array_equal(pok, o["post2_ok"])
    out, n, ok = eng.densify_batch(inp["dense"], inp["dense_info"], B_DENSE_M)
    assert np.array_equal(n, o["dense_n"]) and np.array_equal(ok, o["dense_ok"])
    for k in range(8):
        if n[k] > 0:
            assert np.abs(out[k, :n[k]] - o["dense"][k]).max() < 1e-9  # the bar of test_device_densifying_output_branch
        assert not out[k, n[k]:].any()
    out, n, ok = eng.densify_batch(inp["dense"], inp["dense_info"], B_DENSE_SMALL)
    assert np.array_equal(n, o["dense_small_n"]) and np.array_equal(ok, o["dense_small_ok"]) and (n == -2).any()  # M too small before any collision: -2
    for k in range(8):
        if n[k] > 0:
            assert np.abs(out[k, :n[k]] - o["dense_small"][k]).max() < 1e-9
    for cap, cn, cok in zip(o["dense_caps"], o["dense_cap_n"], o["dense_cap_ok"]):  # M equal to a path's own length: that path is complete, not -2
        out, n, ok = eng.densify_batch(inp["dense"], inp["dense_info"], cap)
        assert np.array_equal(n, cn) and np.array_equal(ok, cok), cap
        for k in range(8):
            if n[k] > 0:
                assert np.abs(out[k, :n[k]] - o["dense"][k][:n[k]]).max() < 1e-9 and not out[k, n[k]:].any()


# ------------------------------------------------------------------ C: both variants of the DP search
PLAN_MAP_KW = dict(size_x=600, size_y=600, resolution=0.2, pos=(1.0, -2.0), n_obstacles=40, r_range=(0.5, 2.0))  # the scene of tests/test_plan_stages.py
C_SCENES = ("plan", "wide")


@functools.lru_cache(maxsize=None)
def _c_map(scene):
    return _frozen(synth.make_distance_map(3, **PLAN_MAP_KW)[:4]) if scene == "plan" else edge_layer("wide", "discs")


def _search(eng, sp, length, start, cap):
    return dict(zip(("layer_s", "lb", "ub", "l0", "n_layers"), eng.dp_search_batch(sp, length, start, cap)))


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def _oracle_search(oracle, m, sp, length, start, cap, p=None):
    B = len(length)
    out = dict(layer_s=np.zeros((B, cap)), lb=np.zeros((B, cap)), ub=np.zeros((B, cap)), l0=np.zeros(B), n_layers=np.zeros(B, dtype=np.int32))
    p = p or oracle.default_params()
    with oracle.portable_math():
        for b in range(B):
            n, ls, lb, ub, out["l0"][b] = oracle.dp_search(p, m, *[sp[k][b] for k in KNOT_KEYS], length[b], start[b], cap=cap)
            out["n_layers"][b] = n
            if n > 0:
                out["layer_s"][b, :n], out["lb"][b, :n], out["ub"][b, :n] = ls, lb, ub
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("scene", C_SCENES)
def test_device_forced_one_wave_search_matches_oracle_and_eight_waves(binding, oracle, scene):
    """dp_search_kernel<1> behind the switch at B = 48: bit-identical to the portable oracle and to dp_search_kernel<8> on the same inputs (each edge cost is the
    same expression, both scans keep the first minimum in ascending order of the previous node), with a vehicle too far from the path and a layer capacity that is
    too small among the calls."""
    mp = _c_map(scene)
    sp, length, start = synth.make_search_inputs(23, 48)
    start[5] += np.array([40.0, 40.0, 0.0])  # graphSearchDp returns false
    eng = binding.Engine(0)
    eng.set_map(*mp)
    m = oracle.make_map(*mp)
    for cap in (64, 8):
        o = _oracle_search(oracle, m, sp, length, start, cap)
        eng.debug_set("dp_one_wave", 1)
        one = _search(eng, sp, length, start, cap)
        assert eng.debug_get("dp_waves_used") == 1
        eng.debug_set("dp_one_wave", 0)
        eight = _search(eng, sp, length, start, cap)
        assert eng.debug_get("dp_waves_used") == 8
        for k in o:
            assert np.array_equal(one[k], o[k]), (cap, k)
            assert np.array_equal(eight[k], one[k]), (cap, k)
        if cap == 64:
            assert o["n_layers"][5] == -1 and (np.delete(o["n_layers"], 5) > 0).all()
        else:
            assert (o["n_layers"] == -2).all() and not one["layer_s"].any()  # flagged, not truncated (the capacity is met before the vehicle's offset is looked at)


def _tie_scene():
    """A scene whose cheapest lattice paths come in mirrored pairs of EXACTLY equal cost, so that the scan's rule for ties (keep the first minimum, in ascending order of
    the previous node) decides the output.  Random scenes hold no exact tie, and a scan that kept the last minimum would pass every other test.
    The reference path is the x axis (knots x = s, y = 0: heading and curvature exactly 0), the vehicle stands on it, the lateral spacing is 0.5 (the running sum from
    -10 is exact and symmetric about the node at 0) and the layer, 400 x 120 cells centred on the axis, is free (10.0) except for two patches of zeros that are
    symmetric about the axis: a block ON the axis at the first layer after the start (x = 4.5: the straight continuation is infeasible, the nodes at -0.5 and +0.5 are
    equally good) and a gate at the third (x = 7.5: only the node on the axis is feasible, the mirrored paths must merge there or one layer earlier).  At the merge
    the two parents tie to the last bit; the first minimum is the node at -0.5, so layer 1's corridor lies below the axis.
    Returns (map tuple, spline dict, length [4], start [4, 3], lateral spacing)."""
    res, sx, sy, px, py = 0.2, 400, 120, 40.0, 0.0
    d = np.full((sx, sy), 10.0, dtype=np.float32)
    X, Y = np.meshgrid(px + 0.5 * sx * res - (np.arange(sx) + 0.5) * res, py + 0.5 * sy * res - (np.arange(sy) + 0.5) * res, indexing="ij")
    d[(np.abs(X - 4.5) < 0.25) & (np.abs(Y) < 0.2)] = 0.0
    d[(np.abs(X - 7.5) < 0.25) & (np.abs(Y) > 0.2)] = 0.0
    ks = np.tile(1.5 * np.arange(41), (4, 1))
    sp = dict(knot_s=ks, knot_x=ks.copy(), knot_y=np.zeros_like(ks))
    return (d, res, px, py), sp, 55.0 - 5.0 * np.arange(4), np.tile([3.0, 0.0, 0.0], (4, 1)), 0.5


def test_oracle_tie_scene_takes_the_first_minimum(oracle):
    """The tie scene does what it is for, in both of the oracle's modes: the layers fall on the block and the gate, and of the two mirrored corridors around the block
    the oracle reports the one below the axis (the lower node index)."""
    mp, sp, length, start, lat = _tie_scene()
    p = oracle.default_params(); p.search_lat_spacing = lat
    assert np.array_equal(mp[0], mp[0][:, ::-1])  # the layer is its own mirror image about the axis
    for portable in (False, True):
        oracle.set_portable_math(portable)
        try:
            r = [oracle.dp_search(p, oracle.make_map(*mp), *[sp[k][b] for k in KNOT_KEYS], length[b], start[b], cap=B_CAP) for b in range(4)]
        finally:
            oracle.set_portable_math(False)
        for n, ls, lb, ub, l0 in r:
            assert n > 20 and l0 == 0.0 and ls[1] == 4.5 and ls[3] == 7.5
            assert ub[1] < 0 and lb[3] < 0 < ub[3] and ub[3] - lb[3] < 1.0  # layer 1 passes below the block, layer 3 through the gate


@pytest.mark.gpu
def test_device_search_variants_break_cost_ties_like_the_oracle(binding, oracle):
    """Both kernels on the scene of exact ties: the one-wave scan keeps the first minimum, the eight waves' partial minima meet as (cost, then the smaller previous
    index) — the oracle's answer either way, bit for bit."""
    mp, sp, length, start, lat = _tie_scene()
    p = binding.default_params(); p.search_lat_spacing = lat
    op = oracle.default_params(); op.search_lat_spacing = lat
    eng = binding.Engine(0, p)
    eng.set_map(*mp)
    o = _oracle_search(oracle, oracle.make_map(*mp), sp, length, start, B_CAP, op)
    assert (o["ub"][:, 1] < 0).all()
    for one_wave, waves in ((1, 1), (0, 8)):
        eng.debug_set("dp_one_wave", one_wave)
        got = _search(eng, sp, length, start, B_CAP)
        assert eng.debug_get("dp_waves_used") == waves
        for k in o:
            assert np.array_equal(got[k], o[k]), (waves, k)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", C_SCENES)
def test_device_search_picks_one_wave_above_512_instances(binding, scene):
    """19 instances tiled 27 times: B = 513 runs one wave per instance and every row is the row of the B = 19 run (eight waves), bit for bit; B = 512 still runs
    eight waves.  Device rows against device rows: no oracle call on the tiled batch."""
    sp, length, start = synth.make_search_inputs(29, 19)
    start[3] += np.array([40.0, 40.0, 0.0])
    eng = binding.Engine(0)
    eng.set_map(*_c_map(scene))
    small = _search(eng, sp, length, start, B_CAP)
    assert eng.debug_get("dp_waves_used") == 8
    assert small["n_layers"][3] == -1 and (np.delete(small["n_layers"], 3) > 0).all()
    tile = lambda a, n: np.ascontiguousarray(np.concatenate([a] * 27, axis=0)[:n])
    for n, waves in ((513, 1), (512, 8)):
        big = _search(eng, {k: tile(sp[k], n) for k in KNOT_KEYS}, tile(length, n), tile(start, n), B_CAP)
        assert eng.debug_get("dp_waves_used") == waves
        for k in small:
            assert np.array_equal(big[k], tile(small[k], n)), (n, k)


def _dp_lds_bytes(binding, K, L):
    f = binding.lib().po_dp_lds_bytes
    f.restype, f.argtypes = C.c_size_t, [C.c_int, C.c_int]
    return int(f(K, L))


@pytest.mark.gpu
@pytest.mark.parametrize("scene", C_SCENES)
def test_device_search_falls_back_to_one_wave_when_the_scratch_does_not_fit(binding, oracle, scene):
    """A spline long enough that, at a capacity of 512 layers, the one-wave kernel's LDS fits in 160 KB but the eight-wave reduction scratch (8 x 3 x 64 doubles) on
    top of it does not (K from po_dp_lds_bytes: the middle of that window).  B = 2 with no switch set runs one wave, bit-identical to the portable oracle; one knot
    more than the largest K that fits is refused; just below the window eight waves run again."""
    cap, limit, scratch = 512, 160 * 1024, 8 * 3 * 64 * 8
    kmax = max(K for K in range(3, 2000) if _dp_lds_bytes(binding, K, cap) <= limit)
    kmin = min(K for K in range(3, 2000) if _dp_lds_bytes(binding, K, cap) + scratch > limit)
    assert 3 < kmin < kmax and _dp_lds_bytes(binding, kmax + 1, cap) > limit
    krun = (kmin + kmax) // 2
    P = synth.make_spline_paths(31, 2, 1700, 0.3, knot_ds=0.5)  # 509.7 m: 1024 knots every 0.5 m
    assert P["knot_s"].shape[1] > kmax
    mp = _c_map(scene)
    eng = binding.Engine(0)
    eng.set_map(*mp)

    def inputs(K):
        sp = {k: np.ascontiguousarray(P[k][:, :K]) for k in KNOT_KEYS}
        length = sp["knot_s"][:, -1] - np.array([2.0, 0.7])
        z = P["ref_z"][:, 2]
        start = np.stack([P["ref_x"][:, 2] - 0.4 * np.sin(z), P["ref_y"][:, 2] + 0.4 * np.cos(z), z + 0.05], axis=1)
        return sp, length, start

    sp, length, start = inputs(krun)
    got = _search(eng, sp, length, start, cap)
    assert eng.debug_get("dp_waves_used") == 1
    o = _oracle_search(oracle, oracle.make_map(*mp), sp, length, start, cap)
    for k in o:
        assert np.array_equal(got[k], o[k]), k
    assert (o["n_layers"] > 3).all()
    with pytest.raises(binding.PoError, match=r"rc=%d\b" % PO_ERR_UNSUPPORTED):
        _search(eng, *inputs(kmax + 1), cap)
    sp, length, start = inputs(kmin - 1)  # the scratch fits again
    wide = _search(eng, sp, length, start, cap)
    assert eng.debug_get("dp_waves_used") == 8
    o = _oracle_search(oracle, oracle.make_map(*mp), sp, length, start, cap)
    for k in o:
        assert np.array_equal(wide[k], o[k]), k


@pytest.mark.gpu
def test_device_plan_pipeline_does_not_depend_on_the_search_variant(binding):
    """po_plan_batch on the planning scenes of tests/test_pipeline.py plus a vehicle far from its path: states, counts, verdicts and stages identical with the
    search on one wave and on eight."""
    g = np.load(os.path.join(os.path.dirname(GOLD), "pipeline_ref.npz"))
    sc = synth.make_planning_scenes(int(g["seed"]), int(g["B"]))
    st = sc["start"][0].copy()
    st[0] += 30 * np.cos(st[2] + 1.5708); st[1] += 30 * np.sin(st[2] + 1.5708)
    wx, wy = np.concatenate([sc["way_x"], sc["way_x"][:1]]), np.concatenate([sc["way_y"], sc["way_y"][:1]])
    start, goal = np.concatenate([sc["start"], st[None]]), np.concatenate([sc["goal"], sc["goal"][:1]])
    eng = binding.Engine(0)
    eng.set_map(*sc["map"])
    runs = []
    for one_wave, waves in ((1, 1), (0, 8)):
        eng.debug_set("dp_one_wave", one_wave)
        runs.append(eng.plan_batch(wx, wy, start, goal, N=512))
        assert eng.debug_get("dp_waves_used") == waves
    (s1, n1, ok1, stage1, _), (s8, n8, ok8, stage8, _) = runs
    assert np.array_equal(s1, s8) and np.array_equal(n1, n8) and np.array_equal(ok1, ok8) and np.array_equal(stage1, stage8)
    assert ok1[:-1].all() and stage1[-1] == 3 and not ok1[-1]  # the plain scenes plan, the far start fails in the search
