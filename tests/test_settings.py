"""Every stage around the path QP away from the reference's default flags ("Settings away from the defaults").

The other test files run the bounds producer, the collision check, the densifying output, the DP lattice search, the smoothing QPs, the limits and the plan chain at
the values po_default_params gives the vehicle, the lattice, the smoothing weights, the output spacing, the friction limits and the smoothers' ADMM settings.  A
literal 2.0, 1.45, 0.6, 1.5 or 0.3 in a kernel or in the host code that fills its arguments would pass them all.  Here each of those settings moves:
  0. one table of settings, and for every non-default row a CPU assertion that it changes the oracle's output on the input it is tested with;
  A. CPU: the oracle against the reference's own classes with the same flags (live where the reference tree exists, tests/golden/settings_ref.npz everywhere);
  B. GPU: every stage against the oracle at the table's settings, the refusals and the capacity rules among them;
  C. CPU: the oracle's two arithmetic modes agree on every index output of these inputs, so that the allowances inside _compare / _close are not needed.
tests/golden/make_settings_golden.py imports this module and records what reference_record() returns."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_post_golden as GP  # noqa: E402
import speed_ref  # noqa: E402
import test_bounds as TB  # noqa: E402  (_close)
import test_map_edges as TE  # noqa: E402  (_arc_length, _densify, _solved, _frozen, _search, _oracle_search, _c_map)
import test_smooth as TS  # noqa: E402  (_compare, MAP_SEED, MAP_KW)
from path_optimizer_amd import synth  # noqa: E402
from path_optimizer_amd.abi import PO_ERR_INVALID, PO_ERR_UNSUPPORTED, PO_STATUS_MAX_ITER, PO_STATUS_SOLVED  # noqa: E402

HAVE_REF = os.path.isdir("/root/reference")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "settings_ref.npz")
KNOT_KEYS = TE.KNOT_KEYS
REF_KEYS = TE.REF_KEYS


# ------------------------------------------------------------------ 0: the settings table
def _vehicle(width, length, rtc, margin):
    """A row of po_params fields; d[0 .. 3] by the reference's formula (planning_flags.cpp:10-13), which the library does not apply itself (po_hip.h at po_params.d)."""
    return dict(car_width=width, car_length=length, rear_axle_to_center=rtc, safety_margin=margin,
                d=tuple(c * length + rtc for c in (-3.0 / 8.0, -1.0 / 8.0, 1.0 / 8.0, 3.0 / 8.0)))


def _search_row(lat_range, long_spacing, lat_spacing):
    return dict(search_lateral_range=lat_range, search_long_spacing=long_spacing, search_lat_spacing=lat_spacing)


VEHICLES = {"default": _vehicle(2.0, 4.9, 1.45, 0.0), "compact": _vehicle(1.6, 4.13, 1.9, 0.0), "van": _vehicle(2.4, 5.6, 1.2, 0.15)}  # compact: the reference demo's second car
SEARCHES = {"default": _search_row(10.0, 1.5, 0.6), "fine": _search_row(6.0, 1.0, 0.4), "edge64": _search_row(6.3, 2.5, 0.2), "coarse": _search_row(12.0, 3.0, 0.5)}
SEARCH_REFUSED = _search_row(10.0, 1.5, 0.3)  # 2 * 10 / 0.3 + 1 = 67.7 lateral samples: more than the 64 lanes of a wave
WEIGHTS = {"default": dict(t2_w_dev=0.005, t2_w_curv=1.0, t2_w_curv_rate=10.0, cart_w_curv=1.0, cart_w_curv_rate=50.0, cart_w_dev=0.0),
           "other": dict(t2_w_dev=0.05, t2_w_curv=3.0, t2_w_curv_rate=25.0, cart_w_curv=2.5, cart_w_curv_rate=20.0, cart_w_dev=0.01)}
SPACINGS = (0.3, 0.1, 0.45)
FRICTION = {"default": dict(mu=0.4, max_curvature_rate=0.1), "other": dict(mu=0.7, max_curvature_rate=0.25)}
ADMM = {"max_iter": dict(max_iter=50), "no_adapt": dict(adapt_every=0), "unscaled": dict(scaling=0), "scaling4": dict(scaling=4),
        "check10": dict(check_every=10, alpha=1.2, rho0=0.5, sigma=1e-5), "adapt_tol": dict(adapt_tol=1.5)}
COMBINED = dict(VEHICLES["compact"], **SEARCHES["fine"], output_spacing=0.45)  # part A / B: the whole chain at a second car, a second lattice and a coarser output
SEARCH_CAP = 64  # layer capacity of the search calls; SEARCH_CAP_SHORT is too small for the "fine" lattice only
SEARCH_CAP_SHORT = 48


def settings(mod, *rows, **fields):
    """mod.default_params() (the binding's or the oracle's: one struct) with the rows of the table and single fields applied."""
    p = mod.default_params()
    for row in rows + (fields,):
        for k, v in row.items():
            if k == "d":
                for j in range(4):
                    p.d[j] = v[j]
            else:
                setattr(p, k, v)
    return p


def lattice_nodes(row):
    """Lateral samples of a layer by the reference's running sum (reference_path_smoother.cpp:186-210)."""
    n, cur = 0, -row["search_lateral_range"]
    while cur <= row["search_lateral_range"]:
        n += 1
        cur += row["search_lat_spacing"]
    return n


# ------------------------------------------------------------------ the inputs, built once and frozen
@functools.lru_cache(maxsize=None)
def big_map():
    """The 600 x 600 layer of tests/test_bounds.py and tests/test_post_step.py."""
    return TE._frozen(synth.make_distance_map(**GP.MAP_ARGS)[:4])


@functools.lru_cache(maxsize=None)
def smooth_map():
    return TE._frozen(synth.make_distance_map(TS.MAP_SEED, **TS.MAP_KW)[:4])


@functools.lru_cache(maxsize=None)
def bounds_paths():
    return TE._frozen(synth.make_spline_paths(11, 12, 150))


@functools.lru_cache(maxsize=None)
def post_inputs():
    """16 paths of 150 states every 0.25 m for the walk of the collision check (paths 12 .. 27 of make_post_golden.post_cases: six of them run into a disc, three of
    those at another state for another car), 600 single poses over the whole layer and beyond its border."""
    rng = np.random.default_rng(5)
    poses = np.stack([rng.uniform(-65, 65, 600), rng.uniform(-65, 65, 600), rng.uniform(-4, 4, 600)], axis=1)
    return TE._frozen(dict(states=TE._arc_length(GP.post_cases(npath=28, N=150)[12:]), poses=poses))


@functools.lru_cache(maxsize=None)
def dense_inputs():
    """8 paths of 50 states every 0.75 m (every third state of paths 16 .. 23 of post_cases), one of them unsolved: what the densifying branch splines through."""
    st = TE._arc_length(np.ascontiguousarray(GP.post_cases(npath=24, N=150)[16:, ::3]))
    info = TE._solved(8); info["status"][5] = -2
    return TE._frozen(dict(states=st, info=info))


@functools.lru_cache(maxsize=None)
def search_inputs():
    """The eight instances of make_search_inputs(29, 8); the last vehicle stands 6.1 m to the left of its path: inside a lateral range of 6.3, 10 and 12, outside one of 6."""
    sp, length, start = synth.make_search_inputs(29, 8)
    z = sp["ref_z"][7, 3]
    start[7] = [sp["ref_x"][7, 3] - 6.1 * np.sin(z), sp["ref_y"][7, 3] + 6.1 * np.cos(z), z]
    return TE._frozen((sp, length, start))


@functools.lru_cache(maxsize=None)
def smooth_inputs(kind):
    return TE._frozen(synth.make_smooth_inputs(21, 6, P=40, kind=kind))


@functools.lru_cache(maxsize=None)
def limits_inputs():
    rng = np.random.default_rng(2)
    v = rng.uniform(0, 15, (4, 50)); v[0, :3] = [0, 0.0001, 0.00011]
    return TE._frozen((v, rng.uniform(-4.5, 4.5, (4, 50))))  # |a| above mu g = 3.92 gives NaN at the default and a number at mu = 0.7


PLAN_SEED, PLAN_B, PLAN_N = 31, 4, 256


@functools.lru_cache(maxsize=None)
def plan_scenes():
    """Four planning instances of 12 waypoints (33 m) over a 600 x 600 layer."""
    return TE._frozen(synth.make_planning_scenes(PLAN_SEED, PLAN_B, n_way=12, map_kw=dict(size_x=600, size_y=600)))


# ------------------------------------------------------------------ the stages through the oracle or through the reference's own classes
def _is_ref(mod):
    return mod.__name__.endswith("ref_py")


class _flags:
    """The reference reads its flags, the oracle its po_params: `with _flags(mod, p)` sets the former and is a no-op for the latter."""

    def __init__(self, mod, p):
        self.cm = mod.flags_from(p) if _is_ref(mod) else None

    def __enter__(self):
        if self.cm:
            self.cm.__enter__()

    def __exit__(self, *a):
        if self.cm:
            self.cm.__exit__(*a)


def st_bounds(mod, p, nb=12):
    P, m = bounds_paths(), mod_map(big_map())
    a = (m,) if _is_ref(mod) else (p, m)
    out = dict(bounds=np.zeros((nb, 150, 4, 2)), n_valid=np.zeros(nb, dtype=np.int32))
    with _flags(mod, p):
        for b in range(nb):
            out["bounds"][b], out["n_valid"][b] = mod.bounds_path(*a, *[P[k][b] for k in REF_KEYS], *[P[k][b] for k in KNOT_KEYS])
    return out


def st_post(mod, p):
    inp, m = post_inputs(), mod_map(big_map())
    a = (m,) if _is_ref(mod) else (p, m)
    with _flags(mod, p):
        free = np.array([mod.collision_free(*a, *q) for q in inp["poses"]], dtype=np.int8)
        if _is_ref(mod):
            r = [mod.postcheck(m, st)[:2] for st in inp["states"]]
            ok, nv = np.array([x[0] for x in r], dtype=np.int32), np.array([x[1] for x in r], dtype=np.int32)
        else:
            nv, ok = mod.postcheck_batch(p, m, inp["states"], TE._solved(16))
    return dict(free=free, post_nv=nv, post_ok=ok)


def st_dense(oracle, p, cap):
    """The densifying branch of the oracle (the reference reaches it only through PathOptimizer::solve: st_plan): ok [8], n [8] (-2: capacity), rows."""
    inp, m = dense_inputs(), mod_map(big_map())
    r = [TE._densify(oracle, p, m, inp["states"][k], inp["info"]["status"][k], cap) for k in range(8)]
    return dict(ok=np.array([x[0] for x in r], dtype=np.int32), n=np.array([x[1] for x in r], dtype=np.int32), rows=[x[2] for x in r])


def st_search(mod, p, cap=SEARCH_CAP):
    sp, length, start = search_inputs()
    m = mod_map(TE._c_map("plan"))
    B = len(length)
    out = dict(layer_s=np.zeros((B, cap)), lb=np.zeros((B, cap)), ub=np.zeros((B, cap)), l0=np.zeros(B), n_layers=np.zeros(B, dtype=np.int32))
    with _flags(mod, p):
        for b in range(B):
            a = (m,) if _is_ref(mod) else (p, m)
            n, ls, lb, ub, out["l0"][b] = mod.dp_search(*a, *[sp[k][b] for k in KNOT_KEYS], length[b], start[b], **({} if _is_ref(mod) else {"cap": cap}))
            out["n_layers"][b] = n
            if n > 0:
                out["layer_s"][b, :n], out["lb"][b, :n], out["ub"][b, :n] = ls, lb, ub
    return out


def st_assembly(mod, oracle, p, kind, b):
    """P (upper triangle, CSC), A (CSC), q, l, u of smoothing QP `kind` on instance b, and the QP's solution: dict of flat arrays."""
    inp = smooth_inputs(kind)
    m = mod_map(smooth_map())
    if _is_ref(mod):
        with _flags(mod, p):
            if kind < 2:
                r = mod.osqp_smooth(kind, p, inp["x"][b], inp["y"][b], inp["angle"][b], inp["k"][b], inp["s"][b], m_map=m)
            else:
                sp = synth.make_spline_paths(5, 1, N=200)
                r = mod.post_smooth(p, inp["s"][b], inp["lb"][b], inp["ub"][b], inp["l0"][b], sp["knot_s"][0], sp["knot_x"][0], sp["knot_y"][0])
        Pm, Am, q, l, u, x, rc = r["P"], r["A"], r["q"], r["l"], r["u"], r["x"], r["rc"]
    else:
        Pm, q, Am, l, u = oracle.smooth_assemble(kind, p, inp, b, m_map=m)
        one = {k: (None if v is None else v[b:b + 1]) for k, v in inp.items()}
        _, _, _, info, raw = oracle.smooth_batch(kind, p, one, m_map=m, want_raw=True)
        x, rc = raw[0], int(info["status"][0] == PO_STATUS_SOLVED)
    return dict(Pp=Pm.indptr, Pi=Pm.indices, Px=Pm.data, Ap=Am.indptr, Ai=Am.indices, Ax=Am.data, q=q, l=l, u=u, x=x, rc=np.int32(rc))


def st_limits(mod, p):
    v, a = limits_inputs()
    with _flags(mod, p):
        r = [mod.limits(v[b], a[b]) if _is_ref(mod) else mod.limits(p, v[b], a[b]) for b in range(len(v))]
    return dict(max_k=np.array([x[0] for x in r]), max_kp=np.array([x[1] for x in r]))


def st_plan(mod, p, nb=PLAN_B):
    """PathOptimizer::solve on the planning instances: [(ok, path [n, 5], iterations of the path QP or -1)]"""
    sc = plan_scenes()
    m = mod_map(sc["map"])
    out = []
    with _flags(mod, p):
        for b in range(nb):
            a = (sc["way_x"][b], sc["way_y"][b], sc["start"][b], sc["goal"][b])
            if _is_ref(mod):
                ok, path = mod.path_optimizer_solve(m, p, *a)
                out.append((bool(ok), path, -1))
            else:
                ok, path, tr = mod.path_optimizer_solve(p, m, *a)
                out.append((bool(ok), path, int(tr["qp"]["iters"]) if "qp" in tr else -1))
    return out


def mod_map(mp):
    from oracle import oracle_py

    return oracle_py.make_map(*mp)


# ---- everything part A compares, as one flat dict: from the oracle, or from the reference (then it is what tests/golden/settings_ref.npz holds)
RECORD_BOUNDS_NB = 6   # paths of the bounds scene in the record (the fixture's size; the device tests use all 12)
RECORD_SMOOTH_B = (0, 3)


def reference_record(mod, oracle):
    out = {}
    for name in ("compact", "van"):
        p = settings(oracle, VEHICLES[name])
        for k, v in st_bounds(mod, p, RECORD_BOUNDS_NB).items():
            out[f"bounds_{name}_{k}"] = v
        for k, v in st_post(mod, p).items():
            out[f"post_{name}_{k}"] = v
    for name in ("fine", "edge64", "coarse"):
        for k, v in st_search(mod, settings(oracle, SEARCHES[name])).items():
            out[f"search_{name}_{k}"] = v
    p = settings(oracle, WEIGHTS["other"])
    for kind in (0, 1):
        for b in RECORD_SMOOTH_B:
            for k, v in st_assembly(mod, oracle, p, kind, b).items():
                out[f"smooth_k{kind}_{b}_{k}"] = v
    for k, v in st_limits(mod, settings(oracle, FRICTION["other"])).items():
        out[f"limits_{k}"] = v
    for raw in (1, 0):
        for b, (ok, path, _) in enumerate(st_plan(mod, settings(oracle, COMBINED, enable_raw_output=raw))):
            out[f"plan_raw{raw}_{b}_ok"] = np.int32(ok)
            out[f"plan_raw{raw}_{b}_path"] = path
    return out


def assert_record(o, r):
    """The bars of the default-flag tests of each stage: 1e-12 and equal n_valid for the bounds (tests/test_bounds.py), equal decisions for the collision check
    (tests/test_post_step.py), bit equality for the search (every output of every instance: stricter than the 23 of 24 of tests/test_plan_stages.py), the smoothers' assembly and solution
    (tests/test_smooth.py) and the limits (tests/test_plan_stages.py), 1e-9 for PathOptimizer::solve (tests/test_pipeline.py)."""
    assert set(o) == set(r), set(o) ^ set(r)
    for k in sorted(o):
        a, b = np.asarray(o[k]), np.asarray(r[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if k.startswith("bounds_") and k.endswith("_bounds"):
            assert np.abs(a - b).max() < 1e-12, k
        elif k.startswith("plan_") and k.endswith("_path"):
            assert len(a) == 0 or np.abs(a - b).max() < 1e-9, k
        else:
            assert np.array_equal(a, b, equal_nan=k.startswith("limits_")), k


_ORACLE_RECORD = {}


def oracle_record(oracle):
    if not _ORACLE_RECORD:
        _ORACLE_RECORD.update(reference_record(oracle, oracle))
    return _ORACLE_RECORD


# ------------------------------------------------------------------ 0 (CPU): the table is what it says, and every row is live on its input
def test_table_rows(oracle):
    p = oracle.default_params()
    for name, row in (("vehicle", VEHICLES["default"]), ("search", SEARCHES["default"]), ("weights", WEIGHTS["default"]), ("friction", FRICTION["default"])):
        for k, v in row.items():
            assert (tuple(p.d) if k == "d" else getattr(p, k)) == v, (name, k)  # the "default" rows are po_default_params, d[] by the formula included
    assert p.output_spacing == SPACINGS[0]
    # (the running sum decides, not range / spacing: -6 + 30 x 0.4 lands above 6, so "fine" has 30 samples and not 31)
    assert [lattice_nodes(SEARCHES[k]) for k in ("default", "fine", "edge64", "coarse")] == [34, 30, 63, 49]
    # 6.3 / 0.2: 2 * range / spacing + 1 = 63.99999999999999, which the library accepts (not > 64); the running sum of the offsets reaches 6.100000000000007 at node 62
    # and 6.300000000000007, one rounding error above the range, at the next: 63 nodes, lanes 0 .. 62.  Lane 63 and parent index 63 are NOT in use at this setting.
    row = SEARCHES["edge64"]
    assert 2 * row["search_lateral_range"] / row["search_lat_spacing"] + 1 == 63.99999999999999
    assert 2 * SEARCH_REFUSED["search_lateral_range"] / SEARCH_REFUSED["search_lat_spacing"] + 1 > 64


@pytest.mark.parametrize("name", ("compact", "van"))
def test_vehicle_is_live(oracle, name):
    """Bounds, single poses, the walk of the collision check and the densifying walk all change with the car."""
    p0, p = settings(oracle), settings(oracle, VEHICLES[name])
    b0, b = st_bounds(oracle, p0), st_bounds(oracle, p)
    assert not np.array_equal(b0["bounds"], b["bounds"])
    q0, q = st_post(oracle, p0), st_post(oracle, p)
    assert not np.array_equal(q0["free"], q["free"]) and not np.array_equal(q0["post_nv"], q["post_nv"])
    assert 0 < q["free"].mean() < 1 and (q["post_nv"] < 150).any() and (q["post_nv"] > 0).any()
    assert not np.array_equal(st_dense(oracle, p0, 400)["n"], st_dense(oracle, p, 400)["n"])
    # each primary alone matters too (a stale field would otherwise hide behind the others)
    for field in ("car_width", "car_length", "rear_axle_to_center"):  # (safety_margin is no input of the collision check: CarGeometry does not read it)
        if VEHICLES[name][field] != VEHICLES["default"][field]:
            one = settings(oracle, **{field: VEHICLES[name][field]})
            assert not np.array_equal(st_post(oracle, one)["free"], q0["free"]), field
    for field in ("car_width", "car_length", "safety_margin"):  # the bounds radius; d[] is the fourth input of the bounds
        if VEHICLES[name][field] != VEHICLES["default"][field]:
            assert not np.array_equal(st_bounds(oracle, settings(oracle, **{field: VEHICLES[name][field]}), 4)["bounds"], b0["bounds"][:4]), field
    assert not np.array_equal(st_bounds(oracle, settings(oracle, d=VEHICLES[name]["d"]), 4)["bounds"], b0["bounds"][:4])


@pytest.mark.parametrize("spacing", SPACINGS[1:])
def test_output_spacing_is_live(oracle, spacing):
    a, b = st_dense(oracle, settings(oracle), 400), st_dense(oracle, settings(oracle, output_spacing=spacing), 400)
    assert not np.array_equal(a["n"], b["n"]) and (b["n"] > 0).any() and (b["n"] != -2).all()


@pytest.mark.parametrize("name", ("fine", "edge64", "coarse"))
def test_search_settings_are_live(oracle, name):
    o0, o = st_search(oracle, settings(oracle)), st_search(oracle, settings(oracle, SEARCHES[name]))
    assert not np.array_equal(o0["n_layers"], o["n_layers"]) and not np.array_equal(o0["lb"], o["lb"])
    assert (o["n_layers"][:7] > 3).all()
    assert o["n_layers"][7] == -1 if name == "fine" else o["n_layers"][7] > 3  # 6.1 m beside the path: outside a range of 6 only
    for field, v in SEARCHES[name].items():  # each of the three fields alone
        one = st_search(oracle, settings(oracle, **{field: v}))
        assert any(not np.array_equal(one[k], o0[k]) for k in one), field
    if name == "fine":  # the capacity the device test is short of
        assert o["n_layers"][:7].max() > SEARCH_CAP_SHORT and st_search(oracle, settings(oracle), SEARCH_CAP_SHORT)["n_layers"].min() > 0


@pytest.mark.parametrize("kind", (0, 1))
def test_smoothing_weights_are_live(oracle, kind):
    """TENSION2 reads t2_w_*, TENSION cart_w_*; the QP of postSmooth reads neither (its weights 1, 100, 1000 are literals of the reference)."""
    a, b = (oracle.smooth_batch(kind, settings(oracle, WEIGHTS[w]), smooth_inputs(kind), m_map=mod_map(smooth_map()), want_raw=True) for w in ("default", "other"))
    assert (a[3]["status"] == PO_STATUS_SOLVED).all() and (b[3]["status"] == PO_STATUS_SOLVED).all()
    assert np.abs(a[4] - b[4]).max() > 1e-3
    fields = ("t2_w_dev", "t2_w_curv", "t2_w_curv_rate") if kind == 0 else ("cart_w_curv", "cart_w_curv_rate", "cart_w_dev")
    for f in fields:
        Pm = oracle.smooth_assemble(kind, settings(oracle, **{f: WEIGHTS["other"][f]}), smooth_inputs(kind), 0, m_map=mod_map(smooth_map()))[0]
        assert not np.array_equal(Pm.data, oracle.smooth_assemble(kind, settings(oracle), smooth_inputs(kind), 0, m_map=mod_map(smooth_map()))[0].data), f
    post = [oracle.smooth_batch(2, settings(oracle, WEIGHTS[w]), smooth_inputs(2), want_raw=True)[4] for w in ("default", "other")]
    assert np.array_equal(post[0], post[1])


def test_friction_is_live(oracle):
    a, b = st_limits(oracle, settings(oracle)), st_limits(oracle, settings(oracle, FRICTION["other"]))
    assert not np.array_equal(a["max_k"], b["max_k"], equal_nan=True) and not np.array_equal(a["max_kp"], b["max_kp"])
    assert np.isnan(a["max_k"]).any() and not np.isnan(b["max_k"]).any()  # |a| beyond mu g = 3.92: sqrt of a negative number; none beyond 0.7 g = 6.86
    for f in ("mu", "max_curvature_rate"):
        one = st_limits(oracle, settings(oracle, **{f: FRICTION["other"][f]}))
        assert not (np.array_equal(one["max_k"], a["max_k"], equal_nan=True) and np.array_equal(one["max_kp"], a["max_kp"])), f


_SMOOTH = {}


def oracle_smooth(oracle, kind, name, portable=False):
    """oracle.smooth_batch of smooth_inputs(kind) at ADMM row `name` ("default": none), computed once."""
    key = (kind, name, portable)
    if key not in _SMOOTH:
        p = settings(oracle, ADMM.get(name, {}))
        oracle.set_portable_math(portable)
        try:
            _SMOOTH[key] = oracle.smooth_batch(kind, p, smooth_inputs(kind), m_map=mod_map(smooth_map()), want_raw=True)
        finally:
            oracle.set_portable_math(False)
    return _SMOOTH[key]


# Where an ADMM row changes nothing, as found on the oracle.  TENSION2 (kind 0) has equality rows only: with OSQP's rho of 1e3 on equality rows the iteration is at
# its fixed point when the second termination check comes (50 iterations at every setting), so only the check interval shows there.  adapt_tol 1.5 moves a rho update of
# postSmooth's QP (kind 2) and none of TENSION's (kind 1).  Every row is live on at least one kind; the device test runs the dead pairs too, and proves nothing by them.
ADMM_NOT_LIVE = {("adapt_tol", 0), ("adapt_tol", 1), ("max_iter", 0), ("no_adapt", 0), ("scaling4", 0), ("unscaled", 0)}


@pytest.mark.parametrize("kind", TS.KINDS)
@pytest.mark.parametrize("name", sorted(ADMM))
def test_admm_setting_is_live(oracle, kind, name):
    """Every ADMM row changes a status, an iteration count or a refactorisation count of the smoothing QPs it is tested on — or moves the solution by more than the
    tolerance _compare holds the device to (1e-7; 2e-7 for kind 1) — except on the pairs listed in ADMM_NOT_LIVE, which are asserted to be exactly that."""
    a, b = oracle_smooth(oracle, kind, "default"), oracle_smooth(oracle, kind, name)
    assert (a[3]["status"] == PO_STATUS_SOLVED).all()
    counts = any(not np.array_equal(a[3][k], b[3][k]) for k in ("status", "iters", "n_refactor"))
    moved = float(np.abs(a[4] - b[4]).max())
    print(kind, name, "iters", a[3]["iters"].tolist(), "->", b[3]["iters"].tolist(), "status", b[3]["status"].tolist(), "solution moved by", moved)
    assert (counts or moved > (2e-7 if kind == 1 else 1e-7)) == ((name, kind) not in ADMM_NOT_LIVE)
    assert {n for n, k in ADMM_NOT_LIVE} <= {n for n in ADMM for k in TS.KINDS if (n, k) not in ADMM_NOT_LIVE}  # every row is live somewhere
    if name == "max_iter" and kind > 0:
        hit = b[3]["status"] == PO_STATUS_MAX_ITER
        assert hit.any() and (b[3]["iters"][hit] == 50).all() and (b[3]["status"][~hit] == PO_STATUS_SOLVED).all()
    # no run ends with an infeasibility certificate (were there one, it would be a case to add); without rho updates one postSmooth QP runs into max_iter = 4000
    assert np.isin(b[3]["status"], (PO_STATUS_SOLVED, PO_STATUS_MAX_ITER)).all()
    assert (b[3]["status"] == PO_STATUS_SOLVED).all() or name == "max_iter" or (name, kind) == ("no_adapt", 2)
    if name == "no_adapt":
        assert not b[3]["n_refactor"].any() and (kind == 0 or a[3]["n_refactor"].any())
    if name == "check10":
        assert (b[3]["iters"] % 10 == 0).all() and (b[3]["iters"] % 25 != 0).any()


def test_combined_setting_is_live(oracle):
    rec = oracle_record(oracle)
    for raw in (1, 0):
        base = st_plan(oracle, settings(oracle, enable_raw_output=raw))
        for b, (ok, path, _) in enumerate(base):
            assert ok and rec[f"plan_raw{raw}_{b}_ok"] and len(rec[f"plan_raw{raw}_{b}_path"]) != len(path), (raw, b)
    for b in range(PLAN_B):  # the dense branch samples every 0.45 m
        assert np.allclose(np.diff(rec[f"plan_raw0_{b}_path"][:, 4]), 0.45)


# ------------------------------------------------------------------ A (CPU): the oracle against the reference's own classes at these flags
@pytest.mark.skipif(not HAVE_REF, reason="reference tree not present: covered by tests/golden/settings_ref.npz instead")
def test_oracle_matches_reference_live_at_the_settings(oracle):
    from oracle import ref_py

    before = {f: C.c_double.in_dll(ref_py.lib_smooth(), "FLAGS_" + f).value for f in ("car_width", "search_lateral_spacing", "d1", "circle_radius", "mu")}
    assert_record(oracle_record(oracle), reference_record(ref_py, oracle))
    # the helper put every flag back, in every library
    for L in (ref_py.lib(), ref_py.lib_bounds(), ref_py.lib_smooth()):
        assert {f: C.c_double.in_dll(L, "FLAGS_" + f).value for f in before} == before
    assert before["car_width"] == 2.0 and before["search_lateral_spacing"] == 0.6 and before["mu"] == 0.4


@pytest.mark.skipif(not HAVE_REF, reason="reference tree not present")
def test_reference_flags_helper_reaches_all_three_libraries(oracle):
    """Each reference library is linked with its own copy of planning_flags.cpp: a flag set in one is not seen by the others, so flags_from writes all three."""
    from oracle import ref_py

    p = settings(oracle, VEHICLES["van"], SEARCHES["coarse"])
    with ref_py.flags_from(p):
        for L in (ref_py.lib(), ref_py.lib_bounds(), ref_py.lib_smooth()):
            g = lambda f: C.c_double.in_dll(L, "FLAGS_" + f).value
            assert (g("car_width"), g("car_length"), g("rear_axle_to_center"), g("safety_margin")) == (2.4, 5.6, 1.2, 0.15)
            assert (g("search_lateral_range"), g("search_longitudial_spacing"), g("search_lateral_spacing")) == (12.0, 3.0, 0.5)
            assert [g("d1"), g("d2"), g("d3"), g("d4")] == list(VEHICLES["van"]["d"])
            assert g("circle_radius") == np.sqrt((5.6 / 8) ** 2 + (2.4 / 2) ** 2) + 0.15
    assert C.c_double.in_dll(ref_py.lib_bounds(), "FLAGS_car_width").value == 2.0


def test_oracle_matches_reference_fixture_at_the_settings(oracle):
    """The same comparison against what the reference's classes returned when tests/golden/make_settings_golden.py ran."""
    g = np.load(GOLD)
    assert_record(oracle_record(oracle), {k: g[k] for k in g.files})


# ------------------------------------------------------------------ C (CPU): the oracle's two modes agree, so the device comparisons need no allowance
def _in_both_modes(oracle, fn):
    a = fn()
    with oracle.portable_math():
        c = fn()
    return a, c


@pytest.mark.parametrize("name", sorted(VEHICLES))
def test_oracle_modes_agree_on_the_vehicle_stages(oracle, name):
    """glibc mode (pinned against the reference) and portable mode (the device's arithmetic): every n_valid, every collision decision and every densified count equal —
    the one n_valid flip that _close of tests/test_bounds.py would allow is not used on these inputs."""
    p = settings(oracle, VEHICLES[name])
    a, c = _in_both_modes(oracle, lambda: (st_bounds(oracle, p), st_post(oracle, p), [st_dense(oracle, settings(oracle, VEHICLES[name], output_spacing=s), 400) for s in SPACINGS]))
    assert np.array_equal(a[0]["n_valid"], c[0]["n_valid"]) and np.abs(a[0]["bounds"] - c[0]["bounds"]).max() < 1e-9
    for k in a[1]:
        assert np.array_equal(a[1][k], c[1][k]), k
    for u, v in zip(a[2], c[2]):
        assert np.array_equal(u["n"], v["n"]) and np.array_equal(u["ok"], v["ok"])
        assert max(float(np.abs(x - y).max()) for x, y in zip(u["rows"], v["rows"]) if len(x)) < 1e-9


@pytest.mark.parametrize("name", sorted(SEARCHES))
def test_oracle_modes_agree_on_the_searches(oracle, name):
    p = settings(oracle, SEARCHES[name])
    a, c = _in_both_modes(oracle, lambda: st_search(oracle, p))
    assert np.array_equal(a["n_layers"], c["n_layers"])
    assert max(float(np.abs(a[k] - c[k]).max()) for k in ("layer_s", "lb", "ub", "l0")) < 1e-9


@pytest.mark.parametrize("kind", TS.KINDS)
def test_oracle_modes_agree_on_the_smoothing_runs(oracle, kind):
    """Statuses, iteration counts and refactorisations of every smoothing run of part B in both modes (the smoothers read the map through map_distance only and take
    sin / cos from glibc in either mode: the runs are the same bit for bit, which is what lets _compare's 10 % allowance go unused)."""
    for name in ["default"] + sorted(ADMM):
        a, c = oracle_smooth(oracle, kind, name, False), oracle_smooth(oracle, kind, name, True)
        for k in ("status", "iters", "n_refactor"):
            assert np.array_equal(a[3][k], c[3][k]), (name, k)
        assert np.array_equal(a[4], c[4]), name


def test_oracle_modes_agree_on_the_plan_inputs(oracle):
    for raw in (1, 0):
        p = settings(oracle, COMBINED, enable_raw_output=raw)
        a, c = _in_both_modes(oracle, lambda: st_plan(oracle, p))
        for (ok1, p1, it1), (ok2, p2, it2) in zip(a, c):
            assert (ok1, p1.shape, it1) == (ok2, p2.shape, it2) and np.abs(p1 - p2).max() < 1e-9


# ------------------------------------------------------------------ B (GPU)
@pytest.fixture(scope="module")
def binding():
    from path_optimizer_amd import binding as b

    b.lib()
    return b


def _engine(binding, mp, *rows, **fields):
    eng = binding.Engine(0, settings(binding, *rows, **fields))
    if mp is not None:
        eng.set_map(*mp)
    return eng


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached inputs are read-only)


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(VEHICLES))
def test_device_bounds_at_the_vehicles(binding, oracle, name):
    """DevBounds::radius and d[4] from a fresh handle's car: both entries against the portable oracle, every n_valid equal and every bound within 1e-9 (_close of
    tests/test_bounds.py with nothing left over), and bit for bit as tests/test_map_edges.py holds the default car."""
    import torch

    eng = _engine(binding, big_map(), VEHICLES[name])
    P = bounds_paths()
    with oracle.portable_math():
        o = st_bounds(oracle, settings(oracle, VEHICLES[name]))
    bd, nv = eng.bounds_batch(P)
    assert TB._close(bd, o["bounds"], nv, o["n_valid"]) == (1.0, 1.0)
    assert np.array_equal(nv, o["n_valid"]) and np.array_equal(bd, o["bounds"])
    assert all(not bd[b, nv[b]:].any() for b in range(12))
    t = {k: _dev(P[k]) for k in REF_KEYS + KNOT_KEYS}
    bounds = torch.full((12, 150, 4, 2), 7.0, dtype=torch.float64, device="cuda"); nvalid = torch.full((12,), 77, dtype=torch.int32, device="cuda")
    eng.bounds_batch_device(t, bounds, nvalid)
    assert np.array_equal(_host(nvalid), nv) and np.array_equal(_host(bounds), bd)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(VEHICLES))
def test_device_collision_check_and_dense_output_at_the_vehicles_and_spacings(binding, oracle, name):
    """make_car and densify_kernel's spacing: po_postcheck_batch per vehicle, po_densify_batch per vehicle and output spacing, against the portable oracle with the
    bars of tests/test_post_step.py (decisions equal) and tests/test_glue_edges.py / test_map_edges.py (counts equal, rows within 1e-9, zero beyond), and a capacity
    that is one sample short at the finer spacing only: n_out = -2, ok = 0 for the paths it is short for, as po_hip.h says."""
    post, dense = post_inputs(), dense_inputs()
    for spacing in SPACINGS:
        eng = _engine(binding, big_map(), VEHICLES[name], output_spacing=spacing)
        p = settings(oracle, VEHICLES[name], output_spacing=spacing)
        with oracle.portable_math():
            o = st_dense(oracle, p, 400)
        out, n, ok = eng.densify_batch(dense["states"], dense["info"], 400)
        assert np.array_equal(n, o["n"]) and np.array_equal(ok, o["ok"]), (spacing, n, o["n"])
        for k in range(8):
            assert not out[k, max(n[k], 0):].any()
            if n[k] > 0:
                assert np.abs(out[k, :n[k]] - o["rows"][k]).max() < 1e-9
                assert np.allclose(np.diff(out[k, :n[k], 4]), spacing, rtol=0, atol=1e-9)
        if spacing == SPACINGS[0]:
            with oracle.portable_math():
                q = st_post(oracle, p)
            nv, okp = eng.postcheck_batch(post["states"], TE._solved(16))
            assert np.array_equal(nv, q["post_nv"]) and np.array_equal(okp, q["post_ok"])
            pose_states = np.zeros((1, 600, 5)); pose_states[0, :, :3] = post["poses"]
            # single poses through the same kernel: a path of one state per pose would be 600 launches; a walk stops at the first collision, so walk 600 paths of 1 state
            nv1, _ = eng.postcheck_batch(np.ascontiguousarray(pose_states.reshape(600, 1, 5)), TE._solved(600))
            assert np.array_equal(nv1, q["free"].astype(np.int32))
    # the capacity: the longest complete walk at 0.3 m fits M exactly; at 0.1 m the same M is short for every path that is longer than M samples
    p3, p1 = settings(oracle, VEHICLES[name]), settings(oracle, VEHICLES[name], output_spacing=0.1)
    with oracle.portable_math():
        full3, full1 = st_dense(oracle, p3, 400), st_dense(oracle, p1, 400)
        M = int(full1["n"].max()) - 1
        o3, o1 = st_dense(oracle, p3, M), st_dense(oracle, p1, M)
    assert M > full3["n"].max() and np.array_equal(o3["n"], full3["n"]) and (o1["n"] == -2).sum() >= 1 and (o1["n"][full1["n"] <= M] == full1["n"][full1["n"] <= M]).all()
    for spacing, want in ((0.3, o3), (0.1, o1)):
        eng = _engine(binding, big_map(), VEHICLES[name], output_spacing=spacing)
        out, n, ok = eng.densify_batch(dense["states"], dense["info"], M)
        assert np.array_equal(n, want["n"]) and np.array_equal(ok, want["ok"]) and not ok[n == -2].any(), (spacing, n, want["n"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEARCHES))
def test_device_search_at_the_lattices(binding, oracle, name):
    """DevSearch{range, long_spacing, lat_spacing} in both launch variants, bit for bit against the portable oracle as tests/test_map_edges.py does.  "edge64" lays out
    63 lateral samples (lanes 0 .. 62; test_table_rows counts them) one rounding error below the 64-sample limit; "fine" needs more layers than SEARCH_CAP_SHORT."""
    sp, length, start = search_inputs()
    eng = _engine(binding, TE._c_map("plan"), SEARCHES[name])
    with oracle.portable_math():
        o = st_search(oracle, settings(oracle, SEARCHES[name]))
        short = st_search(oracle, settings(oracle, SEARCHES[name]), SEARCH_CAP_SHORT)
    for one_wave, waves in ((1, 1), (0, 8)):
        eng.debug_set("dp_one_wave", one_wave)
        got = TE._search(eng, sp, length, start, SEARCH_CAP)
        assert eng.debug_get("dp_waves_used") == waves
        for k in o:
            assert np.array_equal(got[k], o[k]), (waves, k)
        got = TE._search(eng, sp, length, start, SEARCH_CAP_SHORT)
        for k in short:
            assert np.array_equal(got[k], short[k]), (waves, k, "short")
    if name == "fine":  # flagged, not truncated — the far vehicle too: the capacity is met before the vehicle's offset is looked at
        assert (short["n_layers"] == -2).all() and not short["layer_s"].any() and o["n_layers"][7] == -1
    else:
        assert (short["n_layers"] > 0).all()


@pytest.mark.gpu
def test_device_search_refuses_a_lattice_wider_than_a_wave(binding):
    """More than 64 lateral samples: PO_ERR_UNSUPPORTED from both entries, nothing launched (no search variant recorded, the outputs as they were)."""
    import torch

    sp, length, start = search_inputs()
    eng = _engine(binding, TE._c_map("plan"), SEARCH_REFUSED)
    with pytest.raises(binding.PoError, match=r"rc=%d\b" % PO_ERR_UNSUPPORTED):
        eng.dp_search_batch(sp, length, start, SEARCH_CAP)
    t = {k: _dev(sp[k]) for k in KNOT_KEYS}
    t["length"] = _dev(length)
    out = {k: torch.full((8, SEARCH_CAP), 7.0, dtype=torch.float64, device="cuda") for k in ("layer_s", "lb", "ub")}
    out["l0"] = torch.full((8,), 7.0, dtype=torch.float64, device="cuda"); out["n_layers"] = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    with pytest.raises(binding.PoError, match=r"rc=%d\b" % PO_ERR_UNSUPPORTED):
        eng.dp_search_batch_device(t, _dev(start), SEARCH_CAP, out)
    assert eng.debug_get("dp_waves_used") == 0
    assert all((_host(out[k]) == 7.0).all() for k in ("layer_s", "lb", "ub", "l0")) and (_host(out["n_layers"]) == 77).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", TS.KINDS)
def test_device_smoothers_at_the_weights_and_admm_settings(binding, oracle, kind):
    """assemble<KIND>'s weights and every ADMM setting of the smoothers, one at a time, through _compare of tests/test_smooth.py with its tolerances unchanged.  With
    six instances its 90 % shares mean every instance (test_oracle_modes_agree_on_the_smoothing_runs is the CPU side of that)."""
    inp = smooth_inputs(kind)
    m = mod_map(smooth_map())
    eng = _engine(binding, smooth_map(), WEIGHTS["other"])
    dev = eng.smooth_batch(kind, inp, want_raw=True)
    orc = oracle.smooth_batch(kind, settings(oracle, WEIGHTS["other"]), inp, m_map=m, want_raw=True)
    assert (dev[3]["status"] == PO_STATUS_SOLVED).all()
    TS._compare(kind, dev, orc, inp)
    for name in sorted(ADMM):
        eng = _engine(binding, smooth_map(), ADMM[name])
        dev, orc = eng.smooth_batch(kind, inp, want_raw=True), oracle_smooth(oracle, kind, name)
        try:
            TS._compare(kind, dev, orc, inp)
            assert np.array_equal(dev[3]["iters"], orc[3]["iters"])  # the allowance of _compare is not used
            if name == "max_iter" and kind > 0:  # (kind 0 is solved at iteration 50: ADMM_NOT_LIVE)
                hit = orc[3]["status"] == PO_STATUS_MAX_ITER
                assert hit.any() and (dev[3]["iters"][hit] == 50).all() and np.array_equal(dev[3]["status"], orc[3]["status"])
            if name == "no_adapt":
                assert not dev[3]["n_refactor"].any()
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


@pytest.mark.gpu
def test_device_limits_and_speed_at_the_second_friction_and_vehicle(binding, oracle):
    """limits_kernel's mu and max_curvature_rate, bitwise as tests/test_plan_stages.py; po_speed_batch with the clearance cap on, whose six circles come from make_car,
    at the van and the second friction pair, host and device entry bitwise against tests/speed_ref.py as tests/test_speed.py holds it."""
    import test_speed as SP

    v, a = limits_inputs()
    eng = _engine(binding, None, FRICTION["other"])
    mk, mkp = eng.limits_batch(v, a)
    o = st_limits(oracle, settings(oracle, FRICTION["other"]))
    assert np.array_equal(mk, o["max_k"], equal_nan=True) and np.array_equal(mkp, o["max_kp"])
    eng.close()
    p = settings(oracle, VEHICLES["van"], FRICTION["other"])
    eng = _engine(binding, SP.layer(), VEHICLES["van"], FRICTION["other"])
    st = SP.make_paths(7, 6, 40)
    v0 = np.linspace(0.5, 6.0, 6)
    sp = SP.with_map(a_lat_max=5.0)  # above the default friction limit 0.4 g, allowed at 0.7 g
    want = speed_ref.profile(p, st, v0, sp, maps=[SP.omap(oracle)])
    base = speed_ref.profile(settings(oracle, FRICTION["other"]), st, v0, sp, maps=[SP.omap(oracle)])
    assert not SP.same(want["v"], base["v"]) and (want["status"] > 0).all()  # the car is live in the clearance cap
    SP.assert_same(eng.speed_batch(st, v0, params=sp), want, tag="host")
    SP.assert_same(SP.run_device(eng, st, v0, sp), want, tag="device")
    eng.close()


def _plan(eng, sc, N=PLAN_N, **kw):
    return dict(zip(("states", "n", "ok", "stage", "info"), eng.plan_batch(sc["way_x"], sc["way_y"], sc["start"], sc["goal"], N=N, **kw)))


@pytest.mark.gpu
@pytest.mark.parametrize("raw", (1, 0))
def test_device_plan_at_the_combined_setting(binding, oracle, raw):
    """po_plan_batch with the compact car, the fine lattice (Lc in po_plan.cpp follows search_long_spacing = 1.0) and output spacing 0.45 in both output branches,
    against oracle.path_optimizer_solve with the bars of tests/test_pipeline.py: verdict, count and QP iterations equal, states within 1e-6."""
    sc = plan_scenes()
    eng = _engine(binding, sc["map"], COMBINED, enable_raw_output=raw)
    r = _plan(eng, sc)
    want = st_plan(oracle, settings(oracle, COMBINED, enable_raw_output=raw))
    assert not r["stage"].any()
    for b, (ok, path, iters) in enumerate(want):
        assert bool(r["ok"][b]) == ok and r["n"][b] == len(path) and int(r["info"]["iters"][b]) == iters, (b, r["n"][b], len(path), r["info"]["iters"][b], iters)
        assert np.abs(r["states"][b, :r["n"][b]] - path).max() < 1e-6 and not r["states"][b, r["n"][b]:].any(), b


LONG_WAY = 88  # waypoints every 3 m: a 261 m route, whose lattice at search_long_spacing = 0.5 has more than 512 layers


@functools.lru_cache(maxsize=None)
def long_route():
    """Two instances on a free 300 m x 300 m layer (600 x 600 cells of 0.5 m): a gently curving route of LONG_WAY waypoints and its own first 12 waypoints."""
    s = 3.0 * np.arange(LONG_WAY)
    z = 0.3 * np.sin(s / 60.0)
    x = -125.0 + np.concatenate(([0.0], np.cumsum(3.0 * np.cos(z[:-1])))); y = -20.0 + np.concatenate(([0.0], np.cumsum(3.0 * np.sin(z[:-1]))))
    wx = np.stack([x, np.where(np.arange(LONG_WAY) < 12, x, 0.0)]); wy = np.stack([y, np.where(np.arange(LONG_WAY) < 12, y, 0.0)])
    start = np.array([[x[0], y[0], z[0], 0.0]] * 2)
    goal = np.array([[x[-1], y[-1], z[-1]], [x[11], y[11], z[11]]])
    return TE._frozen(dict(way_x=wx, way_y=wy, n_way=np.array([LONG_WAY, 12], dtype=np.int32), start=start, goal=goal,
                           map=(np.full((600, 600), 10.0, dtype=np.float32), 0.5, 0.0, 0.0)))


def test_long_route_needs_more_than_512_layers(oracle):
    """CPU side of the Lc test: at search_long_spacing = 0.5 the oracle's search on the long instance asks for more than its 512 layers (n_layers = -2 inside
    path_optimizer_solve, which then gives up), the short instance plans; at the default spacing the long search fits (the spacing is what overruns)."""
    sc = long_route()
    m = mod_map(sc["map"])
    p = settings(oracle, search_long_spacing=0.5)
    ok, path, tr = oracle.path_optimizer_solve(p, m, sc["way_x"][0], sc["way_y"][0], sc["start"][0], sc["goal"][0])
    assert not ok and tr["dp"][0] == -2
    ok, path, tr = oracle.path_optimizer_solve(p, m, sc["way_x"][1, :12], sc["way_y"][1, :12], sc["start"][1], sc["goal"][1])
    assert ok and len(path) > 20
    ok, path, tr = oracle.path_optimizer_solve(settings(oracle), m, sc["way_x"][0], sc["way_y"][0], sc["start"][0], sc["goal"][0])
    assert tr["dp"][0] > 100
    # why the chain's layer capacity stops below the search's own 512: the layers are the stride of postSmooth's QP, which must fit 160 KB of LDS
    from path_optimizer_amd import binding

    f = binding.lib().po_smooth_lds_bytes
    f.restype, f.argtypes = C.c_size_t, [C.c_int, C.c_int]
    assert f(2, 512) > 160 * 1024 >= f(2, 473) and f(2, 440) > 160 * 1024 and all(f(2, L) <= 160 * 1024 for L in range(4, 440))


@pytest.mark.gpu
def test_device_plan_layer_capacity_at_a_fine_long_spacing(binding, oracle):
    """Lc in po_plan.cpp: a 261 m route at search_long_spacing = 0.5 needs more layers than the chain has room for.  po_hip.h: that instance comes back with stage 9
    (capacity), ok 0 and no states; the call returns PO_OK and the other instance of the batch is planned as if it were alone.  (Before this test the capacity was
    min(512, ...), a stride at which postSmooth's QP does not fit on chip: the whole call came back PO_ERR_UNSUPPORTED, the short instance with it.)"""
    sc = long_route()
    eng = _engine(binding, sc["map"], search_long_spacing=0.5)
    r = _plan(eng, sc, N=512, n_way=sc["n_way"])
    assert r["stage"][0] == 9 and not r["ok"][0] and r["n"][0] == 0 and not r["states"][0].any()
    ok, path, tr = oracle.path_optimizer_solve(settings(oracle, search_long_spacing=0.5), mod_map(sc["map"]), sc["way_x"][1, :12], sc["way_y"][1, :12], sc["start"][1], sc["goal"][1])
    assert r["stage"][1] == 0 and bool(r["ok"][1]) == ok and r["n"][1] == len(path) and int(r["info"]["iters"][1]) == int(tr["qp"]["iters"])
    assert np.abs(r["states"][1, :r["n"][1]] - path).max() < 1e-6


@pytest.mark.gpu
def test_device_argument_checks_on_the_settings(binding):
    """What po_hip.h says of a non-positive or NaN setting, with nothing launched (outputs keep the values they were filled with):
    search_lat_spacing -> PO_ERR_UNSUPPORTED from po_dp_search_batch*; output_spacing -> PO_ERR_INVALID from po_densify_batch*, and from po_plan_batch* when the raw
    output branch would re-sample with it (also for a spacing below the 0.15 m of the dense step: the reference's CHECK_LE).  car_width is NOT validated (po_hip.h
    says so): no call is made with such a car here."""
    import torch

    sp, length, start = search_inputs()
    dense = dense_inputs()
    sc = plan_scenes()
    t = {k: _dev(sp[k]) for k in KNOT_KEYS}
    t["length"] = _dev(length)
    states, info = _dev(dense["states"]), _dev(dense["info"].view(np.uint8).reshape(8, -1))
    for bad in (0.0, -0.6, float("nan")):
        eng = _engine(binding, TE._c_map("plan"), search_lat_spacing=bad)
        out = {k: torch.full((8, SEARCH_CAP), 7.0, dtype=torch.float64, device="cuda") for k in ("layer_s", "lb", "ub")}
        out["l0"] = torch.full((8,), 7.0, dtype=torch.float64, device="cuda"); out["n_layers"] = torch.full((8,), 77, dtype=torch.int32, device="cuda")
        with pytest.raises(binding.PoError, match=r"rc=%d\b" % PO_ERR_UNSUPPORTED):
            eng.dp_search_batch_device(t, _dev(start), SEARCH_CAP, out)
        with pytest.raises(binding.PoError, match=r"rc=%d\b" % PO_ERR_UNSUPPORTED):
            eng.dp_search_batch(sp, length, start, SEARCH_CAP)
        assert eng.debug_get("dp_waves_used") == 0 and (_host(out["n_layers"]) == 77).all() and (_host(out["layer_s"]) == 7.0).all()
        eng = _engine(binding, big_map(), output_spacing=bad)
        o_states = torch.full((8, 400, 5), 7.0, dtype=torch.float64, device="cuda")
        n_out = torch.full((8,), 77, dtype=torch.int32, device="cuda"); ok = torch.full((8,), 77, dtype=torch.int32, device="cuda")
        ptr = lambda x: C.c_void_p(x.data_ptr())
        assert binding.lib().po_densify_batch_device(eng._h, 8, 50, None, ptr(states), ptr(info), 400, ptr(o_states), ptr(n_out), ptr(ok)) == PO_ERR_INVALID
        with pytest.raises(binding.PoError, match=r"rc=%d\b" % PO_ERR_INVALID):
            eng.densify_batch(dense["states"], dense["info"], 400)
        assert (_host(n_out) == 77).all() and (_host(ok) == 77).all() and (_host(o_states) == 7.0).all()
    for bad in (0.0, -0.3, float("nan"), 0.1):
        eng = _engine(binding, sc["map"], output_spacing=bad)
        with pytest.raises(binding.PoError, match=r"rc=%d\b" % PO_ERR_INVALID):
            _plan(eng, sc)
    r = _plan(_engine(binding, sc["map"], output_spacing=0.1, enable_raw_output=0), sc, N=512)  # the dense branch re-samples at 0.5 / 1.0 and samples every 0.1: fine
    assert r["ok"].all() and all(np.allclose(np.diff(r["states"][b, :r["n"][b], 4]), 0.1, rtol=0, atol=1e-9) for b in range(PLAN_B))
