"""The speed profile: po_speed_batch* (csrc/po_speed.hip; include/po_hip.h states the definition).

Every v, a, t, total time and status is a fixed sequence of rounded IEEE double operations, so every comparison with the device here is BIT equality on byte views
against tests/speed_ref.py (numpy, one ufunc per operation); the only tolerances are the closed forms of the hand cases, 1e-12 relative: at most 512 accumulated
roundings of 2^-53 each, about 6e-14.

CPU: the reference against a scalar loop over the definition, hand cases with closed forms, properties of the reference on random inputs, every status-0 trigger,
updateLimits (the oracle's) on the reference's output including an interval whose unclamped acceleration exceeds A by an ulp, exports and the ABI mirror,
argument checks without a device, the kernel's tile constant against the one the boundary cases use, the host mirror's header and test program compile and link.
GPU: path lengths around the LDS tile and the wave, batch sizes around the workgroup of 64 paths, position in the batch, every cap alone, zero and negative ds,
the status-2 threshold, end speeds, status-0 triggers, NULL optional outputs, empty calls, the map stack, the chain plan -> select -> speed -> limits on one stream,
the C++ mirror's program against the Python call, host validation."""
import ctypes
import functools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import select_ref
import speed_ref
from path_optimizer_amd import abi, binding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["po_default_speed_params", "po_speed_batch", "po_speed_batch_device"]
KEYS = ("v", "a", "t", "total_time", "status")
SX, SY, RES = 120, 90, 0.2
SPEED_TILE = 16  # kSpeedTile of po_speed.hip: states per LDS tile of the sweeps
T = SPEED_TILE


def test_boundary_cases_follow_the_kernel_constant():
    """The tile-boundary lengths below are built from SPEED_TILE: it must be the kernel's own constant."""
    import re

    src = open(os.path.join(ROOT, "path_optimizer_amd", "csrc", "po_speed.hip")).read()
    assert int(re.search(r"constexpr int kSpeedTile = (\d+);", src).group(1)) == SPEED_TILE


def same(a, b):
    """Bitwise equality of two arrays (any dtype)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(got, want, keys=KEYS, tag=""):
    for k in keys:
        if not same(got[k], want[k]):
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert g.shape == w.shape and g.dtype == w.dtype, (tag, k, g.shape, w.shape, g.dtype, w.dtype)
            bad = np.flatnonzero((g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)).any(axis=1))
            raise AssertionError(f"{tag} {k}: paths {bad[:8]} differ; got {g[bad[0]]} want {w[bad[0]]}")


@functools.lru_cache(maxsize=None)
def layer(seed=1, pos=(2.0, -1.0)):
    d, res, px, py, _ = synth.make_distance_map(seed, SX, SY, RES, pos=pos, n_obstacles=10, r_range=(0.3, 1.2))
    d.setflags(write=False)
    return d, res, px, py


def omap(oracle, seed=1, pos=(2.0, -1.0)):
    return oracle.make_map(*layer(seed, pos))


def make_paths(seed, B, N, ds=0.3, box=6.0, centre=(2.0, -1.0)):
    """B smooth paths of N states (x, y, heading, k, s) that start inside the map (24 m x 18 m around `centre`); long ones leave it.  Curvatures up to 0.18 1/m
    that change by up to 0.05 1/m^2: with the default parameters the lateral and the rate cap both bite."""
    rng = np.random.default_rng([24, seed])
    st = np.zeros((B, N, 5))
    for b in range(B):
        step = ds * rng.uniform(0.7, 1.3, N - 1) if N > 1 else np.zeros(0)
        s = np.concatenate(([0.0], np.cumsum(step)))
        k = rng.uniform(0, 0.15) * np.sin(s / rng.uniform(3, 9) + rng.uniform(0, 6.28)) + rng.uniform(-0.03, 0.03)
        z = rng.uniform(-math.pi, math.pi) + np.concatenate(([0.0], np.cumsum(0.5 * (k[1:] + k[:-1]) * step)))
        x = centre[0] + rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(np.cos(z[:-1]) * step)))
        y = centre[1] + rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(np.sin(z[:-1]) * step)))
        st[b] = np.stack([x, y, z, k, s], axis=1)
    return st


def straight(n, ds, k=0.0):
    st = np.zeros((1, n, 5))
    st[0, :, 0] = ds * np.arange(n); st[0, :, 3] = k; st[0, :, 4] = ds * np.arange(n)
    return st


def with_map(**kw):
    sp = binding.default_speed_params()
    sp.use_map = 1
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


def no_map(**kw):
    sp = binding.default_speed_params()
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def _scalar_profile(params, sp, st, n, v0, v_end, limit, okb, m, oracle):
    """The definition as a plain scalar Python loop over ONE path (Python floats are IEEE doubles; every operation rounds once).  st [N, 5]."""
    N = len(st)
    n = min(max(int(n), 0), N)
    zero = dict(v=[0.0] * N, a=[0.0] * N, t=[0.0] * N, total_time=0.0, status=0)
    fin = lambda x: abs(x) <= select_ref.DBL_MAX  # False for NaN and +-inf
    mn = lambda a, b: b if b < a else a
    mx = lambda a, b: b if b > a else a
    v0 = float(v0)
    if okb == 0 or n < 2 or not (fin(v0) and v0 >= 0):
        return zero
    x, y, z, k, s = ([float(v) for v in st[:n, c]] for c in range(5))
    if not all(fin(v) for v in k + s) or (sp.use_map and not all(fin(v) for v in x + y + z)):
        return zero
    A = params.mu * 9.8
    R = params.max_curvature_rate
    rate = lambda j: (abs(k[j + 1] - k[j]) / (s[j + 1] - s[j])) if (s[j + 1] - s[j]) > 0 else 0.0
    W = [0.0] * n
    if sp.use_map:
        L = select_ref.trig_lib()
        cx, cy, cr = ([float(v) for v in arr] for arr in select_ref.car_circles(params))
    for i in range(n):
        Wi = sp.v_max * sp.v_max
        ak = abs(k[i])
        if ak > 0:
            Wi = mn(Wi, sp.a_lat_max / ak)
        rr = 0.0
        if i > 0:
            rr = mx(rr, rate(i - 1))
        if i < n - 1:
            rr = mx(rr, rate(i))
        if rr > 0:
            q = R / rr
            Wi = mn(Wi, q * q)
        if limit is not None:
            l = float(limit[i])
            if l >= 0:
                Wi = mn(Wi, l * l)
        if sp.use_map:
            cz, sz = L.po_oracle_pcos(z[i]), L.po_oracle_psin(z[i])
            ci = None
            for q in range(6):
                gx = (cx[q] * cz - cy[q] * sz) + x[i]
                gy = (cx[q] * sz + cy[q] * cz) + y[i]
                cq = float(oracle.map_distance(m, [[gx, gy]])[0][0]) - cr[q]
                ci = cq if q == 0 else mn(ci, cq)
            cc = ci if ci > 0 else 0.0
            vc = sp.clear_v0 + sp.clear_gain * cc
            Wi = mn(Wi, vc * vc)
        W[i] = Wi
    d = [(s[i + 1] - s[i]) if (s[i + 1] - s[i]) > 0 else 0.0 for i in range(n - 1)]
    w = [0.0] * n
    w[0] = mn(W[0], v0 * v0)
    for i in range(n - 1):
        lat = w[i] * abs(k[i])
        rem = A * A - lat * lat
        rem = rem if rem > 0 else 0.0
        ax = mn(math.sqrt(rem), sp.a_max)
        w[i + 1] = mn(W[i + 1], w[i] + (2 * ax) * d[i])
    if v_end is not None:
        e = float(v_end)
        if fin(e) and e >= 0:
            w[n - 1] = mn(w[n - 1], e * e)
    for i in range(n - 2, -1, -1):
        lat = w[i + 1] * abs(k[i + 1])
        rem = A * A - lat * lat
        rem = rem if rem > 0 else 0.0
        bx = mn(math.sqrt(rem), sp.b_max)
        w[i] = mn(w[i], w[i + 1] + (2 * bx) * d[i])
    v = [math.sqrt(wi) for wi in w] + [0.0] * (N - n)
    a, t = [0.0] * N, [0.0] * N
    for i in range(n - 1):
        ds = s[i + 1] - s[i]
        ai = (w[i + 1] - w[i]) / (2 * ds) if ds > 0 else 0.0
        a[i] = mx(-A, mn(ai, A))
        vs = v[i] + v[i + 1]
        t[i + 1] = t[i] + ((2 * d[i]) / vs if vs > 0 else 0.0)
    return dict(v=v, a=a, t=t, total_time=t[n - 1], status=2 if w[0] < v0 * v0 else 1)


def random_case(seed, B, N):
    """Ragged paths with start speeds, end speeds (some free, some NaN / negative = free), per-state limits with negative and NaN entries."""
    rng = np.random.default_rng([25, seed])
    st = make_paths(seed, B, N, box=3.0)
    n = rng.integers(0, N + 1, B).astype(np.int32)
    n[rng.integers(0, B)] = N
    v0 = rng.uniform(0, 6, B)
    v_end = rng.uniform(0, 4, B)
    v_end[rng.random(B) < 0.3] = -1.0
    v_end[rng.random(B) < 0.1] = np.nan
    lim = rng.uniform(1, 9, (B, N))
    lim[rng.random((B, N)) < 0.6] = -1.0
    lim[rng.random((B, N)) < 0.1] = np.nan
    return dict(states=st, v0=v0, n_states=n, v_end=v_end, v_limit=lim)


def test_reference_agrees_with_a_scalar_loop_over_the_definition(oracle):
    params = oracle.default_params()
    m = omap(oracle)
    for case, (N, use_map) in enumerate([(23, False), (40, True), (7, False)]):
        sp = with_map() if use_map else no_map()
        c = random_case(case, 12, N)
        st = c["states"]
        if N > 6:
            st[1, 2, 4] = st[1, 1, 4]  # ds = 0
            st[1, 4, 4] = st[1, 3, 4] - 0.1  # ds < 0
            st[2, 3:6, 3] = 0.0  # k = 0 rows
            st[3, N - 1, 0] += 100.0  # a state outside the map
        ok = np.ones(12, dtype=np.int32); ok[5] = 0
        got = speed_ref.profile(params, st, c["v0"], sp, n_states=c["n_states"], ok=ok, v_end=c["v_end"], v_limit=c["v_limit"], maps=[m])
        for b in range(12):
            want = _scalar_profile(params, sp, st[b], c["n_states"][b], c["v0"][b], c["v_end"][b], c["v_limit"][b], ok[b], m, oracle)
            for key in ("v", "a", "t"):
                assert same(got[key][b], np.array(want[key])), (case, b, key)
            assert same(got["total_time"][b], np.float64(want["total_time"])) and got["status"][b] == want["status"], (case, b)
        assert set(got["status"].tolist()) >= {0, 1}


def test_hand_cases(oracle):
    params = oracle.default_params()
    A = params.mu * 9.8
    n, ds = 100, 0.25
    st = straight(n, ds)
    s = st[0, :, 4]
    L = s[-1]
    sp = no_map(v_max=7.0)  # a_max = 2, b_max = 3 < A = 3.92: on a straight path the friction circle leaves both caps alone
    assert sp.a_max < A and sp.b_max < A
    r = speed_ref.profile(params, st, [0.0], sp)
    want = np.minimum(2 * sp.a_max * s, sp.v_max ** 2)
    assert np.abs(r["w"][0] - want).max() <= 1e-12 * want.max() and (want == sp.v_max ** 2).any() and r["status"][0] == 1
    r = speed_ref.profile(params, st, [0.0], sp, v_end=[0.0])
    want = np.minimum(np.minimum(2 * sp.a_max * s, sp.v_max ** 2), 2 * sp.b_max * (L - s))
    assert np.abs(r["w"][0] - want).max() <= 1e-12 * want.max() and r["v"][0, -1] == 0.0 and r["v"][0, 0] == 0.0
    assert (want == sp.v_max ** 2).any() and (want == 2 * sp.b_max * (L - s)).sum() > 5
    # times of the acceleration ramp: v = a_max t
    ramp = 2 * sp.a_max * s < sp.v_max ** 2
    assert np.abs(r["t"][0][ramp] - r["v"][0][ramp] / sp.a_max).max() <= 1e-2  # (trapezoid in v over an interval that starts at rest: not a closed form, a sanity bound)
    # a constant-curvature arc: the interior sits at sqrt(a_lat_max / |k|)
    for k in (0.1, -0.1):
        st = straight(200, 0.25, k)
        r = speed_ref.profile(params, st, [0.0], no_map())
        cap = np.sqrt(np.float64(3.0) / np.float64(0.1))
        assert (r["v"][0, 100:] == cap).all() and (r["v"][0, :5] < cap).all() and (r["a"][0, 100:] == 0).all()


def test_properties_of_the_reference(oracle):
    params = oracle.default_params()
    A = float(speed_ref.friction(params))
    m = omap(oracle)
    for seed, sp in ((1, no_map()), (2, with_map()), (3, no_map(a_max=10.0, b_max=10.0))):
        c = random_case(10 + seed, 40, 50)
        r = speed_ref.profile(params, maps=[m], sp=sp, **c)
        n, prof = np.clip(c["n_states"], 0, 50), r["status"] > 0
        assert prof.sum() > 25 and (r["status"][n < 2] == 0).all()
        assert (r["w"] <= r["W"]).all() and (r["W"] <= sp.v_max ** 2).all()
        assert (r["a"] >= -A).all() and (r["a"] <= A).all()
        ds = np.diff(c["states"][:, :, 4], axis=1)
        # a_i <= min(a_max, A) up to the rounding of w_i + 2 ax d and of the difference: 2 eps w in the numerator, over 2 ds
        slack = np.finfo(float).eps * sp.v_max ** 2 / np.where(ds > 0, ds, 1.0)
        assert (r["a"][:, :-1] <= min(sp.a_max, A) * (1 + 4 * np.finfo(float).eps) + slack).all()
        assert (np.diff(r["t"], axis=1)[:, :] >= 0)[np.arange(49)[None, :] < (n[:, None] - 1)].all()
        for b in np.flatnonzero(prof):
            assert r["total_time"][b] == r["t"][b, n[b] - 1] and not r["v"][b, n[b]:].any() and not r["t"][b, n[b]:].any() and r["a"][b, n[b] - 1] == 0
        v0 = c["v0"]
        assert ((r["status"] == 2) == (prof & (r["w"][:, 0] < v0 * v0))).all() and (r["status"] == 2).any() and (r["status"] == 1).any()
    # status 2 means what it says: entering above the cap of state 0, or too fast to brake for an end speed of 0
    st = straight(20, 0.5)
    assert speed_ref.profile(params, st, [3.0], no_map(), v_limit=np.full((1, 20), 3.0))["status"][0] == 1
    assert speed_ref.profile(params, st, [3.5], no_map(), v_limit=np.full((1, 20), 3.0))["status"][0] == 2
    assert speed_ref.profile(params, st, [7.0], no_map(), v_end=[0.0])["status"][0] == 1  # 49 <= 2 * 3 * 9.5
    assert speed_ref.profile(params, st, [8.0], no_map(), v_end=[0.0])["status"][0] == 2  # 64 > 57


def status0_cases(N=12):
    """(tag, use_map, keyword changes) of every trigger of 'not profiled', and two inputs that must NOT trigger it."""
    def poke(col, val, row=5):
        def f(c):
            c["states"] = c["states"].copy(); c["states"][1, row, col] = val
        return f

    def setk(key, val):
        def f(c):
            c[key] = np.array(c[key], dtype=np.float64 if key != "ok" and key != "n_states" else np.int32).copy(); c[key][1] = val
        return f

    cases = [("ok", 0, setk("ok", 0), 0), ("n=1", 0, setk("n_states", 1), 0), ("n=0", 0, setk("n_states", 0), 0), ("n<0", 0, setk("n_states", -4), 0),
             ("v0 nan", 0, setk("v0", np.nan), 0), ("v0 inf", 0, setk("v0", np.inf), 0), ("v0 < 0", 0, setk("v0", -0.5), 0),
             ("k nan", 0, poke(3, np.nan), 0), ("k inf", 0, poke(3, -np.inf), 0), ("s nan", 0, poke(4, np.nan), 0), ("s inf", 0, poke(4, np.inf), 0),
             ("x nan map", 1, poke(0, np.nan), 0), ("y inf map", 1, poke(1, np.inf), 0), ("z nan map", 1, poke(2, np.nan), 0),
             ("x nan no map", 0, poke(0, np.nan), 1), ("k nan beyond n", 0, poke(3, np.nan, N - 1), 1), ("v0 = 0", 0, setk("v0", 0.0), 1),
             ("n > N", 0, setk("n_states", N + 50), 1)]  # read clamped to N, as in the device entry, which cannot validate its table
    return cases


def status0_inputs(N=12):
    st = make_paths(30, 3, N, box=2.0)
    return dict(states=st, v0=np.array([2.0, 3.0, 1.0]), n_states=np.array([N, N - 1, N], dtype=np.int32), ok=np.ones(3, dtype=np.int32))


def test_status_zero_triggers_of_the_reference(oracle):
    params = oracle.default_params()
    m = omap(oracle)
    clean = speed_ref.profile(params, sp=no_map(), maps=[m], **status0_inputs())
    assert (clean["status"] > 0).all()
    for tag, use_map, change, want_status in status0_cases():
        c = status0_inputs()
        change(c)
        r = speed_ref.profile(params, sp=with_map() if use_map else no_map(), maps=[m], **c)
        assert (r["status"][1] > 0) == bool(want_status), tag
        if not want_status:
            assert not r["v"][1].any() and not r["a"][1].any() and not r["t"][1].any() and r["total_time"][1] == 0, tag
        if not use_map:
            for k in KEYS:  # the neighbours do not notice
                assert same(r[k][[0, 2]], clean[k][[0, 2]]), (tag, k)


def ulp_case():
    """Straight paths, a_max above A: every acceleration interval is friction-limited, w_{i+1} = w_i + (2 A) d_i, and the quotient (w_{i+1} - w_i) / (2 ds_i)
    lands an ulp above A on some of them."""
    rng = np.random.default_rng(41)
    st = np.zeros((8, 60, 5))
    for b in range(8):
        s = np.concatenate(([0.0], np.cumsum(rng.uniform(0.05, 0.6, 59))))
        st[b, :, 0] = s; st[b, :, 4] = s
    return st, rng.uniform(0, 3, 8)


def test_limits_on_the_profile_have_no_nan(oracle):
    params = oracle.default_params()
    A = float(speed_ref.friction(params))
    st, v0 = ulp_case()
    sp = no_map(a_max=50.0, b_max=50.0, v_max=30.0)
    r = speed_ref.profile(params, st, v0, sp, v_end=np.zeros(8))
    ds = np.diff(st[:, :, 4], axis=1)
    with np.errstate(all="ignore"):
        raw = (r["w"][:, 1:] - r["w"][:, :-1]) / (2.0 * ds)
    assert (np.abs(raw) > A).any(), "the case no longer produces an unclamped |a| above A"
    b = int(np.flatnonzero((np.abs(raw) > A).any(axis=1))[0])
    assert np.isnan(oracle.limits(params, r["v"][b], np.concatenate((raw[b], [0.0])))[0]).any()  # what the clamp is for: updateLimits on the unclamped a
    assert (np.abs(r["a"]) <= A).all() and (np.abs(r["a"]) == A).any()
    cases = [(r, 8)]
    c = random_case(50, 30, 45)
    cases.append((speed_ref.profile(params, sp=with_map(), maps=[omap(oracle)], **c), 30))
    for prof, B in cases:
        for b in range(B):
            mk, mkp = oracle.limits(params, prof["v"][b], prof["a"][b])
            assert not np.isnan(mk).any() and not np.isnan(mkp).any(), b


def test_new_symbols_and_abi_mirror():
    L = binding.lib()
    for name in NEW_ENTRIES:
        assert hasattr(L, name), name
        assert name in binding.EXPORTS
    fields = {"po_speed_params": ["v_max", "a_lat_max", "a_max", "b_max", "clear_v0", "clear_gain", "use_map"],
              "po_speed_in": ["B", "N", "states", "n_states", "ok", "v0", "v_end", "v_limit"],
              "po_speed_out": ["v", "a", "t", "total_time", "status"]}
    mirror = {"po_speed_params": abi.PoSpeedParams, "po_speed_in": abi.PoSpeedIn, "po_speed_out": abi.PoSpeedOut}
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
    sp = binding.default_speed_params()
    assert [sp.v_max, sp.a_lat_max, sp.a_max, sp.b_max, sp.clear_v0, sp.clear_gain, sp.use_map] == [15, 3, 2, 3, 1, 2, 0]


def test_null_arguments_are_refused_without_a_device():
    L = binding.lib()
    sp, si, so = binding.default_speed_params(), abi.PoSpeedIn(), abi.PoSpeedOut()
    for entry in (L.po_speed_batch, L.po_speed_batch_device):
        assert entry(None, ctypes.byref(sp), ctypes.byref(si), ctypes.byref(so)) == abi.PO_ERR_INVALID
        assert entry(None, None, None, None) == abi.PO_ERR_INVALID
    L.po_default_speed_params(None)  # a NULL struct is ignored


def test_host_mirror_header_compiles():
    inc = os.path.join(ROOT, "path_optimizer_amd", "host", "include")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "path_optimizer_amd/speed_profile.hpp"\nint main() { PathOptimizationNS::SpeedProfiler s; (void)s; return 0; }\n')
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-I", os.path.join(ROOT, "include"), src])


def test_host_mirror_speed_test_compiles_and_links():
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "speed_test"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(host, "speed_test"))
    assert "SpeedProfiler" in open(os.path.join(host, "test", "speed_test.cpp")).read()


def mirror_case():
    """The seeded case of host/test/speed_test.cpp, rebuilt with the same integer generator and the same dyadic arithmetic: bit for bit its inputs."""
    state = [24680]

    def u():
        state[0] = (state[0] * 1103515245 + 12345) & 0x7fffffff
        return (((state[0] >> 8) % 257) - 128) / 64.0

    sx, sy, B = 40, 30, 9
    i, j = np.meshgrid(np.arange(sx), np.arange(sy), indexing="ij")
    dist = (np.float32(0.125) * ((i * 7 + j * 13) % 23).astype(np.float32)).astype(np.float32)
    n = np.array([3 + (b * 7) % 37 for b in range(B)], dtype=np.int32)
    N = int(n.max())
    states = np.zeros((B, N, 5))
    for b in range(B):
        for k in range(n[b]):
            x = -9.0 + 0.5 * k + u() / 4; y = u() * 2; z = u() / 2; kk = u() / 8
            states[b, k] = (x, y, z, kk, 0.5 * k)
    v0, v_end = np.zeros(B), np.zeros(B)
    for b in range(B):
        v0[b] = 2.0 + u(); v_end[b] = -1.0 if b % 2 else 0.0
    v0[6] = 12.0
    ok = np.ones(B, dtype=np.int32); ok[4] = 0
    lim = np.full((B, N), -1.0)
    for b in range(0, B, 3):
        lim[b, :n[b]] = 3.0
    return dict(dist=dist, res=0.5, states=states, n_states=n, v0=v0, v_end=v_end, ok=ok, v_limit=lim)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0)
    e.set_map(*layer())
    yield e
    e.close()


def _dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def run_device(e, states, v0, sp=None, want=KEYS, **kw):
    """The device entry on device copies; outputs start as 7 / 77."""
    B, N = states.shape[0], states.shape[1]
    t = {"states": _dev(np.asarray(states, dtype=np.float64)), "v0": _dev(np.asarray(v0, dtype=np.float64))}
    for k in ("n_states", "ok"):
        t[k] = None if kw.get(k) is None else _dev(np.asarray(kw[k], dtype=np.int32))
    for k in ("v_end", "v_limit"):
        t[k] = None if kw.get(k) is None else _dev(np.asarray(kw[k], dtype=np.float64))
    shapes = {"v": ((B, N), np.float64), "a": ((B, N), np.float64), "t": ((B, N), np.float64), "total_time": ((B,), np.float64), "status": ((B,), np.int32)}
    out = {k: _dev(np.full(shapes[k][0], 77 if shapes[k][1] == np.int32 else 7.0, dtype=shapes[k][1])) for k in want}
    e.speed_batch_device(t, out, sp)
    return {k: _host(v) for k, v in out.items()}


def both(e, oracle, states, v0, sp=None, tag="", maps=None, **kw):
    """Host entry, device entry and the reference: all three bitwise equal.  Returns the reference's dict."""
    sp = sp or binding.default_speed_params()
    want = speed_ref.profile(oracle.default_params(), states, v0, sp, maps=maps or [omap(oracle)], **kw)
    assert_same(e.speed_batch(states, v0, params=sp, **kw), want, tag=tag + " host")
    assert_same(run_device(e, states, v0, sp, **kw), want, tag=tag + " device")
    return want


@pytest.mark.gpu
def test_path_lengths_around_the_tile_and_the_wave(eng, oracle):
    lengths = [0, 1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1, 63, 64, 65]
    N = 66
    c = random_case(60, len(lengths), N)
    c["n_states"] = np.array(lengths, dtype=np.int32)
    for sp, tag in ((no_map(), "no map"), (with_map(), "map")):
        r = both(eng, oracle, sp=sp, tag=tag, **c)
        assert r["status"][:2].tolist() == [0, 0] and (r["status"][2:] > 0).all()
    c.pop("v_end"); c.pop("v_limit")
    both(eng, oracle, sp=no_map(), tag="no options", **c)
    st = make_paths(61, 2, 5 * T + 3, ds=0.1)  # N itself, no n_states
    both(eng, oracle, st, [1.0, 4.0], with_map(), tag="N")


@pytest.mark.gpu
def test_batch_sizes_around_the_workgroup(eng, oracle):
    for B in (1, 63, 64, 65, 130):
        c = random_case(70 + B, B, 40)  # ragged n inside every workgroup of 64 paths, 0 and 1 among them
        c["n_states"][B // 2] = 1
        ok = np.ones(B, dtype=np.int32); ok[B // 3] = 0
        both(eng, oracle, sp=with_map() if B % 2 else no_map(), ok=ok, tag=f"B {B}", **c)


@pytest.mark.gpu
def test_position_in_the_batch(eng, oracle):
    c = random_case(80, 300, 35)
    c["n_states"][217] = 35
    sp = with_map()
    big = eng.speed_batch(params=sp, **c)
    assert_same(big, speed_ref.profile(oracle.default_params(), sp=sp, maps=[omap(oracle)], **c), tag="300")
    one = eng.speed_batch(params=sp, **{k: v[217:218] for k, v in c.items()})
    assert big["status"][217] > 0
    for k in KEYS:
        assert same(big[k][217:218], one[k]), k


@pytest.mark.gpu
def test_every_cap_alone(oracle):
    params = oracle.default_params()
    N = 50
    s = 0.25 * np.arange(N)
    v0 = [20.0] * 2
    top = 15.0 ** 2

    def paths(k):
        st = np.zeros((2, N, 5))
        st[:, :, 0] = 2.0 - 5.0 + s; st[:, :, 1] = -1.0; st[:, :, 3] = k; st[:, :, 4] = s
        st[1, :, 1] = 0.5
        return st

    e = binding.Engine(0)
    e.set_map(*layer())
    # only the lateral cap: constant curvature (no rate), both signs
    st = paths(0.125); st[1, :, 3] = -0.0625
    r = both(e, oracle, st, v0, no_map(), tag="lateral")
    assert (r["W"][0] == 3.0 / 0.125).all() and (r["W"][1] == 3.0 / 0.0625).all() and (r["status"] == 2).all()
    # only the rate cap: a small curvature that changes quickly (|k| <= 0.004: the lateral cap is at 750 > 225)
    k = 0.004 * np.sin(s * 3.0)
    r = both(e, oracle, paths(k), v0, no_map(), tag="rate")
    assert (r["W"][0] < top).any() and (3.0 / np.abs(k[k != 0]) > top).all()
    # only the per-state limit, with negative and NaN entries (no limit there)
    lim = np.full((2, N), 6.0); lim[0, 10:20] = -1.0; lim[0, 30:35] = np.nan; lim[1, ::3] = 2.5; lim[1, 0] = -0.0
    r = both(e, oracle, paths(0.0), v0, no_map(), v_limit=lim, tag="limit")
    assert (r["W"][0, 10:20] == top).all() and (r["W"][0, 30:35] == top).all() and (r["W"][0, :10] == 36.0).all() and r["W"][1, 0] == 0.0 and r["v"][1, 0] == 0.0
    e.close()
    # only the clearance cap: a layer built on the device from a small occupancy image, states outside the map included (clearance -r there: speed clear_v0)
    occ = np.ones((60, 40), dtype=np.uint8); occ[20:24, 10:30] = 0; occ[45, 5] = 0
    e = binding.Engine(0)
    e.set_map_occupancy(occ, 0.25, 1.0, 0.5)
    m = oracle.make_map(*e.get_map())
    st = np.zeros((2, N, 5))
    st[:, :, 0] = 1.0 - 9.0 + 0.4 * np.arange(N); st[0, :, 1] = 3.0; st[1, :, 1] = 0.4; st[1, :, 2] = 0.3; st[:, :, 4] = 0.4 * np.arange(N)
    for sp in (with_map(), with_map(clear_v0=0.0, clear_gain=5.0), with_map(clear_gain=0.0)):
        r = both(e, oracle, st, [0.5, 0.5], sp, maps=[m], tag="clearance")
        assert (r["W"] < top).any() and (r["W"][:, 0] == sp.clear_v0 ** 2).all()  # the first states lie outside the map
    e.close()


@pytest.mark.gpu
def test_zero_and_negative_ds_and_straight_rows(eng, oracle):
    st = make_paths(90, 6, 40, box=2.0)
    st[0, 5, 4] = st[0, 4, 4]; st[0, 6, 4] = st[0, 5, 4]  # two zero intervals in a row
    st[1, 9, 4] = st[1, 8, 4] - 0.2  # a negative one
    st[2, :, 4] = st[2, 0, 4]  # a path of zero length
    st[3, :, 4] = st[3, ::-1, 4].copy()  # decreasing everywhere
    st[4, 10:20, 3] = 0.0; st[5, :, 3] = 0.0
    st[4, T - 1, 4] = st[4, T, 4] = st[4, T - 2, 4]  # zero intervals across the tile boundary
    for sp in (no_map(), with_map()):
        r = both(eng, oracle, st, [2.0] * 6, sp, v_end=[1.0] * 6, tag="ds")
        assert (r["status"] > 0).all() and r["total_time"][2] == 0 and r["total_time"][3] == 0 and np.isfinite(r["t"]).all()


@pytest.mark.gpu
def test_start_speed_threshold_and_end_speeds(eng, oracle):
    st = np.repeat(straight(30, 0.5), 5, axis=0)
    lim = np.full((5, 30), -1.0); lim[:, 0] = 3.0  # W_0 = 9
    v0 = [np.nextafter(3.0, 0), 3.0, np.nextafter(3.0, 4), 0.0, 14.0]
    r = both(eng, oracle, st, v0, no_map(), v_limit=lim, tag="threshold")
    assert r["status"].tolist() == [1, 1, 2, 1, 2] and r["v"][1, 0] == 3.0 and r["v"][2, 0] == 3.0
    for v_end, tag in ((None, "free"), (np.zeros(5), "zero"), (np.full(5, 40.0), "above the cap"), (np.array([0.0, -1.0, np.nan, np.inf, 2.0]), "mixed")):
        r2 = both(eng, oracle, st, v0, no_map(), v_limit=lim, v_end=v_end, tag="v_end " + tag)
        if tag in ("free", "above the cap"):
            assert_same(r2, r, tag=tag)
        if tag == "zero":
            assert not r2["v"][:, -1].any() and r2["status"].tolist() == [1, 1, 2, 1, 2]
        if tag == "mixed":
            assert r2["v"][0, -1] == 0 and r2["v"][4, -1] == 2.0 and same(r2["v"][1:4], r["v"][1:4])
    # too fast to brake for the end: 2 * b_max * L = 87, so 9 m/s passes and 9.5 does not
    r = both(eng, oracle, st[:2], [9.0, 9.5], no_map(), v_end=[0.0, 0.0], tag="brake")
    assert r["status"].tolist() == [1, 2]


@pytest.mark.gpu
def test_status_zero_triggers(eng, oracle):
    for tag, use_map, change, want_status in status0_cases():
        c = status0_inputs()
        change(c)
        r = both(eng, oracle, sp=with_map() if use_map else no_map(), tag=tag, **c)
        assert (r["status"][1] > 0) == bool(want_status), tag


@pytest.mark.gpu
def test_optional_outputs_and_empty_calls(eng, oracle):
    c = random_case(100, 70, 20)
    sp = with_map()
    want = speed_ref.profile(oracle.default_params(), sp=sp, maps=[omap(oracle)], **c)
    for keys in (("v", "a", "status"), ("v", "a", "status", "total_time"), ("v", "a", "status", "t")):
        assert_same(run_device(eng, c["states"], c["v0"], sp, want=keys, **{k: c[k] for k in ("n_states", "v_end", "v_limit")}), want, keys=keys, tag=str(keys))
    r = eng.speed_batch(params=sp, want_t=False, **c)
    assert r["t"] is None and r["total_time"] is None
    assert_same(r, want, keys=("v", "a", "status"), tag="host, no t")
    # B = 0: PO_OK from both entries, on a handle without a map too and with use_map set; nothing is looked at
    L = binding.lib()
    bare = binding.Engine(0)
    for h in (eng, bare):
        for entry in (L.po_speed_batch, L.po_speed_batch_device):
            si = abi.PoSpeedIn(); si.N = 5
            assert entry(h._h, ctypes.byref(sp), ctypes.byref(si), ctypes.byref(abi.PoSpeedOut())) == abi.PO_OK
    # use_map = 0 works without a map; use_map = 1 does not
    r = bare.speed_batch(params=no_map(), **c)
    assert_same(r, speed_ref.profile(oracle.default_params(), sp=no_map(), **c), tag="bare")
    with pytest.raises(binding.PoError):
        bare.speed_batch(params=sp, **c)
    bare.close()


@pytest.mark.gpu
def test_map_stack(oracle):
    pos = [(2.0, -1.0), (3.5, 0.25), (-1.0, 2.0)]
    layers = [layer(s, p) for s, p in zip((1, 2, 3), pos)]
    params, sp = oracle.default_params(), with_map()
    c = random_case(110, 12, 30)
    c["n_states"][:] = np.maximum(c["n_states"], 5)
    layer_of = np.arange(12, dtype=np.int32) % 3
    e = binding.Engine(0)
    e.set_map_stack(np.stack([l[0] for l in layers]), RES, pos_xy=np.array(pos))
    e.set_map_assignment(layer_of)
    got = e.speed_batch(params=sp, **c)
    maps = [oracle.make_map(*l) for l in layers]
    assert_same(got, speed_ref.profile(params, sp=sp, maps=maps, layer_of=layer_of, **c), tag="stack")
    dev = run_device(e, c["states"], c["v0"], sp, **{k: c[k] for k in ("n_states", "v_end", "v_limit")})
    assert_same(dev, got, tag="stack device")
    e.close()
    differs = False
    for k in range(3):  # path b on layer k == the same path on a handle whose only map is layer k
        one = binding.Engine(0)
        one.set_map(*layers[k])
        alone = one.speed_batch(params=sp, **c)
        one.close()
        idx, rest = np.flatnonzero(layer_of == k), np.flatnonzero(layer_of != k)
        for key in KEYS:
            assert same(got[key][idx], alone[key][idx]), (k, key)
        differs = differs or not same(got["v"][rest], alone["v"][rest])
    assert differs  # the layers are not interchangeable: the clearance cap is read


@pytest.mark.gpu
def test_chain_plan_select_speed_limits_on_one_stream(oracle):
    """3 vehicles x 4 waypoint variants: plan, select, speed on the winners and limits on the speeds, all enqueued on the handle's stream with no synchronisation
    between the calls (the plan call synchronises once inside itself)."""
    import torch

    sc = synth.make_planning_scenes(21, 3, n_way=12, map_kw=dict(size_x=450, size_y=450), n_discs=25, near=1)
    rng = np.random.default_rng(22)
    rep = lambda a: np.repeat(a, 4, axis=0)
    wx, wy, start, goal = rep(sc["way_x"]), rep(sc["way_y"]), rep(sc["start"]), rep(sc["goal"])
    jit = rng.uniform(-0.3, 0.3, wx.shape); jit[::4] = 0; jit[:, 0] = 0; jit[:, -1] = 0
    wx, wy = wx + jit, wy - jit
    B, N, G = 12, 256, 3
    e = binding.Engine(0)
    e.set_map(*sc["map"])
    t = {"way_x": _dev(wx), "way_y": _dev(wy), "start": _dev(start), "goal": _dev(goal)}
    plan = {"states": _dev(np.zeros((B, N, 5))), "n_states": _dev(np.zeros(B, dtype=np.int32)), "ok": _dev(np.zeros(B, dtype=np.int32))}
    gs = np.arange(0, B + 1, 4).astype(np.int32)
    sel = {"best": _dev(np.zeros(G, dtype=np.int32)), "sel_states": _dev(np.full((G, N, 5), 7.0)), "sel_n": _dev(np.zeros(G, dtype=np.int32))}
    sel_in = {"states": plan["states"], "n_states": plan["n_states"], "ok": plan["ok"], "goal": t["goal"], "group_start": _dev(gs)}
    v0, v_end = np.array([3.0, 0.0, 30.0]), np.array([0.0, -1.0, 2.0])
    spd_in = {"states": sel["sel_states"], "n_states": sel["sel_n"], "v0": _dev(v0), "v_end": _dev(v_end)}
    spd = {"v": _dev(np.full((G, N), 7.0)), "a": _dev(np.full((G, N), 7.0)), "t": _dev(np.full((G, N), 7.0)), "total_time": _dev(np.full(G, 7.0)),
           "status": _dev(np.full(G, 77, dtype=np.int32))}
    mk, mkp = _dev(np.full((G, N), 7.0)), _dev(np.full((G, N), 7.0))
    sp = with_map()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    torch.cuda.synchronize()
    e.plan_batch_device(t, plan, N, 40.0)
    e.select_batch_device(sel_in, sel)
    e.speed_batch_device(spd_in, spd, sp)
    assert binding.lib().po_limits_batch_device(e._h, G, N, ptr(sel["sel_n"]), ptr(spd["v"]), ptr(spd["a"]), ptr(mk), ptr(mkp)) == abi.PO_OK
    got = {k: _host(v) for k, v in spd.items()}
    sel_states, sel_n, best = _host(sel["sel_states"]), _host(sel["sel_n"]), _host(sel["best"])
    mk, mkp = _host(mk), _host(mkp)
    e.close()
    assert (best >= 0).any() and sel_n.max() > 2 * T
    params = oracle.default_params()
    want = speed_ref.profile(params, sel_states, v0, sp, n_states=sel_n, v_end=v_end, maps=[oracle.make_map(*sc["map"])])
    assert_same(got, want, tag="chain")
    assert (got["status"][best >= 0] > 0).all() and not got["status"][best < 0].any()
    for g in range(G):
        n = int(sel_n[g])
        ok_, okp = oracle.limits(params, got["v"][g, :n], got["a"][g, :n])
        assert same(mk[g, :n], ok_) and same(mkp[g, :n], okp), g
        assert not mk[g, n:].any() and not mkp[g, n:].any()
    assert not np.isnan(mk).any() and not np.isnan(mkp).any() and not any(np.isnan(got[k]).any() for k in ("v", "a", "t", "total_time"))


@pytest.mark.gpu
def test_host_mirror_speed_program(oracle):
    """SpeedProfiler::profile end to end in its own process: the program checks its own outputs; its statuses and its checksum of v equal the Python call's."""
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "speed_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "speed_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "speed_test passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]
    printed = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("status", "checksum")}
    c = mirror_case()
    dist, res = c.pop("dist"), c.pop("res")
    e = binding.Engine(0)
    e.set_map(dist, res, 0.0, 0.0)
    sp = with_map()
    got = e.speed_batch(params=sp, **c)
    e.close()
    assert_same(got, speed_ref.profile(oracle.default_params(), sp=sp, maps=[oracle.make_map(dist, res, 0.0, 0.0)], **c), tag="mirror case")
    assert printed["status"] == got["status"].tolist() and got["status"].tolist()[4] == 0 and got["status"].tolist()[6] == 2
    rows = np.concatenate([got["v"][b, :c["n_states"][b]] for b in range(len(c["v0"]))])
    assert printed["checksum"] == [int(rows.view(np.uint64).sum(dtype=np.uint64))]


@pytest.mark.gpu
def test_host_validation(eng):
    st = make_paths(120, 4, 8, box=2.0)
    v0 = np.ones(4)
    assert eng.speed_batch(st, v0)["status"].tolist() == [1, 1, 1, 1]
    A = 0.4 * 9.8
    bad = [("v_max", 0.0), ("v_max", -1.0), ("v_max", np.inf), ("v_max", np.nan), ("a_lat_max", 0.0), ("a_lat_max", float(np.nextafter(A, 9.0))), ("a_lat_max", np.nan),
           ("a_max", 0.0), ("a_max", np.nan), ("b_max", -2.0), ("b_max", np.nan), ("clear_v0", -0.1), ("clear_v0", np.nan), ("clear_gain", -1.0), ("clear_gain", np.nan)]
    for field, val in bad:
        with pytest.raises(binding.PoError):
            eng.speed_batch(st, v0, params=no_map(**{field: val}))
    assert eng.speed_batch(st, v0, params=no_map(a_lat_max=A))["status"].tolist() == [1, 1, 1, 1]  # the upper end of the range is inside it
    L = binding.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    sp = no_map()
    v, a, status = np.zeros((4, 8)), np.zeros((4, 8)), np.zeros(4, dtype=np.int32)
    full_in = [4, 8, p(st), None, None, p(v0), None, None]
    full_out = [p(v), p(a), None, None, p(status)]
    for entry in (L.po_speed_batch, L.po_speed_batch_device):
        for drop in (2, 5):  # states, v0
            args = list(full_in); args[drop] = None
            assert entry(eng._h, ctypes.byref(sp), ctypes.byref(abi.PoSpeedIn(*args)), ctypes.byref(abi.PoSpeedOut(*full_out))) == abi.PO_ERR_INVALID
        for drop in (0, 1, 4):  # v, a, status
            args = list(full_out); args[drop] = None
            assert entry(eng._h, ctypes.byref(sp), ctypes.byref(abi.PoSpeedIn(*full_in)), ctypes.byref(abi.PoSpeedOut(*args))) == abi.PO_ERR_INVALID
        for B, N in ((-1, 8), (4, -1)):
            args = list(full_in); args[0] = B; args[1] = N
            assert entry(eng._h, ctypes.byref(sp), ctypes.byref(abi.PoSpeedIn(*args)), ctypes.byref(abi.PoSpeedOut(*full_out))) == abi.PO_ERR_INVALID
        assert entry(eng._h, None, ctypes.byref(abi.PoSpeedIn(*full_in)), ctypes.byref(abi.PoSpeedOut(*full_out))) == abi.PO_ERR_INVALID
        assert entry(eng._h, ctypes.byref(sp), None, ctypes.byref(abi.PoSpeedOut(*full_out))) == abi.PO_ERR_INVALID
        assert entry(eng._h, ctypes.byref(sp), ctypes.byref(abi.PoSpeedIn(*full_in)), None) == abi.PO_ERR_INVALID
    assert L.po_speed_batch(eng._h, ctypes.byref(sp), ctypes.byref(abi.PoSpeedIn(*full_in)), ctypes.byref(abi.PoSpeedOut(*full_out))) == abi.PO_OK
    # the map rule, with use_map only
    bare = binding.Engine(0)
    with pytest.raises(binding.PoError):  # no map
        bare.speed_batch(st, v0, params=with_map())
    bare.set_map(*layer())
    bare.set_map_assignment(np.zeros(3, dtype=np.int32))
    with pytest.raises(binding.PoError):  # the assignment covers 3 of 4 paths
        bare.speed_batch(st, v0, params=with_map())
    assert bare.speed_batch(st, v0, params=no_map())["status"].tolist() == [1, 1, 1, 1]  # ... which use_map = 0 does not ask about
    bare.set_map_assignment(np.zeros(4, dtype=np.int32))
    assert bare.speed_batch(st, v0, params=with_map())["status"].tolist() == [1, 1, 1, 1]
    bare.close()
