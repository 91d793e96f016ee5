"""Per-instance obstacle maps: a stack of M layers on the handle and an assignment of batch instances to layers (po_set_map_stack*, po_set_map_assignment*,
po_get_map_layer, po_map_sample_layer).

The yardstick is BIT equality (byte views of every element of every output) against the same instance on a fresh handle whose single map is that layer — the path
the other test files pin against the oracle and the reference-compiled binaries.  The map stages are written in explicitly rounded arithmetic, so "instance b on
layer k of a stack" and "instance b on a handle that holds layer k alone" run the same operations on the same numbers.  The CPU oracle is a second check.

The single-map runs always take the WHOLE batch (18 instances on each of three handles) and row b of the run on layer b % 3 is what the stack must reproduce: batch
size and launch shapes are the same on both sides, only the map differs.

CPU: argument checks of every new entry without a device, the declarations against a compiled C snippet, the host mirror's test source compiles and links.
GPU: install / read-back / sampling, stacks from occupancy images, every map-reading stage and po_plan_batch with an interleaved assignment, the assignment's
semantics, stream order of the device entries, the host mirror's test program."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import edt_ref
from path_optimizer_amd import abi, binding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["po_set_map_stack", "po_set_map_stack_occupancy", "po_set_map_stack_occupancy_device", "po_set_map_assignment", "po_set_map_assignment_device",
               "po_get_map_layer", "po_map_sample_layer"]
SEEDS = (11, 12, 13)
B, M = 18, 3
LAYER_OF = np.arange(B, dtype=np.int32) % M  # interleaved: neither sorted nor contiguous


def same(a, b):
    """Bitwise equality of two arrays (any dtype, structured ones included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rows_equal(got, want):
    """Per-instance bitwise equality of a tuple of [B, ...] outputs: bool [B]."""
    return np.array([all(same(g[b], w[b]) for g, w in zip(got, want)) for b in range(len(got[0]))])


def pick(refs):
    """Row b of the run on layer b % M, for every output of a stage."""
    return tuple(np.stack([refs[b % M][i][b] for b in range(B)]) for i in range(len(refs[0])))


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_new_entries_are_exported_and_check_their_arguments_without_a_device():
    L = binding.lib()
    for name in NEW_ENTRIES:
        assert name in binding.EXPORTS
        getattr(L, name)
    d = np.ones((2, 4, 4), dtype=np.float32)
    cells = np.ones((2, 4, 4), dtype=np.uint8)
    m = abi.PoMap(d.ctypes.data_as(ctypes.c_void_p), 4, 4, 0.2, 0.0, 0.0)
    occ = abi.PoOccupancy(cells.ctypes.data_as(ctypes.c_void_p), 4, 4, 0.2, 0.0, 0.0)
    pos = np.zeros((2, 2))
    tab = np.zeros(4, dtype=np.int32)
    xy = np.zeros((3, 2)); dist = np.zeros(3); ins = np.zeros(3, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # a null handle is PO_ERR_INVALID on every entry, before any device call
    assert L.po_set_map_stack(None, 2, ctypes.byref(m), p(pos)) == abi.PO_ERR_INVALID
    assert L.po_set_map_stack_occupancy(None, 2, ctypes.byref(occ), p(pos)) == abi.PO_ERR_INVALID
    assert L.po_set_map_stack_occupancy_device(None, 2, ctypes.byref(occ), p(pos)) == abi.PO_ERR_INVALID
    assert L.po_set_map_assignment(None, 4, p(tab)) == abi.PO_ERR_INVALID
    assert L.po_set_map_assignment_device(None, 4, p(tab)) == abi.PO_ERR_INVALID
    assert L.po_get_map_layer(None, 0, ctypes.byref(abi.PoMap()), None) == abi.PO_ERR_INVALID
    assert L.po_map_sample_layer(None, 0, 3, p(xy), p(dist), p(ins)) == abi.PO_ERR_INVALID


def test_declarations_match_the_header():
    """No struct is added; the prototypes, as the binding drives them, are what the header declares (a C compiler checks the assignment to typed pointers)."""
    src = ('#include <stdio.h>\n#include "po_hip.h"\n'
           'int (*a)(po_handle, int, const po_map *, const double *) = po_set_map_stack;\n'
           'int (*b)(po_handle, int, const po_occupancy *, const double *) = po_set_map_stack_occupancy;\n'
           'int (*c)(po_handle, int, const po_occupancy *, const double *) = po_set_map_stack_occupancy_device;\n'
           'int (*d)(po_handle, int, const int *) = po_set_map_assignment;\n'
           'int (*e)(po_handle, int, const int *) = po_set_map_assignment_device;\n'
           'int (*f)(po_handle, int, po_map *, float *) = po_get_map_layer;\n'
           'int (*g)(po_handle, int, int, const double *, double *, int *) = po_map_sample_layer;\n'
           'int main(){printf("%d %zu %zu\\n", PO_ABI_VERSION, sizeof(po_map), sizeof(po_occupancy));return (a && b && c && d && e && f && g) ? 0 : 1;}\n')
    lib_dir = os.path.join(ROOT, "path_optimizer_amd")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t"),
                               "-L", lib_dir, "-l:libpo_hip.so", "-Wl,-rpath," + lib_dir])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [abi.PO_ABI_VERSION, ctypes.sizeof(abi.PoMap), ctypes.sizeof(abi.PoOccupancy)]


def test_host_mirror_test_source_compiles_and_links():
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "map_stack_test"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(host, "map_stack_test"))


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _sample_points(rng, sx, sy, res, px, py, n):
    """World positions over 1.2 x the map's extent: inside and outside."""
    return np.stack([px + (rng.random(n) - 0.5) * 1.2 * sx * res, py + (rng.random(n) - 0.5) * 1.2 * sy * res], axis=1)


@pytest.mark.gpu
def test_stack_install_read_back_and_sampling(oracle):
    sx, sy, res = 63, 65, 0.25
    pos = np.array([[1.5, -2.0], [-7.25, 3.0], [40.0, 40.5]])
    layers = np.stack([synth.make_distance_map(20 + k, size_x=sx, size_y=sy, resolution=res, pos=tuple(pos[k]), n_obstacles=4, r_range=(0.3, 1.0))[0] for k in range(3)])
    e = binding.Engine(0)
    assert e.debug_get("map_layers") == 0
    e.set_map_stack(layers, res, pos)
    assert e.debug_get("map_layers") == 3 and e.debug_get("map_ptr") != 0
    for k in range(3):
        d, r, px, py = e.get_map_layer(k)
        assert same(d, layers[k]) and (r, px, py) == (res, pos[k, 0], pos[k, 1])
        xy = _sample_points(np.random.default_rng(30 + k), sx, sy, res, pos[k, 0], pos[k, 1], 2000)
        got_d, got_in = e.map_sample_layer(k, xy)
        want_d, want_in = oracle.map_distance(oracle.make_map(layers[k], res, pos[k, 0], pos[k, 1]), xy)
        assert 0 < got_in.sum() < len(got_in)  # positions inside and outside
        assert same(got_d, want_d) and np.array_equal(got_in, want_in)
    d0, *g0 = e.get_map()
    assert same(d0, layers[0]) and g0 == [res, pos[0, 0], pos[0, 1]]  # the single-map entries mean layer 0
    xy = _sample_points(np.random.default_rng(33), sx, sy, res, pos[0, 0], pos[0, 1], 500)
    assert all(same(a, b) for a, b in zip(e.map_sample(xy), e.map_sample_layer(0, xy)))
    L = binding.lib()
    for k in (-1, 3):  # a layer outside the stack is refused
        assert L.po_get_map_layer(e._h, k, ctypes.byref(abi.PoMap()), None) == abi.PO_ERR_INVALID
        with pytest.raises(binding.PoError):
            e.map_sample_layer(k, xy)
    # without per-layer positions every layer sits at the common centre
    e.set_map_stack(layers, res, None, pos_x=2.0, pos_y=-3.0)
    assert [e.get_map_layer(k)[1:] for k in range(3)] == [(res, 2.0, -3.0)] * 3 and same(e.get_map_layer(2)[0], layers[2])
    m = abi.PoMap(layers.ctypes.data_as(ctypes.c_void_p), 4097, 4, res, 0.0, 0.0)
    assert L.po_set_map_stack(e._h, 1, ctypes.byref(m), None) == abi.PO_ERR_UNSUPPORTED
    assert L.po_set_map_stack(e._h, 0, ctypes.byref(m), None) == abi.PO_ERR_INVALID
    e.close()


@pytest.mark.gpu
def test_stack_from_occupancy_either_entry():
    import torch

    sx, sy, res = 257, 129, 0.2
    rng = np.random.default_rng(41)
    occ = np.stack([edt_ref.random_occupancy(rng, sx, sy, kind) for kind in (0.003, 0.30, "none")])
    pos = np.array([[0.0, 0.0], [5.0, -1.0], [-3.0, 8.0]])
    want = [edt_ref.distance_map(o, res) for o in occ]
    a, b = binding.Engine(0), binding.Engine(0)
    raw = a.distance_map_batch(occ, res)
    a.set_map_stack_occupancy(occ, res, pos)
    dev_occ = torch.from_numpy(np.ascontiguousarray(occ.transpose(0, 2, 1))).cuda()  # [M, size_y, size_x]
    dev_pos = torch.from_numpy(pos).cuda()
    torch.cuda.synchronize()
    b.set_map_stack_occupancy_device(dev_occ, res, dev_pos)
    for e in (a, b):
        assert e.debug_get("map_layers") == 3
        for k in range(3):
            d, r, px, py = e.get_map_layer(k)
            assert same(d, want[k]) and same(d, raw[k]), k
            assert (r, px, py) == (res, pos[k, 0], pos[k, 1])
    with pytest.raises(ValueError):
        b.set_map_stack_occupancy_device(dev_occ.transpose(1, 2), res, dev_pos)  # not contiguous: refused, not misread
    a.close(); b.close()


# ---- the 18 planning instances over three maps ----
@pytest.fixture(scope="module")
def scenes():
    sc = [synth.make_planning_scenes(seed, 6, near=(2 if seed == 13 else 0), map_kw=dict(size_x=420, size_y=380, pos=(3.0 * i, -2.0 * i)))
          for i, seed in enumerate(SEEDS)]
    out = {k: np.stack([sc[b % M][k][b // M] for b in range(B)]) for k in ("way_x", "way_y", "start", "goal")}
    out["layers"] = np.stack([s["map"][0] for s in sc])
    out["res"] = sc[0]["map"][1]
    out["pos"] = np.array([[s["map"][2], s["map"][3]] for s in sc])
    assert out["layers"].shape == (M, 420, 380) and all(s["map"][1] == out["res"] for s in sc)
    return out


def _single(scenes, k, params=None):
    e = binding.Engine(0, params)
    e.set_map(scenes["layers"][k], scenes["res"], *scenes["pos"][k])
    return e


def _stacked(scenes, params=None):
    e = binding.Engine(0, params)
    e.set_map_stack(scenes["layers"], scenes["res"], scenes["pos"])
    e.set_map_assignment(LAYER_OF)
    return e


def _plan(e, sc):
    return e.plan_batch(sc["way_x"], sc["way_y"], sc["start"], sc["goal"], N=512)


@pytest.fixture(scope="module")
def plan_refs(scenes):
    """po_plan_batch of all 18 instances on three fresh single-map handles: refs[k] = (states, n_states, ok, stage, info) on layer k."""
    refs = []
    for k in range(M):
        e = _single(scenes, k)
        refs.append(_plan(e, scenes))
        e.close()
    return refs


@pytest.fixture(scope="module")
def traces(oracle, scenes):
    """oracle.path_optimizer_solve of every instance on its own layer: (ok, path, trace)."""
    p = oracle.default_params()
    maps = [oracle.make_map(scenes["layers"][k], scenes["res"], *scenes["pos"][k]) for k in range(M)]
    return [oracle.path_optimizer_solve(p, maps[b % M], scenes["way_x"][b], scenes["way_y"][b], scenes["start"][b], scenes["goal"][b]) for b in range(B)]


def _padded(rows, width=None):
    """Ragged per-instance lists -> [B, width] array + lengths."""
    n = np.array([len(r) for r in rows], dtype=np.int32)
    out = np.zeros((len(rows), width or int(n.max())))
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, n


def _from_trace(traces, key):
    """The trace entry `key` of every instance; an instance whose pipeline stopped before that stage borrows the entry of the next instance on the SAME layer that
    has one (the stage still runs on natural inputs that lie inside that instance's map)."""
    out = []
    for b in range(B):
        donors = [c for c in list(range(b, B, M)) + list(range(b % M, b, M)) if key in traces[c][2]]
        out.append(traces[donors[0]][2][key])
    return out


def _stage_inputs(oracle, scenes, traces, plan_refs):
    """The natural inputs of every map-reading stage, taken from the oracle pipeline's intermediates of each instance on its own layer."""
    inp = {}
    # TENSION smoothing: the lists segmentRawReference hands over
    raw = []
    for b in range(B):
        n, bx, by, bs = oracle.bspline(scenes["way_x"][b], scenes["way_y"][b])
        raw.append(oracle.segment_raw(bs, bx, by)[1])  # x, y, s, angle, k
    sm = {}
    for i, key in enumerate(("x", "y", "s", "angle", "k")):
        sm[key], sm["n_points"] = _padded([r[i] for r in raw])
    sm.update(lb=None, ub=None, l0=None)
    inp["smooth"] = sm
    # DP search: the smoothed spline, its length + 3, the start state
    t2 = _from_trace(traces, "tension2")
    ks, nk = _padded([t[2] for t in t2]); kx, _ = _padded([t[0] for t in t2]); ky, _ = _padded([t[1] for t in t2])
    inp["dp"] = (dict(knot_s=ks, knot_x=kx, knot_y=ky), np.array([t[2][-1] + 3 for t in t2]), np.ascontiguousarray(scenes["start"][:, :3]), nk)
    # corridor bounds: the re-sampled reference and the second spline
    ref, post = _from_trace(traces, "reference"), _from_trace(traces, "post")
    P = {}
    for i, key in enumerate(("ref_x", "ref_y", "ref_z", "ref_k", "ref_s")):
        P[key], npts = _padded([r[i] for r in ref])
    for i, key in enumerate(("knot_s", "knot_x", "knot_y")):
        P[key], nkn = _padded([q[i] for q in post])
    for b in range(B):  # padding knots stay increasing
        P["knot_s"][b, nkn[b]:] = P["knot_s"][b, nkn[b] - 1] + 1.0 + np.arange(P["knot_s"].shape[1] - nkn[b])
    inp["bounds"] = (P, npts, nkn)
    # collision check / densifying output: the QP states the device pipeline produced for each instance on its own layer
    states, n, ok, stage, info = pick(plan_refs)
    inp["post"] = (states, info, np.where(n > 0, n, 2).astype(np.int32))
    return inp


def _run_stages(e, inp):
    sp, length, start, nk = inp["dp"]
    P, npts, nkn = inp["bounds"]
    states, info, n = inp["post"]
    return {
        "bounds": e.bounds_batch(P, n_points=npts, n_knots=nkn),
        "dp_search": e.dp_search_batch(sp, length, start, 64, n_knots=nk),
        "postcheck": e.postcheck_batch(states, info, n_points=n),
        "densify": e.densify_batch(states, info, 400, n_points=n),
        "smooth": e.smooth_batch(abi.PO_SMOOTH_TENSION, inp["smooth"])[:4],
    }


@pytest.mark.gpu
def test_each_map_stage_reads_its_instances_layer(oracle, scenes, traces, plan_refs):
    inp = _stage_inputs(oracle, scenes, traces, plan_refs)
    refs = []
    for k in range(M):
        e = _single(scenes, k)
        refs.append(_run_stages(e, inp))
        e.close()
    e = _stacked(scenes)
    got = _run_stages(e, inp)
    e.close()
    for stage in got:
        want = pick([r[stage] for r in refs])
        eq = rows_equal(got[stage], want)
        assert eq.all(), (stage, np.flatnonzero(~eq))
        # not vacuous: some instance of layers 1 / 2 comes out differently on layer 0 alone
        differs = ~rows_equal(got[stage], refs[0][stage])
        assert differs[LAYER_OF != 0].any() and not differs[LAYER_OF == 0].any(), (stage, differs)
    # the stages did real work on these inputs: the instances the oracle pipeline plans on their own layer (all but DP ties, as in the end-to-end test) pass
    # the collision check of their own states, and the other stages give them a search result, a corridor and a solved QP
    n_ok = sum(bool(t[0]) for t in traces)
    assert n_ok >= 12 and got["postcheck"][1].sum() >= n_ok - 1
    assert (got["smooth"][3]["status"] == 1).sum() >= n_ok - 1 and (got["dp_search"][4] >= 4).sum() >= n_ok - 1 and (got["bounds"][1] >= 2).sum() >= n_ok - 1


def _agrees_with_oracle(b, out, trace, tol):
    """The agreement rule of test_device_pipeline_on_cluttered_scenes (tests/test_pipeline.py)."""
    states, n, ok, stage, info = out
    ook, opath, tr = trace
    same_ = bool(ok[b]) == bool(ook) and n[b] == len(opath)
    if same_ and ook:
        same_ = np.abs(states[b, :n[b]] - opath).max() < tol
    if same_ and not ook:  # the stage the device blames must be the one where the oracle pipeline stopped
        stopped = 7 if "qp" in tr else (6 if "reference" in tr else (5 if "init" in tr else (4 if "dp" in tr and tr["dp"][0] >= 0 else 3)))
        same_ = stage[b] == stopped or (stopped == 4 and stage[b] in (3, 4))
    return bool(same_)


@pytest.mark.gpu
def test_plan_batch_end_to_end_on_the_stack(scenes, traces, plan_refs):
    want = pick(plan_refs)
    e = _stacked(scenes)
    got = _plan(e, scenes)
    e.close()
    for name, g, w in zip(("states", "n_states", "ok", "stage", "info"), got, want):
        assert same(g, w), name
    differs = ~rows_equal(got, plan_refs[0])
    assert differs[LAYER_OF != 0].any() and not differs[LAYER_OF == 0].any()
    # against the oracle pipeline, instance by instance on its own layer: 1e-6 on the plain scenes, 1e-5 on the cluttered one (seed 13 = layer 2)
    agree = sum(_agrees_with_oracle(b, got, traces[b], 1e-5 if b % M == 2 else 1e-6) for b in range(B))
    assert agree >= B - 1, agree  # a DP tie / threshold may flip on the device (last-ulp trigonometry): 2 of 24 there, 1 of 18 here
    # the stack built from thresholded occupancy images against po_set_map_occupancy per layer
    occ = (scenes["layers"] > 0).astype(np.uint8)
    refs = []
    for k in range(M):
        s = binding.Engine(0)
        s.set_map_occupancy(occ[k], scenes["res"], *scenes["pos"][k])
        refs.append(_plan(s, scenes))
        s.close()
    e = binding.Engine(0)
    e.set_map_stack_occupancy(occ, scenes["res"], scenes["pos"])
    e.set_map_assignment(LAYER_OF)
    got2 = _plan(e, scenes)
    e.close()
    for name, g, w in zip(("states", "n_states", "ok", "stage", "info"), got2, pick(refs)):
        assert same(g, w), name
    assert (~rows_equal(got2, refs[0]))[LAYER_OF != 0].any()


@pytest.mark.gpu
def test_assignment_semantics(scenes, plan_refs):
    states, n, ok, stage, info = pick(plan_refs)
    npts = np.where(n > 0, n, 2).astype(np.int32)
    run = lambda eng: eng.postcheck_batch(states, info, n_points=npts)
    refs = []
    for k in range(M):
        s = _single(scenes, k)
        refs.append(run(s))
        s.close()
    assert not same(refs[0][0], refs[1][0]) and not same(refs[0][0], refs[2][0])  # the layer matters on these inputs
    want = pick(refs)
    L = binding.lib()
    e = binding.Engine(0)
    with pytest.raises(binding.PoError):
        e.set_map_assignment(LAYER_OF)  # no stack to assign into
    e.set_map_stack(scenes["layers"], scenes["res"], scenes["pos"])
    assert all(same(g, w) for g, w in zip(run(e), refs[0]))  # no assignment: every instance reads layer 0
    e.set_map_assignment(LAYER_OF)
    assert all(same(g, w) for g, w in zip(run(e), want))
    # a host table with an index outside [0, M) is refused and the previous table stays in force
    for bad in (-1, M):
        t = LAYER_OF.copy(); t[7] = bad
        assert L.po_set_map_assignment(e._h, B, t.ctypes.data_as(ctypes.c_void_p)) == abi.PO_ERR_INVALID
        assert all(same(g, w) for g, w in zip(run(e), want))
    # B > n
    e.set_map_assignment(LAYER_OF[:10])
    nv = np.zeros(B, dtype=np.int32); okv = np.zeros(B, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.po_postcheck_batch(e._h, B, 512, p(npts), p(np.ascontiguousarray(states)), p(np.ascontiguousarray(info)), p(nv), p(okv)) == abi.PO_ERR_INVALID
    with pytest.raises(binding.PoError):
        _plan(e, scenes)
    sub = e.postcheck_batch(states[:10], info[:10], n_points=npts[:10])  # B <= n is served
    assert all(same(g, w[:10]) for g, w in zip(sub, want))
    # a same-M re-install keeps the table (and reads the new layers): layers rotated, table unchanged
    e.set_map_assignment(LAYER_OF)
    rot = [2, 0, 1]
    e.set_map_stack(scenes["layers"][rot], scenes["res"], scenes["pos"][rot])
    want_rot = tuple(np.stack([refs[rot[b % M]][i][b] for b in range(B)]) for i in range(2))
    assert all(same(g, w) for g, w in zip(run(e), want_rot))
    # a clear: layer 0 of the stack in place
    e.set_map_assignment(None)
    assert all(same(g, w) for g, w in zip(run(e), refs[2]))
    # an install with another M clears the table
    e.set_map_assignment(LAYER_OF)
    e.set_map_stack(scenes["layers"][:2], scenes["res"], scenes["pos"][:2])
    assert e.debug_get("map_layers") == 2
    assert all(same(g, w) for g, w in zip(run(e), refs[0]))
    # po_set_map after a stack: like a fresh handle, whatever the handle ran before
    e.set_map_stack(scenes["layers"], scenes["res"], scenes["pos"])
    e.set_map_assignment(LAYER_OF)
    run(e)
    e.set_map(scenes["layers"][1], scenes["res"], *scenes["pos"][1])
    assert e.debug_get("map_layers") == 1
    assert all(same(g, w) for g, w in zip(run(e), refs[1]))
    assert all(same(g, w) for g, w in zip(_plan(e, scenes), plan_refs[1]))
    e.close()


@pytest.mark.gpu
def test_device_entries_are_ordered_by_the_stream(scenes, plan_refs):
    import torch

    occ = (scenes["layers"] > 0).astype(np.uint8)
    rot = [1, 2, 0]

    def host_way(images, pos):
        refs = []
        for k in range(len(images)):
            s = binding.Engine(0)
            s.set_map_occupancy(images[k], scenes["res"], *pos[k])
            refs.append(_plan(s, scenes))
            s.close()
        return pick(refs)

    want1, want2 = host_way(occ, scenes["pos"]), host_way(occ[rot], scenes["pos"][rot])
    assert not same(want1[0], want2[0])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    img1, img2 = dev(occ.transpose(0, 2, 1)), dev(occ[rot].transpose(0, 2, 1))
    pos1, pos2 = dev(scenes["pos"]), dev(scenes["pos"][rot])
    table = dev(LAYER_OF)
    t = {k: dev(scenes[k]) for k in ("way_x", "way_y", "start", "goal")}
    length = float(np.hypot(np.diff(scenes["way_x"], axis=1), np.diff(scenes["way_y"], axis=1)).sum(axis=1).max())

    def outputs():
        return dict(states=torch.zeros((B, 512, 5), dtype=torch.float64, device="cuda"), n_states=torch.zeros(B, dtype=torch.int32, device="cuda"),
                    ok=torch.zeros(B, dtype=torch.int32, device="cuda"), stage=torch.zeros(B, dtype=torch.int32, device="cuda"),
                    info=torch.zeros((B, abi.INFO_BYTES), dtype=torch.uint8, device="cuda"))

    o1, o2, o3 = outputs(), outputs(), outputs()
    torch.cuda.synchronize()  # the inputs are in place; from here on the stream alone orders the work
    e = binding.Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.set_map_stack_occupancy_device(img1, scenes["res"], pos1)
    e.set_map_assignment_device(table)
    e.plan_batch_device(t, o1, 512, length)   # no synchronisation in between
    p1 = e.debug_get("map_ptr")
    e.set_map_stack_occupancy_device(img2, scenes["res"], pos2)  # the refresh: same M and size, the table stays
    e.plan_batch_device(t, o2, 512, length)
    p2 = e.debug_get("map_ptr")
    torch.cuda.synchronize()
    assert p1 != 0 and p2 == p1  # rebuilt where it was

    def check(o, want):
        got = (o["states"].cpu().numpy(), o["n_states"].cpu().numpy(), o["ok"].cpu().numpy(), o["stage"].cpu().numpy(),
               o["info"].cpu().numpy().view(abi.INFO_DTYPE).reshape(B))
        for name, g, w in zip(("states", "n_states", "ok", "stage", "info"), got, want):
            assert same(g, w), name

    check(o1, want1)
    check(o2, want2)
    # a larger stack: four layers (the blocks grow behind a synchronisation), the table is dropped with the change of M and sent again
    occ4 = np.concatenate([occ, occ[:1]])
    pos4 = np.concatenate([scenes["pos"], scenes["pos"][:1]])
    img4, dpos4 = dev(occ4.transpose(0, 2, 1)), dev(pos4)
    table4 = dev(np.where(LAYER_OF == 0, 3, LAYER_OF).astype(np.int32))  # layer 3 is a copy of layer 0
    torch.cuda.synchronize()
    e.set_map_stack_occupancy_device(img4, scenes["res"], dpos4)
    assert e.debug_get("map_layers") == 4
    e.set_map_assignment_device(table4)
    e.plan_batch_device(t, o3, 512, length)
    torch.cuda.synchronize()
    check(o3, want1)
    e.set_stream(None)
    e.close()


@pytest.mark.gpu
def test_host_mirror_program():
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "map_stack_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "map_stack_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "map stack ok" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]
