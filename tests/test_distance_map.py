"""The obstacle-distance layer from an occupancy image (csrc/po_edt.hip; po_distance_map_batch*, po_set_map_occupancy*, po_get_map).

The result is a function of exact integers — d2 = min (i - p)^2 + (j - q)^2 over the occupied cells, dist = float32(sqrt(double(d2))) * float32(resolution) — so every
comparison here is BIT equality (uint32 views), on every cell of every image; nothing is a tolerance.  The CPU reference is tests/edt_ref.py (pure numpy, exact).

CPU: the reference reproduces the committed benchmark layer and agrees with scipy; the ABI mirror; argument checking without a device.
GPU: the fixture, a size / density matrix up to 4096 x 4096, the handle's map installed either way, the whole pipeline on the benchmark scene either way, the device
entry on a stream, determinism, four threads with a handle each (one process)."""
import ctypes
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import edt_ref
from path_optimizer_amd import abi, binding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "benchmark_scene.npz")

# (size_x, size_y): the boundary shapes (1 x 1, one line either way), sizes around the wave / strip width of the kernels and sizes that are no multiple of anything
SIZES = [(1, 1), (1, 300), (300, 1), (33, 517), (63, 65), (64, 64), (257, 129), (513, 511)]
KINDS = ["single", "corner", 0.003, 0.05, 0.30, "all", "none"]   # one cell ... 30 % occupied, all occupied, none (the library's rule)
NEW_ENTRIES = ["po_distance_map_batch", "po_distance_map_batch_device", "po_set_map_occupancy", "po_set_map_occupancy_device", "po_get_map"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def _occ_of(g):
    return (g["distance"] != 0).astype(np.uint8)


def _batch(seed, sx, sy):
    rng = np.random.default_rng(seed)
    return np.stack([edt_ref.random_occupancy(rng, sx, sy, k) for k in KINDS])


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_reference_reproduces_the_committed_layer(g):
    """Guards the yardstick: the numpy reference gives the fixture's layer (cv::distanceTransform(L2, MASK_PRECISE) * resolution) bit for bit."""
    d = g["distance"]
    got = edt_ref.distance_map(_occ_of(g), float(g["resolution"]))
    assert d.shape == (495, 497) and same_bits(got, d)
    assert same_bits(edt_ref.distance_map(_occ_of(g), float(g["resolution"]), route="shifted"), d)


def test_reference_routes_agree_with_each_other_and_with_scipy():
    from scipy import ndimage

    res = 0.2
    for n, (sx, sy) in enumerate(SIZES + [(200, 150)]):
        for occ in _batch(100 + n, sx, sy):
            a = edt_ref.d2(occ, route="broadcast")
            assert np.array_equal(a, edt_ref.d2(occ, route="shifted"))
            if (occ == 0).sum() <= 64:
                assert np.array_equal(a, edt_ref.d2_brute(occ))
            if (occ == 0).any():  # (scipy has no answer of its own for an image without a zero)
                sc = ndimage.distance_transform_edt(occ != 0).astype(np.float32) * np.float32(res)
                assert same_bits(edt_ref.to_metres(a, res), sc), (sx, sy)
            else:
                assert (a == sx * sx + sy * sy).all()
    corner = edt_ref.random_occupancy(np.random.default_rng(0), 64, 64, "corner")
    assert edt_ref.d2(corner)[63, 63] == 2 * 63 * 63 and edt_ref.d2(corner)[0, 0] == 0


def test_occupancy_struct_layout_matches_c():
    fields = ["cells", "size_x", "size_y", "resolution", "pos_x", "pos_y"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "po_hip.h"\nint main(){printf("%zu", sizeof(po_occupancy));'
           + "".join(f'printf(" %zu", offsetof(po_occupancy, {f}));' for f in fields) + 'printf(" %d\\n", PO_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got[0] == ctypes.sizeof(abi.PoOccupancy)
    assert got[1:7] == [getattr(abi.PoOccupancy, f).offset for f in fields]
    assert got[7] == abi.PO_ABI_VERSION == 7
    assert [n for n, _ in abi.PoOccupancy._fields_] == fields


def test_new_entries_are_exported_and_check_their_arguments_without_a_device():
    L = binding.lib()
    for name in NEW_ENTRIES:
        assert name in binding.EXPORTS
        getattr(L, name)
    cells = np.ones((4, 4), dtype=np.uint8)
    out = np.zeros((4, 4), dtype=np.float32)
    occ = abi.PoOccupancy(cells.ctypes.data_as(ctypes.c_void_p), 4, 4, 0.2, 0.0, 0.0)
    m = abi.PoMap()
    po, pf = ctypes.byref(occ), out.ctypes.data_as(ctypes.c_void_p)
    # a null handle is PO_ERR_INVALID on every entry, before any device call
    assert L.po_distance_map_batch(None, 1, po, pf) == abi.PO_ERR_INVALID
    assert L.po_distance_map_batch_device(None, 1, po, pf) == abi.PO_ERR_INVALID
    assert L.po_set_map_occupancy(None, po) == abi.PO_ERR_INVALID
    assert L.po_set_map_occupancy_device(None, po) == abi.PO_ERR_INVALID
    assert L.po_get_map(None, ctypes.byref(m), None) == abi.PO_ERR_INVALID


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
def test_argument_checks_with_a_handle(eng):
    L = binding.lib()
    cells = np.ones((4, 4), dtype=np.uint8)
    out = np.zeros((4, 4), dtype=np.float32)
    pf = out.ctypes.data_as(ctypes.c_void_p)
    mk = lambda **kw: abi.PoOccupancy(**{**dict(cells=cells.ctypes.data, size_x=4, size_y=4, resolution=0.2, pos_x=0.0, pos_y=0.0), **kw})
    bad = [mk(cells=None), mk(size_x=0), mk(size_y=-1), mk(resolution=0.0), mk(resolution=-1.0), mk(resolution=float("nan"))]
    for o in bad:
        for fn in (L.po_distance_map_batch, L.po_distance_map_batch_device):
            assert fn(eng._h, 1, ctypes.byref(o), pf) == abi.PO_ERR_INVALID
        for fn in (L.po_set_map_occupancy, L.po_set_map_occupancy_device):
            assert fn(eng._h, ctypes.byref(o)) == abi.PO_ERR_INVALID
    ok = mk()
    assert L.po_distance_map_batch(eng._h, 0, ctypes.byref(ok), pf) == abi.PO_ERR_INVALID
    assert L.po_distance_map_batch(eng._h, 1, None, pf) == abi.PO_ERR_INVALID
    assert L.po_distance_map_batch(eng._h, 1, ctypes.byref(ok), None) == abi.PO_ERR_INVALID
    assert L.po_set_map_occupancy(eng._h, None) == abi.PO_ERR_INVALID
    assert L.po_get_map(eng._h, None, None) == abi.PO_ERR_INVALID
    # beyond the cap: unsupported, never a wrong layer
    assert L.po_distance_map_batch(eng._h, 1, ctypes.byref(mk(size_x=4097)), pf) == abi.PO_ERR_UNSUPPORTED
    assert L.po_set_map_occupancy(eng._h, ctypes.byref(mk(size_y=1 << 20))) == abi.PO_ERR_UNSUPPORTED
    fresh = binding.Engine(0)
    assert L.po_get_map(fresh._h, ctypes.byref(abi.PoMap()), None) == abi.PO_ERR_INVALID  # no map set
    assert fresh.debug_get("map_ptr") == 0
    fresh.close()


@pytest.mark.gpu
def test_fixture_layer_bit_for_bit(eng, g):
    d = eng.distance_map_batch(_occ_of(g)[None], float(g["resolution"]))
    assert d.shape == (1, 495, 497) and d.dtype == np.float32
    diff = bits(d[0]) != bits(g["distance"])
    print("fixture: cells", diff.size, "different", int(diff.sum()))
    assert diff.size == 246015 and not diff.any()


@pytest.mark.gpu
@pytest.mark.parametrize("sx,sy", SIZES)
def test_size_and_density_matrix_bit_for_bit(eng, sx, sy):
    res = 0.2
    occ = _batch(7 * sx + sy, sx, sy)
    got = eng.distance_map_batch(occ, res)
    assert got.shape == occ.shape
    for m, kind in enumerate(KINDS):
        ref = edt_ref.distance_map(occ[m], res)
        diff = bits(got[m]) != bits(ref)
        print(f"{sx} x {sy} {kind}: occupied {int((occ[m] == 0).sum())} different cells {int(diff.sum())}")
        assert not diff.any(), (sx, sy, kind, int(diff.sum()))
        assert (bits(got[m][occ[m] == 0]) == 0).all()  # occupied cells: +0.0f
    none = got[KINDS.index("none")]
    assert (none == np.float32(np.sqrt(np.float64(sx * sx + sy * sy))) * np.float32(res)).all() and np.isfinite(none).all()


@pytest.mark.gpu
def test_2048_by_1500_bit_for_bit(eng):
    rng = np.random.default_rng(2048)
    occ = np.stack([edt_ref.random_occupancy(rng, 2048, 1500, 0.01), edt_ref.random_occupancy(rng, 2048, 1500, 0.30)])
    occ[0, 700:1400, 300:1200] = 255   # a free region some hundred cells across inside the 1 % image: long searches
    got = eng.distance_map_batch(occ, 0.05)
    for m in range(2):
        ref2 = edt_ref.d2(occ[m])
        diff = bits(got[m]) != bits(edt_ref.to_metres(ref2, 0.05))
        print(f"2048 x 1500 image {m}: largest d2 {int(ref2.max())} different cells {int(diff.sum())}")
        assert not diff.any()


@pytest.mark.gpu
def test_4096_by_4096_sparse_crosses_two_to_the_24(eng):
    """A handful of occupied cells near one corner, the corner cell among them: d2 reaches 2 * 3845^2 > 2^24 (then, with the far corner alone, 2 * 4095^2), where an int -> float32 conversion is no longer exact."""
    occ = np.full((4096, 4096), 1, dtype=np.uint8)
    for p, q in [(0, 0), (3, 40), (100, 17), (57, 300), (250, 250)]:
        occ[p, q] = 0
    ref2 = edt_ref.d2_brute(occ)
    assert ref2.max() > 1 << 24
    got = eng.distance_map_batch(occ[None], 0.1)[0]
    diff = bits(got) != bits(edt_ref.to_metres(ref2, 0.1))
    print("4096 x 4096: largest d2", int(ref2.max()), "cells above 2^24", int((ref2 > 1 << 24).sum()), "different cells", int(diff.sum()))
    assert not diff.any()
    # and the far corner alone: every cell's d2 is i^2 + j^2, up to 2 * 4095^2
    occ[:] = 1
    occ[4095, 4095] = 0
    got = eng.distance_map_batch(occ[None], 0.1)[0]
    assert same_bits(got, edt_ref.to_metres(edt_ref.d2_brute(occ), 0.1))


def _sample_points(rng, sx, sy, res, px, py, n):
    """World positions over 1.2 x the map's extent: inside and outside."""
    return np.stack([px + (rng.random(n) - 0.5) * 1.2 * sx * res, py + (rng.random(n) - 0.5) * 1.2 * sy * res], axis=1)


@pytest.mark.gpu
def test_map_from_occupancy_is_the_map_from_the_layer(g):
    res, px, py = 0.25, 3.5, -7.25
    occ = edt_ref.random_occupancy(np.random.default_rng(5), 203, 151, 0.02)
    ref = edt_ref.distance_map(occ, res)
    a, b = binding.Engine(0), binding.Engine(0)
    a.set_map_occupancy(occ, res, px, py)
    b.set_map(ref, res, px, py)
    da, *ga = a.get_map()
    db, *gb = b.get_map()
    assert ga == gb == [res, px, py] and da.shape == (203, 151)
    assert same_bits(da, db) and same_bits(da, ref)
    xy = _sample_points(np.random.default_rng(6), 203, 151, res, px, py, 10000)
    (sa, ia), (sb, ib) = a.map_sample(xy), b.map_sample(xy)
    assert 0 < ia.sum() < len(ia)  # positions inside and outside
    assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64)) and np.array_equal(ia, ib)
    c = binding.Engine(0)
    c.set_map(*a.get_map())  # round trip
    assert same_bits(c.get_map()[0], ref)
    for e in (a, b, c):
        e.close()


def _pipeline(eng, g, eps):
    """plan_batch, then bounds_batch -> solve_batch -> postcheck_batch, exactly as tests/test_benchmark_scene.py runs them."""
    states, n, ok, stage, info = eng.plan_batch(g["way_x"][None], g["way_y"][None], g["start"][None], g["goal"][None], N=512)
    tag = "e4" if eps == 1e-4 else "e3"
    path1 = states[0, :n[0]]
    P = dict(ref_x=path1[None, :, 0], ref_y=path1[None, :, 1], ref_z=path1[None, :, 2], ref_s=path1[None, :, 4],
             knot_s=g[f"knot_s_{tag}"][None], knot_x=g[f"knot_x_{tag}"][None], knot_y=g[f"knot_y_{tag}"][None])
    bd, nv = eng.bounds_batch(P)
    N2 = int(nv[0])
    keep = binding.keep_control_steps(0, path1[:N2, 4])
    b = synth.Batch(0, 1, N2, keep, *(np.ascontiguousarray(path1[None, :N2, c]) for c in (0, 1, 2, 3, 4)), np.ascontiguousarray(bd[:, :N2]),
                    np.array([[0.0, 0.0, g["start"][3]]]), np.array([g["goal"][2]]))
    st2, info2, _ = eng.solve_batch(b)
    nk, ok2 = eng.postcheck_batch(st2, info2)
    return dict(states=states, n=n, ok=ok, stage=stage, info=info, bounds=bd, nv=nv, st2=st2, info2=info2, nk=nk, ok2=ok2)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,eps", [("e3", 1e-3), ("e4", 1e-4)])
def test_benchmark_scene_end_to_end_either_way(g, tag, eps):
    res, px, py = float(g["resolution"]), float(g["pos"][0]), float(g["pos"][1])
    out = []
    for from_occupancy in (False, True):
        p = binding.default_params()
        p.eps_abs = p.eps_rel = eps
        e = binding.Engine(0, p)
        if from_occupancy:
            e.set_map_occupancy(_occ_of(g), res, px, py)
        else:
            e.set_map(g["distance"], res, px, py)
        out.append(_pipeline(e, g, eps))
        e.close()
    a, b = out
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k  # bitwise: states, n, ok, stage, info, bounds, the second solve, the collision check
    n = b["n"][0]
    ref1, ref2 = g[f"path1_{tag}"], g[f"path2_{tag}"]
    assert b["ok"][0] == 1 and b["stage"][0] == 0 and n == len(ref1)
    assert np.abs(b["states"][0, :n] - ref1).max() < 1e-6
    assert b["ok2"][0] == 1 and b["nk"][0] == len(ref2) and np.abs(b["st2"][0, :b["nk"][0]] - ref2).max() < 1e-6


class _DevPaths:
    """What postcheck_batch_device reads of a DeviceBatch: solved states in HBM."""

    def __init__(self, states):
        import torch

        self.B, self.N, self.n_points = states.shape[0], states.shape[1], None
        info = np.zeros(self.B, dtype=abi.INFO_DTYPE)
        info["status"] = 1
        self.info_np = info
        self.out_states = torch.from_numpy(np.ascontiguousarray(states)).cuda()
        self.out_info = torch.from_numpy(info.view(np.uint8).reshape(self.B, -1).copy()).cuda()


@pytest.mark.gpu
def test_device_entry_refreshes_the_map_in_place_on_the_stream(g):
    import torch

    res, px, py = float(g["resolution"]), float(g["pos"][0]), float(g["pos"][1])
    path = np.ascontiguousarray(g["path1_e4"])
    states = np.stack([path, path + np.array([0.0, 0.6, 0.0, 0.0, 0.0])])
    occ1 = _occ_of(g)
    # second image, same size: a block of occupied cells across the middle of the path (cell index = (pos + len / 2 - position) / resolution)
    occ2 = occ1.copy()
    mid = path[len(path) // 2]
    ci, cj = int((px + 0.5 * 495 * res - mid[0]) / res), int((py + 0.5 * 497 * res - mid[1]) / res)
    occ2[ci - 4:ci + 5, cj - 4:cj + 5] = 0
    # third image: larger
    occ3 = np.full((640, 700), 1, dtype=np.uint8)
    occ3[70:70 + 495, 100:100 + 497] = occ2
    images = [occ1, occ2, occ3]

    def host_way(occ):
        e = binding.Engine(0)
        e.set_map_occupancy(occ, res, px, py)
        r = e.postcheck_batch(states, _DevPaths(states).info_np)
        e.close()
        return r

    want = [host_way(o) for o in images]
    assert not np.array_equal(want[0][0], want[1][0])  # the second map changes the answer
    # [size_x, size_y] views with x contiguous: the transposed view of a contiguous [size_y, size_x] image
    dev_imgs = [torch.from_numpy(np.ascontiguousarray(o.T)).cuda().t() for o in images]
    dp = _DevPaths(states)
    nv = [torch.zeros(2, dtype=torch.int32, device="cuda") for _ in images]
    ok = [torch.zeros(2, dtype=torch.int32, device="cuda") for _ in images]
    torch.cuda.synchronize()  # the inputs are in place; from here on the handle's stream alone orders the work
    e = binding.Engine(0)
    ptrs = []
    for k, img in enumerate(dev_imgs):
        e.set_map_occupancy_device(img, res, px, py)
        e.postcheck_batch_device(dp, nv[k], ok[k])   # no synchronisation in between
        ptrs.append(e.debug_get("map_ptr"))          # (reads a host field: does not synchronise)
    torch.cuda.synchronize()
    for k in range(3):
        assert np.array_equal(nv[k].cpu().numpy(), want[k][0]) and np.array_equal(ok[k].cpu().numpy(), want[k][1]), k
    assert ptrs[0] != 0 and ptrs[1] == ptrs[0]  # same size: the layer was rebuilt where it was
    assert same_bits(e.get_map()[0], edt_ref.distance_map(occ3, res))
    with pytest.raises(ValueError):
        e.set_map_occupancy_device(torch.from_numpy(occ1).cuda(), res, px, py)  # y contiguous: refused, not misread
    e.close()


@pytest.mark.gpu
def test_same_batch_twice_gives_identical_bits(eng):
    occ = _batch(99, 257, 129)
    a = eng.distance_map_batch(occ, 0.2)
    b = eng.distance_map_batch(occ, 0.2)
    other = binding.Engine(0)
    c = other.distance_map_batch(occ, 0.2)
    other.close()
    assert same_bits(a, b) and same_bits(a, c)


@pytest.mark.gpu
def test_four_threads_each_with_a_handle_get_their_own_map():
    res, px, py, sx, sy = 0.2, 1.0, -2.0, 200, 150
    occs = [edt_ref.random_occupancy(np.random.default_rng(40 + t), sx, sy, (0.002, 0.01, 0.05, 0.2)[t]) for t in range(4)]
    xy = _sample_points(np.random.default_rng(44), sx, sy, res, px, py, 2000)
    want = []
    for o in occs:  # serial: a fresh engine fed the reference layer
        e = binding.Engine(0)
        e.set_map(edt_ref.distance_map(o, res), res, px, py)
        want.append(e.map_sample(xy))
        e.close()
    assert not np.array_equal(want[0][0], want[1][0])
    bad, engines = [], [binding.Engine(0) for _ in range(4)]
    gate = threading.Barrier(4)

    def work(t):
        try:
            gate.wait(timeout=60)
            for rep in range(5):
                engines[t].set_map_occupancy(occs[t], res, px, py)
                d, ins = engines[t].map_sample(xy)
                if not (np.array_equal(d.view(np.uint64), want[t][0].view(np.uint64)) and np.array_equal(ins, want[t][1])):
                    bad.append((t, rep))
        except Exception as ex:  # noqa: BLE001
            bad.append((t, repr(ex)))

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not any(x.is_alive() for x in th) and not bad, bad
    for e in engines:
        e.close()
