"""The map stack from per-layer obstacle lists, rasterised on the device (csrc/po_raster.hip; po_rasterize_batch*, po_set_map_stack_obstacles*).

The images are a function of IEEE double operations that are each rounded once (include/po_hip.h states them), so every comparison here is BIT equality — byte views of
every cell of every image, uint32 views of every element of every layer; nothing is a tolerance.  The CPU reference is tests/raster_ref.py (numpy, one ufunc per
operation, no culling); the layers behind the images are checked against the occupancy entries, which test_distance_map.py / test_map_stack.py pin.

CPU: the reference against a scalar loop over the definition, exact lattice counts, the ABI mirror, argument checks without a device, the host mirror's test source.
GPU: a size x list x base matrix, ties on every tile boundary, both entries and stream order, bad device lists (clamped, never out of bounds), host validation, the
stack against the occupancy route, po_plan_batch end to end, the handle contract."""
import ctypes
import math
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import edt_ref
import raster_ref
from path_optimizer_amd import abi, binding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["po_rasterize_batch", "po_rasterize_batch_device", "po_set_map_stack_obstacles", "po_set_map_stack_obstacles_device"]
# (size_x, size_y): one cell, one line either way, sizes around the tile (64 x 16) and the 4-cell store, sizes that are no multiple of anything, more than one tile
SIZES = [(1, 1), (1, 300), (300, 1), (33, 517), (63, 65), (64, 64), (257, 129), (513, 511)]
M5 = 5
POS5 = np.array([[0.0, 0.0], [1.5, -2.0], [-7.25, 3.0], [40.0, 40.5], [0.1, 0.3]])


def same(a, b):
    """Bitwise equality of two arrays (any dtype)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lists_struct(obs, first, sx, sy, res, base=None, base_count=0, pos=(0.0, 0.0)):
    """po_obstacle_lists over host arrays, exactly as given (nothing derived, nothing checked)."""
    return abi.PoObstacleLists(p(obs) if obs is not None else None, p(first) if first is not None else None, 0 if obs is None else len(obs),
                               None if base is None else p(base), base_count, sx, sy, res, pos[0], pos[1])


def _extent(sx, sy, res, pos):
    return pos[0] - 0.5 * sx * res, pos[0] + 0.5 * sx * res, pos[1] - 0.5 * sy * res, pos[1] + 0.5 * sy * res


def _random_disc(rng, sx, sy, res, pos, rmax):
    x0, x1, y0, y1 = _extent(sx, sy, res, pos)
    return binding.obstacle_disc(rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(0.3 * res, rmax))


def _random_box(rng, sx, sy, res, pos, rmax):
    x0, x1, y0, y1 = _extent(sx, sy, res, pos)
    return binding.obstacle_box(rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(0.3 * res, rmax), rng.uniform(0.3 * res, 0.6 * rmax), rng.uniform(-math.pi, math.pi))


def _random_polygon(rng, sx, sy, res, pos, rmax):
    """A convex polygon with 3 .. 8 vertices on an ellipse, either orientation."""
    x0, x1, y0, y1 = _extent(sx, sy, res, pos)
    n = int(rng.integers(3, 9))
    ang = np.sort(rng.uniform(0, 2 * math.pi, n))
    if rng.uniform() < 0.5:
        ang = ang[::-1]
    cx, cy, a, b = rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(0.5 * res, rmax), rng.uniform(0.5 * res, rmax)
    return binding.obstacle_polygon(np.stack([cx + a * np.cos(ang), cy + b * np.sin(ang)], axis=1))


def five_lists(seed, sx, sy, res, pos_xy):
    """The five lists of the size matrix: none; one disc inside; discs straddling each border and one wholly outside; 40 random discs + 20 random boxes; 200
    obstacles (more than any LDS round of the kernel)."""
    rng = np.random.default_rng(seed)
    ext = max(sx, sy) * res
    rmax = max(0.08 * ext, 2.0 * res)
    lay = [[] for _ in range(M5)]
    lay[1] = [binding.obstacle_disc(pos_xy[1][0] + 0.11 * sx * res, pos_xy[1][1] - 0.07 * sy * res, 0.2 * min(sx, sy) * res + 0.4 * res)]
    x0, x1, y0, y1 = _extent(sx, sy, res, pos_xy[2])
    r = 0.15 * min(sx, sy) * res + 0.7 * res
    lay[2] = [binding.obstacle_disc(x0, pos_xy[2][1], r), binding.obstacle_disc(x1, pos_xy[2][1] + 0.3 * res, r), binding.obstacle_disc(pos_xy[2][0], y0, r),
              binding.obstacle_disc(pos_xy[2][0] - 0.4 * res, y1, r), binding.obstacle_disc(x1 + 0.3 * r, y1 + 0.2 * r, r),  # a corner
              binding.obstacle_disc(x1 + 3.0 * r + ext, pos_xy[2][1], r)]  # wholly outside
    lay[3] = [_random_disc(rng, sx, sy, res, pos_xy[3], rmax) for _ in range(40)] + [_random_box(rng, sx, sy, res, pos_xy[3], rmax) for _ in range(20)]
    kinds = (_random_disc, _random_box, _random_polygon)
    lay[4] = [kinds[int(rng.integers(0, 3))](rng, sx, sy, res, pos_xy[4], 0.5 * rmax) for _ in range(200)]
    return lay


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def _scalar_cell(o, px, py):
    """The definition for one cell centre and one obstacle, in plain Python floats (IEEE double, one rounding per operation)."""
    v = [float(x) for x in o["v"]]
    if int(o["kind"]) == abi.PO_OBS_DISC:
        if any(math.isnan(x) for x in v[:3]):
            return False
        dx, dy = px - v[0], py - v[1]
        return dx * dx + dy * dy <= v[2] * v[2]
    if int(o["kind"]) == abi.PO_OBS_POLY:
        n = min(max(int(o["n_verts"]), 0), abi.PO_OBS_MAX_VERTS)
        if n < 3 or any(math.isnan(x) for x in v[:2 * n]):
            return False
        xs, ys = v[0:2 * n:2], v[1:2 * n:2]
        if not (min(xs) <= px <= max(xs) and min(ys) <= py <= max(ys)):
            return False
        cr = []
        for e in range(n):
            ax, ay, bx, by = xs[e], ys[e], xs[(e + 1) % n], ys[(e + 1) % n]
            t1 = (bx - ax) * (py - ay)
            t2 = (by - ay) * (px - ax)
            cr.append(t1 - t2)
        return all(c >= 0 for c in cr) or all(c <= 0 for c in cr)
    return False


def test_reference_agrees_with_a_scalar_loop_over_the_definition():
    sx, sy, res, pos = 33, 17, 0.2, (1.3, -0.7)
    rng = np.random.default_rng(5)
    obs_list = ([_random_disc(rng, sx, sy, res, pos, 1.2) for _ in range(6)] + [_random_box(rng, sx, sy, res, pos, 1.2) for _ in range(4)]
                + [_random_polygon(rng, sx, sy, res, pos, 1.5) for _ in range(6)])
    obs, first = binding.pack_obstacles([obs_list[:5], [], obs_list[5:]])
    base = (rng.random((sx, sy)) > 0.05).astype(np.uint8)
    got = raster_ref.rasterize(obs, first, sx, sy, res, pos=pos, base=base)
    want = np.empty((3, sx, sy), dtype=np.uint8)
    half_x, half_y = 0.5 * (sx * res) - 0.5 * res, 0.5 * (sy * res) - 0.5 * res
    for k in range(3):
        for i in range(sx):
            for j in range(sy):
                px = (pos[0] + half_x) + res * float(-i)
                py = (pos[1] + half_y) + res * float(-j)
                hit = base[i, j] == 0 or any(_scalar_cell(o, px, py) for o in obs[first[k]:first[k + 1]])
                want[k, i, j] = 0 if hit else 255
    assert same(got, want)
    assert 0 < (got[0] == 0).sum() < sx * sy and (got[1] == 0).sum() == (base == 0).sum() and not same(got[0], got[2])


LATTICE = dict(sx=64, sy=64, res=0.25, pos=(0.0, 0.0))  # every cell centre is exactly representable: 7.875 - 0.25 i


def _centre(i, j, size=64, res=0.25):
    return 0.5 * size * res - 0.5 * res - res * i, 0.5 * size * res - 0.5 * res - res * j


def _diamond(cx, cy, reverse=False):
    v = [(cx + 1.0, cy), (cx, cy + 1.0), (cx - 1.0, cy), (cx, cy - 1.0)]
    return binding.obstacle_polygon(v[::-1] if reverse else v)


def _count(o):
    obs, first = binding.pack_obstacles([[o]])
    img = raster_ref.rasterize(obs, first, LATTICE["sx"], LATTICE["sy"], LATTICE["res"], pos=LATTICE["pos"])
    return img[0] == 0


def test_reference_exact_lattice_facts():
    assert np.array_equal(raster_ref.cell_centres(64, 0.25, 0.0), 7.875 - 0.25 * np.arange(64))
    cx, cy = _centre(24, 32)
    # radius 1.25 = 5 cells: the lattice points with a^2 + b^2 <= 25, the 12 boundary points (+-5, 0), (0, +-5), (+-3, +-4), (+-4, +-3) included
    disc = _count(binding.obstacle_disc(cx, cy, 1.25))
    assert disc.sum() == 81
    for a, b in [(5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (3, -4), (-3, 4), (-3, -4), (4, 3), (4, -3), (-4, 3), (-4, -3)]:
        assert disc[24 + a, 32 + b]
    assert not disc[24 + 4, 32 + 4] and not disc[24 + 6, 32]
    point = _count(binding.obstacle_disc(cx, cy, 0.0))
    assert point.sum() == 1 and point[24, 32]
    # the diamond |a| + |b| <= 4 cells: 41 lattice points, whichever way round the vertices run
    for rev in (False, True):
        d = _count(_diamond(cx, cy, rev))
        assert d.sum() == 41 and d[24 + 4, 32] and d[24 + 2, 32 - 2] and not d[24 + 3, 32 + 2]
    # an axis-aligned box with corners on cell centres, 4 x 2 cells apart: 5 x 3 centres, edges and corners included
    (x0, y0), (x1, y1) = _centre(10, 20), _centre(14, 22)
    box = _count(binding.obstacle_polygon([(x0, y0), (x1, y0), (x1, y1), (x0, y1)]))
    assert box.sum() == 15 and box[10:15, 20:23].all()
    # three collinear vertices: every cross product vanishes on the whole LINE; the bounding box keeps the segment
    seg = _count(binding.obstacle_polygon([_centre(20, 20), _centre(24, 24), _centre(28, 28)]))
    assert seg.sum() == 9 and all(seg[20 + t, 20 + t] for t in range(9))


def test_struct_layouts_and_prototypes_match_the_header():
    fo, fl = ["kind", "n_verts", "v"], ["obs", "first", "n_obs", "base", "base_count", "size_x", "size_y", "resolution", "pos_x", "pos_y"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "po_hip.h"\n'
           'int (*a)(po_handle, int, const po_obstacle_lists *, const double *, unsigned char *) = po_rasterize_batch;\n'
           'int (*b)(po_handle, int, const po_obstacle_lists *, const double *, unsigned char *) = po_rasterize_batch_device;\n'
           'int (*c)(po_handle, int, const po_obstacle_lists *, const double *) = po_set_map_stack_obstacles;\n'
           'int (*d)(po_handle, int, const po_obstacle_lists *, const double *) = po_set_map_stack_obstacles_device;\n'
           'int main(){printf("%d %d %d %d %zu %zu", PO_ABI_VERSION, PO_OBS_DISC, PO_OBS_POLY, PO_OBS_MAX_VERTS, sizeof(po_obstacle), sizeof(po_obstacle_lists));'
           + "".join(f'printf(" %zu", offsetof(po_obstacle, {f}));' for f in fo) + "".join(f'printf(" %zu", offsetof(po_obstacle_lists, {f}));' for f in fl)
           + 'printf("\\n");return (a && b && c && d) ? 0 : 1;}\n')
    lib_dir = os.path.join(ROOT, "path_optimizer_amd")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t"),
                               "-L", lib_dir, "-l:libpo_hip.so", "-Wl,-rpath," + lib_dir])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got[:4] == [abi.PO_ABI_VERSION, abi.PO_OBS_DISC, abi.PO_OBS_POLY, abi.PO_OBS_MAX_VERTS] and abi.PO_ABI_VERSION == 7
    assert got[4] == 136 == ctypes.sizeof(abi.PoObstacle) == binding.OBSTACLE_DTYPE.itemsize
    assert got[5] == ctypes.sizeof(abi.PoObstacleLists)
    assert got[6:9] == [getattr(abi.PoObstacle, f).offset for f in fo] == [binding.OBSTACLE_DTYPE.fields[f][1] for f in fo]
    assert got[9:] == [getattr(abi.PoObstacleLists, f).offset for f in fl]
    assert [n for n, _ in abi.PoObstacleLists._fields_] == fl


def test_new_entries_are_exported_and_check_their_arguments_without_a_device():
    L = binding.lib()
    for name in NEW_ENTRIES:
        assert name in binding.EXPORTS
        getattr(L, name)
    obs, first = binding.pack_obstacles([[binding.obstacle_disc(0.0, 0.0, 1.0)]])
    ls = lists_struct(obs, first, 4, 4, 0.2)
    out = np.zeros((1, 4, 4), dtype=np.uint8)
    # a null handle is PO_ERR_INVALID on every entry, before any device call; so is a null struct (the handle is not looked at before the struct)
    fake = ctypes.c_void_p(8)  # (never dereferenced: the struct is looked at first)
    for h, s in ((None, ctypes.byref(ls)), (fake, None)):
        assert L.po_rasterize_batch(h, 1, s, None, p(out)) == abi.PO_ERR_INVALID
        assert L.po_rasterize_batch_device(h, 1, s, None, p(out)) == abi.PO_ERR_INVALID
        assert L.po_set_map_stack_obstacles(h, 1, s, None) == abi.PO_ERR_INVALID
        assert L.po_set_map_stack_obstacles_device(h, 1, s, None) == abi.PO_ERR_INVALID
    # the helpers: a box is a 4-vertex polygon whose corners are computed on the host
    b = binding.obstacle_box(1.0, 2.0, 2.0, 0.5, 0.0)
    assert int(b["kind"]) == abi.PO_OBS_POLY and int(b["n_verts"]) == 4
    assert np.array_equal(b["v"][:8], [3.0, 2.5, -1.0, 2.5, -1.0, 1.5, 3.0, 1.5]) and not b["v"][8:].any()
    d = binding.obstacle_disc(1.0, 2.0, 3.0)
    assert int(d["kind"]) == abi.PO_OBS_DISC and np.array_equal(d["v"][:3], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        binding.obstacle_polygon([(0, 0), (1, 1)])
    o2, f2 = binding.pack_obstacles([[d, b], [], [b]])
    assert f2.tolist() == [0, 2, 2, 3] and o2.dtype == binding.OBSTACLE_DTYPE and same(o2[2], b)


def test_host_mirror_test_source_compiles_and_links():
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "host_test"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(host, "host_test"))
    src = open(os.path.join(host, "test", "host_test.cpp")).read()
    assert "MapStack::fromObstacles" in src and "Obstacle::box" in src  # the lines that build and run the mirror are part of what was compiled


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _bases(rng, sx, sy):
    """Shared base (5 % occupied) and one base per layer."""
    return (rng.random((sx, sy)) >= 0.05).astype(np.uint8) * 255, (rng.random((M5, sx, sy)) >= 0.05).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rasterize_batch_matches_the_reference(size):
    sx, sy = size
    res = 0.2
    lay = five_lists(100 + sx, sx, sy, res, POS5)
    obs, first = binding.pack_obstacles(lay)
    assert len(obs) == 267
    cov = raster_ref.covered(obs, first, sx, sy, res, POS5)  # once; the three base modes share it
    shared, per_layer = _bases(np.random.default_rng(7 + sy), sx, sy)
    e = binding.Engine(0)
    for name, base in (("none", None), ("shared", shared), ("per layer", per_layer)):
        got = e.rasterize_batch(lay, sx, sy, res, POS5, base=base)
        want = raster_ref.to_cells(cov, base)
        assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 255}
        bad = np.argwhere(got != want)
        assert same(got, want), (name, len(bad), bad[:5])
    e.close()
    if sx * sy > 4000:  # the lists did something at this size: every non-empty layer has occupied and free cells
        occ = cov.reshape(M5, -1).sum(axis=1)
        assert occ[0] == 0 and (occ[1:] > 0).all() and (occ < sx * sy).all()


def _sweep(make, along_j):
    """80 layers: the obstacle `make(cx, cy)` centred on cell (24 + k, 40), or (40, 24 + k)."""
    return [[make(*(_centre(40, 24 + k, 128) if along_j else _centre(24 + k, 40, 128)))] for k in range(80)]


@pytest.mark.gpu
def test_ties_on_every_tile_boundary():
    """Cells EXACTLY on the boundary of a disc / on the edges of a diamond, swept over every residue modulo the tile (64 x 16) and the 4-cell store in both
    directions: a cull that is not conservative, or an off-by-one at a tile edge, loses or gains a tie cell here."""
    e = binding.Engine(0)
    for make, count in ((lambda x, y: binding.obstacle_disc(x, y, 1.25), 81), (_diamond, 41)):
        for along_j in (False, True):
            lay = _sweep(make, along_j)
            obs, first = binding.pack_obstacles(lay)
            got = e.rasterize_batch(lay, 128, 128, 0.25)
            want = raster_ref.rasterize(obs, first, 128, 128, 0.25)
            assert same(got, want), (count, along_j, np.argwhere(got != want)[:5])
            assert ((got == 0).reshape(80, -1).sum(axis=1) == count).all()
            k = 37  # and the tie cells themselves
            ci, cj = (40, 24 + k) if along_j else (24 + k, 40)
            ties = [(5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (-4, 3)] if count == 81 else [(4, 0), (-4, 0), (0, 4), (0, -4), (1, 3), (-2, -2)]
            assert all(got[k, ci + a, cj + b] == 0 for a, b in ties)
    e.close()


def _to_device(obs, first, base=None, pos=None):
    import torch

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(-1, 136).copy()).cuda()
    return d_obs, t(first), (None if base is None else t(np.ascontiguousarray(base.transpose(0, 2, 1)))), t(pos)


@pytest.mark.gpu
def test_both_entries_give_the_same_bytes_and_the_device_entry_is_ordered_by_the_stream():
    import torch

    sx, sy, res = 257, 129, 0.2
    lay = five_lists(3, sx, sy, res, POS5)
    obs, first = binding.pack_obstacles(lay)
    _, per_layer = _bases(np.random.default_rng(8), sx, sy)
    e = binding.Engine(0)
    host = e.rasterize_batch(lay, sx, sy, res, POS5, base=per_layer)
    assert same(host, raster_ref.rasterize(obs, first, sx, sy, res, POS5, base=per_layer))
    d_obs, d_first, d_base, d_pos = _to_device(obs, first, per_layer, POS5)
    out = torch.full((M5, sy, sx), 7, dtype=torch.uint8, device="cuda")
    out2 = torch.zeros((M5, sy, sx), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the inputs are in place; from here on the stream alone orders the work
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # torch's current stream: a stream of its own (the default stream's handle is NULL = "the handle's own stream")
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        e.rasterize_batch_device(d_obs, d_first, out, res, d_pos, base=d_base)
        flipped = 255 - out  # a consumer on the same stream, no synchronisation in between
        got = out.cpu().numpy().transpose(0, 2, 1)
        assert same(got, host)
        assert same(255 - flipped.cpu().numpy().transpose(0, 2, 1), host)
        # the shared base through the device entry, pos_xy = None
        e.rasterize_batch_device(d_obs, d_first, out2, res, None, pos_x=1.0, pos_y=-0.5, base=d_base[2:3])
        got2 = out2.cpu().numpy().transpose(0, 2, 1)
    assert same(got2, e.rasterize_batch(lay, sx, sy, res, None, 1.0, -0.5, base=per_layer[2]))
    with pytest.raises(ValueError):
        e.rasterize_batch_device(d_obs, d_first, out.transpose(1, 2), res, d_pos)  # not contiguous: refused, not misread
    e.set_stream(None)
    e.close()


@pytest.mark.gpu
def test_bad_device_lists_are_clamped_and_never_read_outside_obs():
    """What a device entry cannot validate: first[] past n_obs or descending, n_verts far outside 3 .. 8, an unknown kind, NaN coordinates.  Every value here is made
    harmless by the clamps the header documents (first[] into [0, n_obs], n_verts into [0, 8]: v has 16 slots), so the call returns and the result is the
    documented one — the reference applies the same rule."""
    import torch

    sx, sy, res = 100, 70, 0.25
    octagon = binding.obstacle_polygon([(3 * math.cos(a), 3 * math.sin(a)) for a in np.arange(8) * math.pi / 4])
    octagon["n_verts"] = 50  # read as 8: the whole v array, which is there
    tri = binding.obstacle_polygon([(-8.0, -6.0), (-4.0, -6.0), (-6.0, -2.0)])
    neg = tri.copy(); neg["n_verts"] = -5        # read as 0: covers nothing
    two = tri.copy(); two["n_verts"] = 2         # fewer than 3 vertices: covers nothing
    unknown = binding.obstacle_disc(5.0, 5.0, 2.0); unknown["kind"] = 7
    nan_disc = binding.obstacle_disc(float("nan"), 0.0, 50.0)
    nan_r = binding.obstacle_disc(0.0, 0.0, float("nan"))
    nan_poly = tri.copy(); nan_poly["v"][3] = float("nan")
    inf_disc = binding.obstacle_disc(float("inf"), 0.0, 1.0)
    good = binding.obstacle_disc(6.0, -4.0, 1.5)
    obs, _ = binding.pack_obstacles([[octagon, tri, neg, two, unknown, nan_disc, nan_r, nan_poly, inf_disc, good]])
    n = len(obs)
    # layer 0: everything; 1: first[2] far past n_obs (read as n_obs: empty); 2: descending (empty); 3: a negative end (read as 0: empty); 4: a negative start
    # (read as 0): everything again
    first = np.array([0, n, 1000000, 4, -7, n], dtype=np.int32)
    want = raster_ref.rasterize(obs, first, sx, sy, res)
    single = lambda o: raster_ref.rasterize(*binding.pack_obstacles([[o]]), sx, sy, res)[0]
    for o in (neg, two, unknown, nan_disc, nan_r, nan_poly, inf_disc):
        assert (single(o) == 255).all()  # the documented result: covers nothing
    oct8 = octagon.copy(); oct8["n_verts"] = 8
    assert same(single(octagon), single(oct8)) and (single(oct8) == 0).sum() > 300
    assert all((want[k] == 255).all() for k in (1, 2, 3)) and same(want[0], want[4]) and (want[0] == 0).sum() > 400
    d_obs, d_first, _, _ = _to_device(obs, first)
    out = torch.full((5, sy, sx), 9, dtype=torch.uint8, device="cuda")
    e = binding.Engine(0)
    e.rasterize_batch_device(d_obs, d_first, out, res)
    torch.cuda.synchronize()
    got = out.cpu().numpy().transpose(0, 2, 1)
    assert same(got, want), np.argwhere(got != want)[:5]
    e.close()


@pytest.mark.gpu
def test_host_entries_validate_before_they_touch_the_handle():
    L = binding.lib()
    sx, sy, res = 40, 30, 0.25
    e = binding.Engine(0)
    prev = [[binding.obstacle_disc(1.0, 1.0, 1.0)], [binding.obstacle_box(-2.0, 0.0, 1.0, 0.5, 0.3)]]
    e.set_map_stack_obstacles(prev, sx, sy, res)
    before = [e.get_map_layer(k) for k in range(2)]
    disc, box = binding.obstacle_disc(0.0, 0.0, 1.0), binding.obstacle_box(0.0, 0.0, 1.0, 0.5, 0.2)

    def edit(o, **kw):
        o = o.copy()
        for key, val in kw.items():
            if key == "v":
                o["v"][val[0]] = val[1]
            else:
                o[key] = val
        return o

    good_first = np.array([0, 1, 2], dtype=np.int32)
    base = np.full((3, sy, sx), 255, dtype=np.uint8)
    cases = {}
    for name, f in (("first not monotone", [0, 2, 1]), ("first[M] > n_obs", [0, 1, 3]), ("first[0] != 0", [1, 1, 2]), ("first negative", [0, -1, 2])):
        cases[name] = dict(obs=[disc, box], first=np.array(f, dtype=np.int32))
    for name, o in (("unknown kind", edit(disc, kind=2)), ("negative kind", edit(disc, kind=-1)), ("n_verts 2", edit(box, n_verts=2)), ("n_verts 9", edit(box, n_verts=9)),
                    ("negative radius", edit(disc, v=(2, -0.5))), ("infinite radius", edit(disc, v=(2, float("inf")))), ("nan radius", edit(disc, v=(2, float("nan")))),
                    ("nan centre", edit(disc, v=(0, float("nan")))), ("infinite centre", edit(disc, v=(1, float("-inf")))), ("nan vertex", edit(box, v=(5, float("nan")))),
                    ("infinite vertex", edit(box, v=(0, float("inf"))))):
        cases[name] = dict(obs=[disc, o], first=good_first)
    cases["base_count 3 with M 2"] = dict(obs=[disc, box], first=good_first, base=base, base_count=3)
    cases["base_count -1"] = dict(obs=[disc, box], first=good_first, base=base, base_count=-1)
    cases["base NULL with base_count 1"] = dict(obs=[disc, box], first=good_first, base=None, base_count=1)
    out = np.full((2, sy, sx), 3, dtype=np.uint8)
    for name, c in cases.items():
        obs = binding.pack_obstacles([c["obs"]])[0]
        ls = lists_struct(obs, c["first"], sx, sy, res, c.get("base"), c.get("base_count", 0))
        assert L.po_set_map_stack_obstacles(e._h, 2, ctypes.byref(ls), None) == abi.PO_ERR_INVALID, name
        assert L.po_rasterize_batch(e._h, 2, ctypes.byref(ls), None, p(out)) == abi.PO_ERR_INVALID, name
    assert (out == 3).all()  # nothing was written
    # sizes and M beyond the transform's limits
    obs = binding.pack_obstacles([[disc, box]])[0]
    assert L.po_set_map_stack_obstacles(e._h, 2, ctypes.byref(lists_struct(obs, good_first, 4097, 4, res)), None) == abi.PO_ERR_UNSUPPORTED
    many = np.zeros(65537, dtype=np.int32)
    assert L.po_set_map_stack_obstacles(e._h, 65536, ctypes.byref(lists_struct(obs, many, 4, 4, res)), None) == abi.PO_ERR_UNSUPPORTED
    assert L.po_set_map_stack_obstacles(e._h, 0, ctypes.byref(lists_struct(obs, good_first, sx, sy, res)), None) == abi.PO_ERR_INVALID
    assert L.po_set_map_stack_obstacles(e._h, 2, ctypes.byref(lists_struct(obs, good_first, sx, sy, 0.0)), None) == abi.PO_ERR_INVALID
    # the previous stack is intact
    assert e.debug_get("map_layers") == 2
    for k in range(2):
        d, *geo = e.get_map_layer(k)
        assert same(d, before[k][0]) and tuple(geo) == tuple(before[k][1:])
    # valid edge cases: no obstacle at all, an empty layer, a radius of zero
    none = e.rasterize_batch([[], []], sx, sy, res)
    assert (none == 255).all()
    e.set_map_stack_obstacles([[], [binding.obstacle_disc(0.1, 0.1, 0.0)]], sx, sy, res)
    assert same(e.get_map_layer(0)[0], edt_ref.distance_map(np.full((sx, sy), 255, dtype=np.uint8), res))  # the transform's no-obstacle rule, unchanged
    e.close()


def _sample_points(rng, sx, sy, res, px, py, n):
    return np.stack([px + (rng.random(n) - 0.5) * 1.2 * sx * res, py + (rng.random(n) - 0.5) * 1.2 * sy * res], axis=1)


@pytest.mark.gpu
def test_stack_from_obstacles_equals_the_stack_from_the_reference_images():
    sx, sy, res = 257, 129, 0.2
    lay = five_lists(11, sx, sy, res, POS5)
    obs, first = binding.pack_obstacles(lay)
    shared, _ = _bases(np.random.default_rng(12), sx, sy)
    images = raster_ref.rasterize(obs, first, sx, sy, res, POS5, base=shared)
    a, b = binding.Engine(0), binding.Engine(0)
    a.set_map_stack_obstacles(lay, sx, sy, res, POS5, base=shared)
    b.set_map_stack_occupancy(images, res, POS5)
    assert a.debug_get("map_layers") == M5 == b.debug_get("map_layers")
    rng = np.random.default_rng(13)
    for k in range(M5):
        da, *ga = a.get_map_layer(k)
        db, *gb = b.get_map_layer(k)
        assert same(da, db) and ga == gb == [res, POS5[k, 0], POS5[k, 1]], k
        xy = _sample_points(rng, sx, sy, res, POS5[k, 0], POS5[k, 1], 2000)  # 10 000 positions over the five layers, inside and outside
        sa, sb = a.map_sample_layer(k, xy), b.map_sample_layer(k, xy)
        assert same(sa[0], sb[0]) and same(sa[1], sb[1]) and 0 < sa[1].sum() < len(xy)
    a.close(); b.close()


SEEDS = (11, 12, 13)
B, M = 18, 3
LAYER_OF = np.arange(B, dtype=np.int32) % M


@pytest.mark.gpu
def test_plan_batch_end_to_end_from_disc_lists():
    """The three planning scenes of tests/test_map_stack.py, the stack built from the generator's own disc lists."""
    sc = [synth.make_planning_scenes(seed, 6, near=(2 if seed == 13 else 0), map_kw=dict(size_x=420, size_y=380, pos=(3.0 * i, -2.0 * i))) for i, seed in enumerate(SEEDS)]
    inp = {k: np.stack([sc[b % M][k][b // M] for b in range(B)]) for k in ("way_x", "way_y", "start", "goal")}
    res = sc[0]["map"][1]
    pos = np.array([[s["map"][2], s["map"][3]] for s in sc])
    lay = [[binding.obstacle_disc(*d) for d in s["discs"]] for s in sc]
    assert all(len(l) >= 60 for l in lay)
    obs, first = binding.pack_obstacles(lay)
    images = raster_ref.rasterize(obs, first, 420, 380, res, pos)
    plan = lambda eng: eng.plan_batch(inp["way_x"], inp["way_y"], inp["start"], inp["goal"], N=512)
    ref = binding.Engine(0)
    ref.set_map_stack_occupancy(images, res, pos)
    layer0 = plan(ref)  # no assignment: every instance on layer 0
    ref.set_map_assignment(LAYER_OF)
    want = plan(ref)
    ref.close()
    e = binding.Engine(0)
    e.set_map_stack_obstacles(lay, 420, 380, res, pos)
    e.set_map_assignment(LAYER_OF)
    got = plan(e)
    e.close()
    for name, g, w in zip(("states", "n_states", "ok", "stage", "info"), got, want):
        assert same(g, w), name
    assert got[2].sum() >= 12  # the scenes are planned, not refused
    differs = np.array([not all(same(g[b], w[b]) for g, w in zip(got, layer0)) for b in range(B)])
    assert differs[LAYER_OF != 0].any() and not differs[LAYER_OF == 0].any()


def _one_state_paths(n_inst):
    """n_inst paths of two states at the map's centre, solved: the collision check keeps them or not, depending on the layer each instance reads."""
    states = np.zeros((n_inst, 2, 5)); states[:, 1, 0] = 0.1; states[:, 1, 4] = 0.1
    info = np.zeros(n_inst, dtype=abi.INFO_DTYPE); info["status"] = 1
    return states, info


@pytest.mark.gpu
def test_handle_contract_of_the_obstacle_entries():
    import torch

    sx, sy, res = 128, 128, 0.25
    blocked, free = [binding.obstacle_disc(0.0, 0.0, 3.0)], [binding.obstacle_disc(12.0, 12.0, 0.5)]
    states, info = _one_state_paths(2)
    e = binding.Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = lambda lay: _to_device(*binding.pack_obstacles(lay))[:2]
    o1, f1 = dev([free, blocked])
    o2, f2 = dev([blocked, free])
    torch.cuda.synchronize()
    e.set_map_stack_obstacles_device(o1, f1, sx, sy, res)
    e.set_map_assignment(np.array([1, 0], dtype=np.int32))
    p1 = e.debug_get("map_ptr")
    assert e.postcheck_batch(states, info)[0].tolist() == [0, 2]  # instance 0 reads layer 1 (blocked), instance 1 layer 0 (free)
    # a same-shape refresh through the device entry: the layers are rebuilt where they were and the assignment stays
    e.set_map_stack_obstacles_device(o2, f2, sx, sy, res)
    assert e.debug_get("map_ptr") == p1 != 0 and e.debug_get("map_layers") == 2
    assert e.postcheck_batch(states, info)[0].tolist() == [2, 0]
    s3, i3 = _one_state_paths(3)
    with pytest.raises(binding.PoError):
        e.postcheck_batch(s3, i3)  # the table of length 2 is still in force: B = 3 > n
    # a larger M, then a larger size: the blocks grow (behind a synchronisation) and the layers are the right ones; the change of M drops the table
    lay3 = [blocked, free, [binding.obstacle_box(-4.0, 2.0, 3.0, 1.0, 0.4)]]
    o3, f3 = dev(lay3)
    torch.cuda.synchronize()
    e.set_map_stack_obstacles_device(o3, f3, sx, sy, res)
    assert e.debug_get("map_layers") == 3 and e.postcheck_batch(s3, i3)[0].tolist() == [0, 0, 0]  # no table: every instance reads layer 0
    img3 = raster_ref.rasterize(*binding.pack_obstacles(lay3), sx, sy, res)
    for k in range(3):
        assert same(e.get_map_layer(k)[0], edt_ref.distance_map(img3[k], res)), k
    bx, by = 200, 150
    e.set_map_stack_obstacles_device(o3, f3, bx, by, res)
    big = raster_ref.rasterize(*binding.pack_obstacles(lay3), bx, by, res)
    for k in range(3):
        d, *geo = e.get_map_layer(k)
        assert d.shape == (bx, by) and same(d, edt_ref.distance_map(big[k], res)), k
    # the same call twice, and on a second handle: bit-identical
    first_layers = [e.get_map_layer(k)[0] for k in range(3)]
    e.set_map_stack_obstacles_device(o3, f3, bx, by, res)
    other = binding.Engine(0)
    other.set_map_stack_obstacles(lay3, bx, by, res)
    for k in range(3):
        assert same(e.get_map_layer(k)[0], first_layers[k]) and same(other.get_map_layer(k)[0], first_layers[k])
    r1, r2 = e.rasterize_batch(lay3, bx, by, res), other.rasterize_batch(lay3, bx, by, res)
    assert same(r1, r2) and same(r1, big) and same(e.rasterize_batch(lay3, bx, by, res), r1)
    e.set_stream(None)
    e.close(); other.close()


@pytest.mark.gpu
def test_four_threads_with_a_handle_each():
    sx, sy, res = 129, 95, 0.2
    jobs = []
    for t in range(4):
        lay = five_lists(50 + t, sx, sy, res, POS5)
        obs, first = binding.pack_obstacles(lay)
        images = raster_ref.rasterize(obs, first, sx, sy, res, POS5)
        jobs.append((lay, images, [edt_ref.distance_map(images[k], res) for k in range(M5)]))
    errors = []

    def work(t):
        try:
            lay, images, layers = jobs[t]
            e = binding.Engine(0)
            for _ in range(3):
                assert same(e.rasterize_batch(lay, sx, sy, res, POS5), images)
                e.set_map_stack_obstacles(lay, sx, sy, res, POS5)
                for k in range(M5):
                    assert same(e.get_map_layer(k)[0], layers[k])
            e.close()
        except Exception as ex:  # noqa: BLE001
            errors.append((t, repr(ex)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
