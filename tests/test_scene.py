"""The static world of the map stack: a world grid on the handle and polygon rings, rasterised on the device (csrc/po_scene.hip; po_set_world_occupancy*,
po_rasterize_scene_batch*, po_set_map_stack_scene*).

The images are a function of IEEE double operations that are each rounded once (include/po_hip.h states them), so every comparison here is BIT equality on byte views
of every element; nothing is a tolerance.  The CPU reference is tests/scene_ref.py (numpy, one ufunc per operation, no culling).

CPU: the reference against a scalar loop over the definition, exact lattice counts, the angle-sum winding number, world windows, the ABI mirror, argument checks
without a device, the host mirror's test source.
GPU: a size x ring case x base matrix, ties on every tile boundary, world grids, both entries and stream order, bad device tables (clamped, never out of bounds), host
validation, the stack against the occupancy route, po_plan_batch end to end, the handle contract."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import edt_ref
import raster_ref
import scene_ref
from path_optimizer_amd import abi, binding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["po_set_world_occupancy", "po_set_world_occupancy_device", "po_rasterize_scene_batch", "po_rasterize_scene_batch_device",
               "po_set_map_stack_scene", "po_set_map_stack_scene_device"]
SOLID, FREE = abi.PO_RING_SOLID, abi.PO_RING_FREE
# (size_x, size_y): one cell, one line either way, sizes around the tile (64 x 16) and the 4-cell store, more than one tile
SIZES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (257, 129), (513, 511)]
M5 = 5
POS5 = np.array([[0.0, 0.0], [1.5, -2.0], [-7.25, 3.0], [40.0, 40.5], [0.1, 0.3]])
L_RING = np.array([(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)], dtype=np.float64)
SQUARE = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], dtype=np.float64)
BOWTIE = np.array([(-2, -1), (2, 1), (2, -1), (-2, 1)], dtype=np.float64)


def same(a, b):
    """Bitwise equality of two arrays (any dtype)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def scene_struct(sx, sy, res, rings=None, use_world=0, obs=None, first=None, M=1, pos=(0.0, 0.0)):
    """po_scene over host arrays, exactly as given (nothing derived, nothing checked); rings = (verts, start, flags, n_shared, first) or an abi.PoRings."""
    if first is None:
        first = np.zeros(M + 1, dtype=np.int32)
    ls = abi.PoObstacleLists(p(obs), p(first), 0 if obs is None else len(obs), None, 0, sx, sy, res, pos[0], pos[1])
    if rings is None:
        rg = abi.PoRings()
    elif isinstance(rings, abi.PoRings):
        rg = rings
    else:
        rg = abi.PoRings(p(rings[0]), p(rings[1]), p(rings[2]), len(rings[2]), len(rings[0]), rings[3], p(rings[4]))
    return abi.PoScene(ls, rg, use_world), (first, obs, rings)


def star(rng, cx, cy, rmin, rmax, n, reverse=False):
    """A star-shaped ring: n vertices at sorted random angles around (cx, cy), radii in [rmin, rmax]."""
    ang = np.sort(rng.uniform(0, 2 * math.pi, n))
    r = rng.uniform(rmin, rmax, n)
    xy = np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], axis=1)
    return xy[::-1].copy() if reverse else xy


def ref_images(lay, rings, sx, sy, res, pos_xy, base=None, world=None):
    obs, first = binding.pack_obstacles(lay)
    return scene_ref.rasterize(obs, first, rings, sx, sy, res, pos_xy, base=base, world=world)


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def _scalar_contains(xy, px, py):
    n, count = len(xy), 0
    for e in range(n):
        ax, ay = float(xy[e][0]), float(xy[e][1])
        bx, by = float(xy[(e + 1) % n][0]), float(xy[(e + 1) % n][1])
        straddles = (ay > py) != (by > py)
        t1 = (bx - ax) * (py - ay)
        t2 = (by - ay) * (px - ax)
        t = t1 - t2
        right = (t > 0) if by > ay else (t < 0)
        count += straddles and right
    return count % 2 == 1


def _scalar_world(world, wres, wpos, outside, px, py):
    wsx, wsy = world.shape
    lx, ly = float(wsx) * wres, float(wsy) * wres
    tx, ty = -((px - wpos[0]) - 0.5 * lx), -((py - wpos[1]) - 0.5 * ly)
    if tx >= 0 and ty >= 0 and tx < lx and ty < ly:
        ix, iy = int(-(((px - 0.5 * lx) - wpos[0]) / wres)), int(-(((py - 0.5 * ly) - wpos[1]) / wres))  # int() truncates
        if 0 <= ix < wsx and 0 <= iy < wsy:
            return world[ix, iy] == 0
    return bool(outside)


def test_reference_agrees_with_a_scalar_loop_over_the_definition():
    sx, sy, res, pos = 33, 17, 0.2, (1.3, -0.7)
    rng = np.random.default_rng(5)
    l_ring = L_RING * 0.9 + (0.4, -1.6)
    free = star(rng, 1.2, -0.6, 1.0, 2.6, 9)
    world = (rng.random((23, 14)) > 0.2).astype(np.uint8)
    wres, wpos = 0.31, (0.95, -0.33)
    shared, layers = [(free, FREE)], [[(l_ring, SOLID)], [], [(l_ring[::-1], SOLID), (l_ring + 0.37, FREE)]]
    rings = binding.pack_rings(shared, layers)
    lay = [[binding.obstacle_disc(2.0, -1.0, 0.5)], [], []]
    obs, first = binding.pack_obstacles(lay)
    for outside in (0, 1):
        got = scene_ref.rasterize(obs, first, rings, sx, sy, res, pos=pos, world=(world, wres, wpos, outside))
        want = np.empty((3, sx, sy), dtype=np.uint8)
        half_x, half_y = 0.5 * (sx * res) - 0.5 * res, 0.5 * (sy * res) - 0.5 * res
        for k in range(3):
            mine = shared + layers[k]
            for i in range(sx):
                for j in range(sy):
                    px = (pos[0] + half_x) + res * float(-i)
                    py = (pos[1] + half_y) + res * float(-j)
                    hit = raster_ref.covers(obs[0], np.array([[px]]), np.array([[py]]))[0, 0] if k == 0 else False
                    hit = hit or _scalar_world(world, wres, wpos, outside, px, py)
                    hit = hit or any(_scalar_contains(xy, px, py) for xy, f in mine if f == SOLID)
                    hit = hit or not any(_scalar_contains(xy, px, py) for xy, f in mine if f == FREE)
                    want[k, i, j] = 0 if hit else 255
        assert same(got, want), outside
        assert all(0 < (got[k] == 0).sum() < sx * sy for k in range(3)) and not same(got[0], got[1]) and not same(got[1], got[2])


def _lattice(shared, size=33):
    """Contained cells on the lattice: 33 x 33 cells of 0.25 centred at (0, 0) — centres are the multiples of 0.25 in [-4, 4], all exact."""
    rings = binding.pack_rings(shared)
    return scene_ref.ring_occupied(rings, 1, size, size, 0.25, np.zeros((1, 2)))[0]


def _cell(x, y):
    return int(round((4.0 - x) / 0.25)), int(round((4.0 - y) / 0.25))


def test_reference_exact_lattice_facts():
    assert np.array_equal(raster_ref.cell_centres(33, 0.25, 0.0), 4.0 - 0.25 * np.arange(33))
    for ring in (L_RING, L_RING[::-1]):  # orientation does not matter
        assert _lattice([(ring, SOLID)]).sum() == 48
    sq = _lattice([(SQUARE, SOLID)])
    assert sq.sum() == 64 and sq[_cell(-1, -1)] and not sq[_cell(1, 1)]  # the low edges belong to the box, the high edges do not
    assert sq[_cell(-1, 0.75)] and not sq[_cell(-1, 1)] and sq[_cell(0.75, -1)] and not sq[_cell(1, -1)]
    obs, first = binding.pack_obstacles([[binding.obstacle_polygon(SQUARE)]])
    poly = raster_ref.covered(obs, first, 33, 33, 0.25, np.zeros((1, 2)))[0]
    assert poly.sum() == 81 and not (sq & ~poly).any()  # POLY is closed; the ring's cells are a subset
    assert _lattice([(BOWTIE, SOLID)]).sum() == 64  # self-intersecting: even-odd
    assert _lattice([(SQUARE, FREE)]).sum() == 1089 - 64 == 1025
    two = _lattice([(SQUARE - (2, 2), FREE), (SQUARE + (1.5, 1.5), FREE)])  # two disjoint FREE squares free both of them
    assert two.sum() == 1089 - 128 and not two[_cell(-2, -2)] and not two[_cell(1.5, 1.5)] and two[_cell(0, 0)]
    island = _lattice([(SQUARE * 3, FREE), (SQUARE, SOLID)])  # a SOLID ring inside a FREE one is occupied
    assert island[_cell(0, 0)] and not island[_cell(2, 2)] and island[_cell(3.5, 0)] and island.sum() == 1089 - 24 * 24 + 64
    flat = _lattice([(np.array([(-1.0, 0.0), (1.0, 0.0), (0.0, 0.0)]), SOLID)])  # horizontal edges never count
    assert flat.sum() == 0


def test_reference_agrees_with_the_angle_sum_winding_number_on_a_star_shaped_ring():
    sx, sy, res, pos = 97, 61, 0.173, (0.31, -0.77)
    xy = star(np.random.default_rng(1), pos[0], pos[1], 1.0, 5.0, 40)
    got = scene_ref.ring_occupied(binding.pack_rings([(xy, SOLID)]), 1, sx, sy, res, np.array([pos]))[0]
    X = raster_ref.cell_centres(sx, res, pos[0])[:, None, None]
    Y = raster_ref.cell_centres(sy, res, pos[1])[None, :, None]
    ux, uy = xy[None, None, :, 0] - X, xy[None, None, :, 1] - Y
    vx, vy = np.roll(ux, -1, axis=2), np.roll(uy, -1, axis=2)
    turn = np.arctan2(ux * vy - uy * vx, ux * vx + uy * vy).sum(axis=2)  # 2 pi times the winding number (a star-shaped ring winds once)
    want = np.abs(turn) > math.pi
    assert (got != want).sum() == 0 and 500 < got.sum() < sx * sy - 500


def test_reference_world_windows():
    rng = np.random.default_rng(2)
    world = (rng.random((200, 120)) > 0.3).astype(np.uint8) * 255
    wres, wpos = 0.2, (3.0, -1.0)
    # a 40 x 30 window of the same resolution whose centre is a whole number of cells off the world's: layer cell (i, j) is world cell (i + 70, j + 42)
    pos = np.array([[wpos[0] + 0.2 * 10, wpos[1] + 0.2 * 3]])
    win = scene_ref.world_occupied(world, wres, wpos, 0, 1, 40, 30, 0.2, pos)[0]
    assert same(win, world[70:110, 42:72] == 0)
    assert same(win, scene_ref.world_occupied(world, wres, wpos, 1, 1, 40, 30, 0.2, pos)[0])  # wholly inside: outside_occupied is not looked at
    # hanging 15 columns over the world's low-index edge (larger x): exactly 15 x 30 cells flip with outside_occupied
    pos = np.array([[wpos[0] + 0.2 * (100 - 20 + 15), wpos[1]]])
    a = scene_ref.world_occupied(world, wres, wpos, 0, 1, 40, 30, 0.2, pos)[0]
    b = scene_ref.world_occupied(world, wres, wpos, 1, 1, 40, 30, 0.2, pos)[0]
    assert (a != b).sum() == 15 * 30 and (a != b)[:15].all() and same(a[15:], world[0:25, 45:75] == 0) and b[:15].all() and not a[:15].any()


def test_struct_layouts_and_prototypes_match_the_header():
    fr, fs = ["verts", "start", "flags", "n_rings", "n_verts", "n_shared", "first"], ["lists", "rings", "use_world"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "po_hip.h"\n'
           'int (*a)(po_handle, const po_occupancy *, int) = po_set_world_occupancy;\n'
           'int (*b)(po_handle, const po_occupancy *, int) = po_set_world_occupancy_device;\n'
           'int (*c)(po_handle, int, const po_scene *, const double *, unsigned char *) = po_rasterize_scene_batch;\n'
           'int (*d)(po_handle, int, const po_scene *, const double *, unsigned char *) = po_rasterize_scene_batch_device;\n'
           'int (*e)(po_handle, int, const po_scene *, const double *) = po_set_map_stack_scene;\n'
           'int (*f)(po_handle, int, const po_scene *, const double *) = po_set_map_stack_scene_device;\n'
           'int main(){printf("%d %d %d %d %zu %zu %zu %zu %zu", PO_ABI_VERSION, PO_RING_SOLID, PO_RING_FREE, PO_RING_MAX_VERTS, sizeof(po_obstacle),'
           ' sizeof(po_obstacle_lists), sizeof(po_occupancy), sizeof(po_rings), sizeof(po_scene));'
           + "".join(f'printf(" %zu", offsetof(po_rings, {f}));' for f in fr) + "".join(f'printf(" %zu", offsetof(po_scene, {f}));' for f in fs)
           + 'printf("\\n");return (a && b && c && d && e && f) ? 0 : 1;}\n')
    lib_dir = os.path.join(ROOT, "path_optimizer_amd")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t"),
                               "-L", lib_dir, "-l:libpo_hip.so", "-Wl,-rpath," + lib_dir])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got[:4] == [abi.PO_ABI_VERSION, SOLID, FREE, abi.PO_RING_MAX_VERTS] == [7, 0, 1, 4096]
    assert got[4:7] == [136, 72, 40] == [ctypes.sizeof(abi.PoObstacle), ctypes.sizeof(abi.PoObstacleLists), ctypes.sizeof(abi.PoOccupancy)]  # unchanged
    assert got[7:9] == [ctypes.sizeof(abi.PoRings), ctypes.sizeof(abi.PoScene)]
    assert got[9:16] == [getattr(abi.PoRings, f).offset for f in fr] and got[16:] == [getattr(abi.PoScene, f).offset for f in fs]
    assert [n for n, _ in abi.PoRings._fields_] == fr and [n for n, _ in abi.PoScene._fields_] == fs


def test_new_entries_are_exported_and_check_their_arguments_without_a_device():
    L = binding.lib()
    for name in NEW_ENTRIES:
        assert name in binding.EXPORTS
        getattr(L, name)
    sc, _keep = scene_struct(4, 4, 0.2, binding.pack_rings([(SQUARE, SOLID)]))
    out = np.zeros((1, 4, 4), dtype=np.uint8)
    img = np.zeros((4, 4), dtype=np.uint8)
    oc = abi.PoOccupancy(p(img), 4, 4, 0.2, 0.0, 0.0)
    fake = ctypes.c_void_p(8)  # (never dereferenced: the struct is looked at first)
    for h, s in ((None, ctypes.byref(sc)), (fake, None)):
        assert L.po_rasterize_scene_batch(h, 1, s, None, p(out)) == abi.PO_ERR_INVALID
        assert L.po_rasterize_scene_batch_device(h, 1, s, None, p(out)) == abi.PO_ERR_INVALID
        assert L.po_set_map_stack_scene(h, 1, s, None) == abi.PO_ERR_INVALID
        assert L.po_set_map_stack_scene_device(h, 1, s, None) == abi.PO_ERR_INVALID
    assert L.po_set_world_occupancy(None, ctypes.byref(oc), 0) == abi.PO_ERR_INVALID
    assert L.po_set_world_occupancy_device(None, ctypes.byref(oc), 0) == abi.PO_ERR_INVALID
    # pack_rings: shared rings first, then each layer's own
    v, s, f, ns, first = binding.pack_rings([(SQUARE, FREE)], [[(L_RING, SOLID)], [], [(BOWTIE, SOLID), (SQUARE, FREE)]])
    assert s.tolist() == [0, 4, 10, 14, 18] and f.tolist() == [1, 0, 0, 1] and ns == 1 and first.tolist() == [1, 2, 2, 4]
    assert v.shape == (18, 2) and v.dtype == np.float64 and same(v[4:10], L_RING) and s.dtype == f.dtype == first.dtype == np.int32
    assert binding.pack_rings([(SQUARE, FREE)])[4] is None


def test_host_mirror_scene_test_source_compiles_and_links():
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "scene_test"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(host, "scene_test"))
    src = open(os.path.join(host, "test", "scene_test.cpp")).read()
    assert "MapStack::fromScene" in src and "Ring::free" in src and "Ring::solid" in src and "World" in src


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.mark.gpu
def test_host_mirror_scene_program():
    """Ring, World and MapStack::fromScene end to end: the lattice counts, a world window and the ring-free case read back through the distance layers."""
    host = os.path.join(ROOT, "path_optimizer_amd", "host")
    subprocess.check_call(["make", "-C", host, "scene_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "scene_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scene_test passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]


def small_lists(seed, sx, sy, res, pos_xy):
    """Discs and boxes for every layer but the first (6 + 3 each), inside and across the borders."""
    rng = np.random.default_rng(seed)
    rmax = max(0.08 * max(sx, sy) * res, 2.0 * res)
    lay = [[]]
    for k in range(1, M5):
        x0, x1 = pos_xy[k][0] - 0.55 * sx * res, pos_xy[k][0] + 0.55 * sx * res
        y0, y1 = pos_xy[k][1] - 0.55 * sy * res, pos_xy[k][1] + 0.55 * sy * res
        lay.append([binding.obstacle_disc(rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(0.3 * res, rmax)) for _ in range(6)]
                   + [binding.obstacle_box(rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(0.3 * res, rmax), rng.uniform(0.3 * res, 0.6 * rmax),
                                           rng.uniform(-math.pi, math.pi)) for _ in range(3)])
    return lay


def ring_cases(seed, sx, sy, res, pos_xy):
    """name -> (shared, per layer) ring lists (None: no ring at all)."""
    rng = np.random.default_rng(seed)
    wx, wy = sx * res, sy * res
    ext = max(wx, wy)
    at = lambda ring, k, s=1.0: ring * s + pos_xy[k]
    tri = np.array([(-0.31, -0.27), (0.38, -0.12), (-0.05, 0.33)]) * (wx, wy)
    cases = {"none": None}
    cases["triangle"] = ([], [[(at(tri, k), FREE if k == 2 else SOLID)] for k in range(M5)])
    cases["L"] = ([], [[(at(L_RING - 1.0, k, 0.21 * ext), FREE if k == 1 else SOLID)] for k in range(M5)])
    far = SQUARE * ext + (5.0 * ext + 7.0, -3.0 * ext)
    cases["outside"] = ([], [[(at(far, k), SOLID if k < 3 else FREE)] for k in range(M5)])
    if sx * sy <= 257 * 129:
        cases["star300"] = ([], [[(star(rng, pos_xy[k][0], pos_xy[k][1], 0.15 * ext, 0.55 * ext, 300, reverse=k == 4), FREE if k % 2 == 0 else SOLID)] for k in range(M5)])
    many = [(star(rng, pos_xy[3][0] + rng.uniform(-0.5, 0.5) * wx, pos_xy[3][1] + rng.uniform(-0.5, 0.5) * wy, 0.02 * ext, 0.09 * ext, int(rng.integers(5, 13))), SOLID)
            for _ in range(64)]
    many += [(star(rng, pos_xy[3][0] + rng.uniform(-0.3, 0.3) * wx, pos_xy[3][1] + rng.uniform(-0.3, 0.3) * wy, 0.1 * ext, 0.3 * ext, int(rng.integers(5, 13))), FREE)
             for _ in range(6)]
    cases["many70"] = ([], [[], [], [], many, []])
    # shared: a FREE ring around layers 0, 1, 2 and 4 and a SOLID one across them; layer 3 lies far away from both
    hub = pos_xy[[0, 1, 2, 4]].mean(axis=0)
    shared = [(star(rng, hub[0], hub[1], 0.6 * ext + 6.0, 0.8 * ext + 9.0, 24), FREE), (at(BOWTIE, 0, 0.2 * ext), SOLID)]
    cases["shared+own"] = (shared, [[(at(tri, 0, 0.5), SOLID)], [], [(at(tri, 2), SOLID), (at(L_RING, 2, 0.1 * ext), SOLID)], [(at(SQUARE, 3, 0.3 * ext), FREE)], []])
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rasterize_scene_batch_matches_the_reference(size):
    sx, sy = size
    res = 0.2
    lay = small_lists(200 + sx, sx, sy, res, POS5)
    obs, first = binding.pack_obstacles(lay)
    cov = raster_ref.covered(obs, first, sx, sy, res, POS5)  # once; every ring case and base mode shares it
    rng = np.random.default_rng(9 + sy)
    shared_base, per_layer = (rng.random((sx, sy)) >= 0.05).astype(np.uint8) * 255, (rng.random((M5, sx, sy)) >= 0.05).astype(np.uint8)
    e = binding.Engine(0)
    for name, case in ring_cases(300 + sy, sx, sy, res, POS5).items():
        rings = None if case is None else binding.pack_rings(*case)
        ring_occ = np.zeros_like(cov) if rings is None else scene_ref.ring_occupied(rings, M5, sx, sy, res, POS5)
        if name == "outside":
            assert not ring_occ[:3].any() and ring_occ[3:].all()  # SOLID: nothing; FREE: every cell occupied
        if name == "many70":
            assert len(case[1][3]) == 70 and (sx * sy < 4000 or 0 < ring_occ[3].sum() < sx * sy)
        if name == "star300" and sx * sy > 4000:
            assert all(0 < ring_occ[k].sum() < sx * sy for k in range(M5))
        for base_name, base in (("none", None), ("shared", shared_base), ("per layer", per_layer)):
            got = e.rasterize_scene_batch(lay, rings, sx, sy, res, POS5, base=base)
            want = raster_ref.to_cells(cov | ring_occ, base)
            assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 255}
            assert same(got, want), (name, base_name, int((got != want).sum()), np.argwhere(got != want)[:5])
    e.close()


@pytest.mark.gpu
def test_a_ring_of_exactly_4096_vertices():
    sx = sy = 64
    pos = np.array([[0.0, 0.0], [2.0, -1.5]])
    rng = np.random.default_rng(41)
    big = star(rng, 0.5, -0.5, 2.0, 6.0, abi.PO_RING_MAX_VERTS)
    rings = binding.pack_rings([(big, FREE)], [[], [(SQUARE * 1.3 + (2.0, -1.5), SOLID)]])
    lay = [[binding.obstacle_disc(-3.0, 3.0, 1.0)], []]
    e = binding.Engine(0)
    got = e.rasterize_scene_batch(lay, rings, sx, sy, 0.2, pos)
    want = ref_images(lay, rings, sx, sy, 0.2, pos)
    assert same(got, want), np.argwhere(got != want)[:5]
    assert all(200 < (got[k] == 0).sum() < sx * sy - 200 for k in range(2))
    e.close()


@pytest.mark.gpu
def test_ties_on_every_tile_boundary():
    """Vertices, vertical edges and horizontal edges EXACTLY on cell centres, swept over every residue modulo the tile (64 x 16) and the 4-cell store in both
    directions: a cull that is not exact, or an off-by-one at a tile edge, loses or gains a tie cell here."""
    centre = lambda i, j: (15.875 - 0.25 * i, 15.875 - 0.25 * j)  # 128 cells of 0.25 centred at 0
    e = binding.Engine(0)
    for ring, count in ((SQUARE, 64), (L_RING, 48)):
        for along_j in (False, True):
            for flag in (SOLID, FREE):
                layers = [[(ring + (centre(40, 24 + k) if along_j else centre(24 + k, 40)), flag)] for k in range(80)]
                rings = binding.pack_rings([], layers)
                got = e.rasterize_scene_batch([[] for _ in range(80)], rings, 128, 128, 0.25)
                want = raster_ref.to_cells(scene_ref.ring_occupied(rings, 80, 128, 128, 0.25, np.zeros((80, 2))))
                assert same(got, want), (count, along_j, flag, np.argwhere(got != want)[:5])
                contained = (got == 0) if flag == SOLID else (got != 0)
                assert (contained.reshape(80, -1).sum(axis=1) == count).all()
    e.close()


def _world_cases():
    rng = np.random.default_rng(17)
    img = lambda wx, wy: (rng.random((wx, wy)) >= 0.3).astype(np.uint8) * 255
    return [("aligned", img(400, 300), 0.2, (1.0, -0.4)), ("another resolution", img(150, 170), 0.3, (0.35, 0.2)), ("smaller than a layer", img(20, 10), 0.2, (1.5, -2.0)),
            ("1 x 1", np.zeros((1, 1), dtype=np.uint8), 0.7, (0.1, 0.3)), ("larger again", img(333, 77), 0.25, (-3.0, 2.0))]


@pytest.mark.gpu
def test_world_grids():
    sx, sy, res = 63, 65, 0.2
    lay = small_lists(4, sx, sy, res, POS5)
    e = binding.Engine(0)
    assert e.debug_get("world_cells") == 0
    for name, world, wres, wpos in _world_cases():  # one handle: every install replaces a world of another size
        for outside in (0, 1):
            e.set_world_occupancy(world, wres, wpos[0], wpos[1], outside_occupied=outside)
            assert e.debug_get("world_cells") == world.size
            got = e.rasterize_scene_batch(lay, None, sx, sy, res, POS5, use_world=True)
            wocc = scene_ref.world_occupied(world, wres, wpos, outside, M5, sx, sy, res, POS5)
            want = ref_images(lay, None, sx, sy, res, POS5, world=(world, wres, wpos, outside))
            assert same(got, want), (name, outside, np.argwhere(got != want)[:5])
            assert wocc[3].all() == bool(outside) and wocc[3].any() == bool(outside)  # layer 3 lies wholly outside every one of these worlds
            if name in ("aligned", "another resolution"):
                assert 0 < wocc[0].sum() < sx * sy
    e.set_world_occupancy(None, 1.0)
    assert e.debug_get("world_cells") == 0
    with pytest.raises(binding.PoError):
        e.rasterize_scene_batch(lay, None, sx, sy, res, POS5, use_world=True)
    e.close()


def _to_device(obs, first, rings=None, base=None, pos=None):
    import torch

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(-1, 136).copy()).cuda()
    d_rings = None if rings is None else (t(rings[0]), t(rings[1]), t(rings[2]), rings[3], t(rings[4]))
    return d_obs, t(first), d_rings, (None if base is None else t(np.ascontiguousarray(base.transpose(0, 2, 1)))), t(pos)


@pytest.mark.gpu
def test_both_entries_give_the_same_bytes_and_the_device_entry_is_ordered_by_the_stream():
    import torch

    sx, sy, res = 257, 129, 0.2
    lay = small_lists(3, sx, sy, res, POS5)
    obs, first = binding.pack_obstacles(lay)
    rings = binding.pack_rings(*ring_cases(5, sx, sy, res, POS5)["shared+own"])
    per_layer = (np.random.default_rng(8).random((M5, sx, sy)) >= 0.05).astype(np.uint8)
    world, wres, wpos = (np.random.default_rng(9).random((300, 200)) >= 0.2).astype(np.uint8), 0.3, (0.5, 0.25)
    e = binding.Engine(0)
    e.set_world_occupancy(world, wres, wpos[0], wpos[1], outside_occupied=False)
    host = e.rasterize_scene_batch(lay, rings, sx, sy, res, POS5, base=per_layer, use_world=True)
    assert same(host, ref_images(lay, rings, sx, sy, res, POS5, base=per_layer, world=(world, wres, wpos, 0)))
    d_obs, d_first, d_rings, d_base, d_pos = _to_device(obs, first, rings, per_layer, POS5)
    d_world = torch.from_numpy(np.ascontiguousarray(world.T)).cuda()
    out = torch.full((M5, sy, sx), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the inputs are in place; from here on the stream alone orders the work
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # torch's current stream: a stream of its own (the default stream's handle is NULL = "the handle's own stream")
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        e.set_world_occupancy_device(d_world, wres, wpos[0], wpos[1], outside_occupied=False)
        e.rasterize_scene_batch_device(d_obs, d_first, d_rings, out, res, d_pos, base=d_base, use_world=True)
        flipped = 255 - out  # a consumer on the same stream, no synchronisation in between
        got = out.cpu().numpy().transpose(0, 2, 1)
        assert same(got, host)
        assert same(255 - flipped.cpu().numpy().transpose(0, 2, 1), host)
    with pytest.raises(ValueError):
        e.rasterize_scene_batch_device(d_obs, d_first, d_rings, out.transpose(1, 2), res, d_pos)  # not contiguous: refused, not misread
    e.set_stream(None)
    e.close()


@pytest.mark.gpu
def test_bad_device_tables_are_clamped_and_never_read_outside_the_arrays():
    """What a device entry cannot validate.  Every value here is made harmless by the clamps the header documents, so the call returns and the result is the
    documented one — the reference applies the same rule."""
    import torch

    sx, sy, res = 100, 70, 0.25
    rng = np.random.default_rng(23)
    long_ring = star(rng, 0.0, 0.0, 3.0, 8.0, 5000)  # read as its first 4096 vertices, closing from vertex 4095 to vertex 0
    two = np.array([(-5.0, -5.0), (5.0, 5.0)])
    nan_ring, inf_ring = SQUARE * 4 + (3.0, 2.0), SQUARE * 5 - (4.0, 1.0)
    nan_ring[2, 0], inf_ring[1, 1] = float("nan"), float("inf")
    verts, start, flags, _, _ = binding.pack_rings([(long_ring, SOLID), (two, FREE), (SQUARE * 3 - (6.0, 2.0), SOLID), (nan_ring, SOLID), (inf_ring, SOLID),
                                                    (L_RING * 3, FREE), (BOWTIE * 2, SOLID)])
    flags[6] = 7  # an unknown flag: ignored
    nv, nr = len(verts), len(flags)
    # per layer: (start, n_shared, first).  Layer ranges pick single rings so that each defect is seen on its own
    good_first = np.array([0, 1, 2, 3, 4, 5, 7], dtype=np.int32)
    tables = {"one ring per layer": (start, 0, good_first),
              "start past n_verts, descending, negative": (np.array([0, 5000, nv + 100000, 5010, -3, nv, 2, 9], dtype=np.int32), 0, good_first),
              "first out of range": (start, 0, np.array([-4, 1, 1000000, 2, 3, -1, nr + 5], dtype=np.int32)),
              "n_shared past n_rings": (start, nr + 9, good_first), "n_shared negative": (start, -2, good_first)}
    e = binding.Engine(0)
    obs0 = torch.zeros((0, 136), dtype=torch.uint8, device="cuda")
    ofirst = torch.zeros(7, dtype=torch.int32, device="cuda")
    d_verts = torch.from_numpy(verts).cuda()
    d_flags = torch.from_numpy(flags).cuda()
    for name, (st, ns, fi) in tables.items():
        want = raster_ref.to_cells(scene_ref.ring_occupied((verts, st, flags, ns, fi), 6, sx, sy, res, np.zeros((6, 2))))
        out = torch.full((6, sy, sx), 9, dtype=torch.uint8, device="cuda")
        e.rasterize_scene_batch_device(obs0, ofirst, (d_verts, torch.from_numpy(st).cuda(), d_flags, ns, torch.from_numpy(fi).cuda()), out, res)
        torch.cuda.synchronize()
        got = out.cpu().numpy().transpose(0, 2, 1)
        assert same(got, want), (name, np.argwhere(got != want)[:5])
        if name == "one ring per layer":
            cut = raster_ref.to_cells(scene_ref.ring_occupied(binding.pack_rings([(long_ring[:4096], SOLID)]), 1, sx, sy, res, np.zeros((1, 2))))
            assert same(got[0], cut[0]) and 500 < (got[0] == 0).sum() < sx * sy
            assert (got[1] == 255).all()  # a 2-vertex ring is ignored and does not count as a FREE ring of the layer
            assert 0 < (got[2] == 0).sum() and 0 < (got[5] == 0).sum() < sx * sy  # (layer 5: the FREE L; the ring with flag 7 adds nothing)
            only_l = raster_ref.to_cells(scene_ref.ring_occupied(binding.pack_rings([(L_RING * 3, FREE)]), 1, sx, sy, res, np.zeros((1, 2))))
            assert same(got[5], only_l[0])
    e.close()


@pytest.mark.gpu
def test_host_entries_validate_before_they_touch_the_handle():
    L = binding.lib()
    sx, sy, res = 40, 30, 0.25
    e = binding.Engine(0)
    world = (np.random.default_rng(1).random((50, 50)) > 0.5).astype(np.uint8)
    e.set_world_occupancy(world, 0.25, outside_occupied=True)
    prev_rings = binding.pack_rings([(SQUARE * 2, FREE)], [[(SQUARE, SOLID)], []])
    e.set_map_stack_scene([[], []], prev_rings, sx, sy, res, use_world=True)
    before = [e.get_map_layer(k) for k in range(2)]
    verts, start, flags, ns, first = binding.pack_rings([(SQUARE * 2, FREE)], [[(L_RING, SOLID)], [(BOWTIE, SOLID)]])
    i32 = lambda *v: np.array(v, dtype=np.int32)
    bad_v = lambda val: np.concatenate([verts[:5], [[val, 0.0]], verts[6:]])
    cases = {"start[0] != 0": (verts, i32(1, 4, 10, 14), flags, ns, first), "start descending": (verts, i32(0, 10, 4, 14), flags, ns, first),
             "start[n_rings] > n_verts": (verts, i32(0, 4, 10, 15), flags, ns, first), "a 2-vertex ring": (verts, i32(0, 4, 6, 14), flags, ns, first),
             "a 4097-vertex ring": (np.zeros((4105, 2)), i32(0, 4, 4101, 4105), flags, ns, first),
             "nan vertex": (bad_v(float("nan")), start, flags, ns, first), "infinite vertex": (bad_v(float("-inf")), start, flags, ns, first),
             "unknown flag": (verts, start, i32(1, 2, 0), ns, first), "negative flag": (verts, start, i32(1, -1, 0), ns, first),
             "first NULL with n_shared != n_rings": (verts, start, flags, ns, None), "first[0] != n_shared": (verts, start, flags, ns, i32(0, 2, 3)),
             "first descending": (verts, start, flags, ns, i32(1, 3, 2)), "first[M] > n_rings": (verts, start, flags, ns, i32(1, 2, 4)),
             "n_shared negative": (verts, start, flags, -1, i32(-1, 2, 3)), "n_shared > n_rings": (verts, start, flags, 4, i32(4, 4, 4))}
    out = np.full((2, sy, sx), 3, dtype=np.uint8)

    def refused(sc, code=abi.PO_ERR_INVALID, name=""):
        assert L.po_set_map_stack_scene(e._h, 2, ctypes.byref(sc), None) == code, name
        assert L.po_rasterize_scene_batch(e._h, 2, ctypes.byref(sc), None, p(out)) == code, name

    for name, rings in cases.items():
        refused(scene_struct(sx, sy, res, rings, M=2)[0], name=name)
    good = (verts, start, flags, ns, first)
    for uw in (2, -1):
        refused(scene_struct(sx, sy, res, good, use_world=uw, M=2)[0], name=f"use_world {uw}")
    # anything po_rasterize_batch refuses: a bad obstacle list under a good ring table
    obs = binding.pack_obstacles([[binding.obstacle_disc(0.0, 0.0, -1.0)]])[0]
    refused(scene_struct(sx, sy, res, good, obs=obs, first=i32(0, 1, 1), M=2)[0], name="negative radius")
    refused(scene_struct(sx, sy, res, good, first=i32(0, 1, 1), M=2)[0], name="first[M] > n_obs")
    # limits
    refused(scene_struct(4097, 4, res, good, M=2)[0], abi.PO_ERR_UNSUPPORTED, "size")
    img = np.zeros((4, 4), dtype=np.uint8)
    for oc, outside, code in ((abi.PoOccupancy(p(img), 16385, 1, 0.2, 0.0, 0.0), 0, abi.PO_ERR_UNSUPPORTED), (abi.PoOccupancy(p(img), 1, 16385, 0.2, 0.0, 0.0), 0, abi.PO_ERR_UNSUPPORTED),
                              (abi.PoOccupancy(p(img), 4, 4, 0.2, 0.0, 0.0), 2, abi.PO_ERR_INVALID), (abi.PoOccupancy(None, 4, 4, 0.2, 0.0, 0.0), 0, abi.PO_ERR_INVALID),
                              (abi.PoOccupancy(p(img), 0, 4, 0.2, 0.0, 0.0), 0, abi.PO_ERR_INVALID), (abi.PoOccupancy(p(img), 4, 4, 0.0, 0.0, 0.0), 0, abi.PO_ERR_INVALID),
                              (abi.PoOccupancy(p(img), 4, 4, float("nan"), 0.0, 0.0), 0, abi.PO_ERR_INVALID), (abi.PoOccupancy(p(img), 4, 4, 0.2, float("inf"), 0.0), 0, abi.PO_ERR_INVALID)):
        assert L.po_set_world_occupancy(e._h, ctypes.byref(oc), outside) == code
        assert L.po_set_world_occupancy_device(e._h, ctypes.byref(oc), outside) == code
    assert (out == 3).all()  # nothing was written
    # the previous stack and the previous world are intact
    assert e.debug_get("map_layers") == 2 and e.debug_get("world_cells") == 2500
    for k in range(2):
        d, *geo = e.get_map_layer(k)
        assert same(d, before[k][0]) and tuple(geo) == tuple(before[k][1:])
    got = e.rasterize_scene_batch([[], []], prev_rings, sx, sy, res, use_world=True)
    assert same(got, ref_images([[], []], prev_rings, sx, sy, res, None, world=(world, 0.25, (0.0, 0.0), 1)))
    assert same(e.get_map_layer(1)[0], edt_ref.distance_map(got[1], res))
    e.close()


@pytest.mark.gpu
def test_a_scene_without_rings_and_without_world_gives_the_bytes_of_rasterize_batch():
    sx, sy, res = 257, 129, 0.2
    lay = small_lists(6, sx, sy, res, POS5)
    base = (np.random.default_rng(3).random((sx, sy)) >= 0.05).astype(np.uint8)
    e = binding.Engine(0)
    e.set_world_occupancy(np.zeros((8, 8), dtype=np.uint8), 100.0)  # a world that would occupy every cell: present on the handle, not asked for
    plain = e.rasterize_batch(lay, sx, sy, res, POS5, base=base)
    assert same(e.rasterize_scene_batch(lay, None, sx, sy, res, POS5, base=base), plain)
    empty = (np.zeros((0, 2)), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), 0, None)
    assert same(e.rasterize_scene_batch(lay, empty, sx, sy, res, POS5, base=base), plain)
    assert 0 < (plain == 0).sum() < plain.size
    e.close()


@pytest.mark.gpu
def test_stack_from_a_scene_equals_the_stack_from_the_reference_images():
    sx, sy, res = 257, 129, 0.2
    lay = small_lists(11, sx, sy, res, POS5)
    rings = binding.pack_rings(*ring_cases(12, sx, sy, res, POS5)["shared+own"])
    world, wres, wpos = (np.random.default_rng(14).random((120, 90)) >= 0.1).astype(np.uint8), 0.5, (1.0, 1.0)
    images = ref_images(lay, rings, sx, sy, res, POS5, world=(world, wres, wpos, 0))
    a, b = binding.Engine(0), binding.Engine(0)
    a.set_world_occupancy(world, wres, wpos[0], wpos[1])
    a.set_map_stack_scene(lay, rings, sx, sy, res, POS5, use_world=True)
    b.set_map_stack_occupancy(images, res, POS5)
    assert a.debug_get("map_layers") == M5 == b.debug_get("map_layers")
    for k in range(M5):
        da, *ga = a.get_map_layer(k)
        db, *gb = b.get_map_layer(k)
        assert same(da, db) and ga == gb == [res, POS5[k, 0], POS5[k, 1]], k
    a.close(); b.close()


SEEDS = (11, 12, 13)
B, M = 18, 3
LAYER_OF = np.arange(B, dtype=np.int32) % M


@pytest.mark.gpu
def test_plan_batch_end_to_end_with_a_corridor_ring_and_a_world_grid():
    """The three planning scenes of tests/test_map_stack.py from their disc lists, a FREE corridor ring in one layer and a world grid under all three."""
    sc = [synth.make_planning_scenes(seed, 6, near=(2 if seed == 13 else 0), map_kw=dict(size_x=420, size_y=380, pos=(3.0 * i, -2.0 * i))) for i, seed in enumerate(SEEDS)]
    inp = {k: np.stack([sc[b % M][k][b // M] for b in range(B)]) for k in ("way_x", "way_y", "start", "goal")}
    res = sc[0]["map"][1]
    pos = np.array([[s["map"][2], s["map"][3]] for s in sc])
    lay = [[binding.obstacle_disc(*d) for d in s["discs"]] for s in sc]
    # layer 1: everything farther than 3.2 m from the polyline through the first instance's waypoints is not drivable
    wx, wy = sc[1]["way_x"][0], sc[1]["way_y"][0]
    tx, ty = np.gradient(wx), np.gradient(wy)
    nrm = np.hypot(tx, ty)
    left = np.stack([wx - 3.2 * ty / nrm, wy + 3.2 * tx / nrm], axis=1)
    right = np.stack([wx + 3.2 * ty / nrm, wy - 3.2 * tx / nrm], axis=1)
    corridor = np.concatenate([left, right[::-1]])
    rings = binding.pack_rings([], [[], [(corridor, FREE)], []])
    world = np.full((300, 300), 255, dtype=np.uint8)
    world[:, 78:81] = 0  # a wall across the site, 33.5 .. 35 m north of its centre: inside every layer
    wres, wpos = 0.5, (0.0, 0.0)
    images = ref_images(lay, rings, 420, 380, res, pos, world=(world, wres, wpos, 0))
    plan = lambda eng: eng.plan_batch(inp["way_x"], inp["way_y"], inp["start"], inp["goal"], N=512)
    ref = binding.Engine(0)
    ref.set_map_stack_occupancy(images, res, pos)
    ref.set_map_assignment(LAYER_OF)
    want = plan(ref)
    ref.close()
    e = binding.Engine(0)
    e.set_world_occupancy(world, wres, wpos[0], wpos[1])
    e.set_map_stack_scene(lay, rings, 420, 380, res, pos, use_world=True)
    e.set_map_assignment(LAYER_OF)
    got = plan(e)
    e.set_map_stack_scene(lay, None, 420, 380, res, pos, use_world=True)  # the same call without the ring (same M: the assignment stays)
    no_ring = plan(e)
    e.close()
    for name, g, w in zip(("states", "n_states", "ok", "stage", "info"), got, want):
        assert same(g, w), name
    differs = np.array([not all(same(g[b], w[b]) for g, w in zip(got, no_ring)) for b in range(B)])
    assert differs[LAYER_OF == 1].any() and not differs[LAYER_OF != 1].any()


def _one_state_paths(n_inst):
    """n_inst paths of two states at the map's centre, solved: the collision check keeps them or not, depending on the layer each instance reads."""
    states = np.zeros((n_inst, 2, 5)); states[:, 1, 0] = 0.1; states[:, 1, 4] = 0.1
    info = np.zeros(n_inst, dtype=abi.INFO_DTYPE); info["status"] = 1
    return states, info


@pytest.mark.gpu
def test_handle_contract_of_the_scene_entries():
    import torch

    sx, sy, res = 128, 128, 0.25
    blocked, free = [(SQUARE * 3, SOLID)], [(SQUARE * 12, FREE)]
    states, info = _one_state_paths(2)
    e = binding.Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = lambda layers: _to_device(*binding.pack_obstacles([[] for _ in layers]), binding.pack_rings([], layers))[:3]
    o1, f1, r1 = dev([free, blocked])
    o2, f2, r2 = dev([blocked, free])
    torch.cuda.synchronize()
    with pytest.raises(binding.PoError):
        e.set_map_stack_scene_device(o1, f1, r1, sx, sy, res, use_world=True)  # no world on the handle
    assert e.debug_get("map_layers") == 0
    e.set_map_stack_scene_device(o1, f1, r1, sx, sy, res)
    e.set_map_assignment(np.array([1, 0], dtype=np.int32))
    p1 = e.debug_get("map_ptr")
    assert e.postcheck_batch(states, info)[0].tolist() == [0, 2]  # instance 0 reads layer 1 (blocked), instance 1 layer 0 (free)
    # a same-shape refresh through the device entry: the layers are rebuilt where they were and the assignment stays
    e.set_map_stack_scene_device(o2, f2, r2, sx, sy, res)
    assert e.debug_get("map_ptr") == p1 != 0 and e.debug_get("map_layers") == 2
    assert e.postcheck_batch(states, info)[0].tolist() == [2, 0]
    # a world arrives, then grows: the refresh reads the new one
    for wsize in (40, 400):
        world = np.full((wsize, wsize), 255, dtype=np.uint8)
        world[wsize // 2 - 2:wsize // 2 + 2, wsize // 2 - 2:wsize // 2 + 2] = 0
        e.set_world_occupancy_device(torch.from_numpy(np.ascontiguousarray(world.T)).cuda(), 0.5, 0.0, 0.0, outside_occupied=False)
        assert e.debug_get("world_cells") == wsize * wsize
        e.set_map_stack_scene_device(o2, f2, r2, sx, sy, res, use_world=True)
        assert e.debug_get("map_ptr") == p1
        want = ref_images([[], []], binding.pack_rings([], [blocked, free]), sx, sy, res, None, world=(world, 0.5, (0.0, 0.0), 0))
        for k in range(2):
            assert same(e.get_map_layer(k)[0], edt_ref.distance_map(want[k], res)), (wsize, k)
    # a larger M, then a larger size: the blocks grow (behind a synchronisation) and the layers are the right ones; the change of M drops the table
    layers3 = [blocked, free, [(L_RING * 4 - 2.0, SOLID)]]
    o3, f3, r3 = dev(layers3)
    s3, i3 = _one_state_paths(3)
    torch.cuda.synchronize()
    e.set_map_stack_scene_device(o3, f3, r3, sx, sy, res)
    assert e.debug_get("map_layers") == 3 and e.postcheck_batch(s3, i3)[0].tolist() == [0, 0, 0]  # no table: every instance reads layer 0
    bx, by = 200, 150
    e.set_map_stack_scene_device(o3, f3, r3, bx, by, res)
    big = ref_images([[], [], []], binding.pack_rings([], layers3), bx, by, res, None)
    for k in range(3):
        d, *geo = e.get_map_layer(k)
        assert d.shape == (bx, by) and same(d, edt_ref.distance_map(big[k], res)), k
    e.set_stream(None)
    e.close()
