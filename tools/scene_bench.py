"""Measurement (GPU): what it costs to fill the map stack from scenes — obstacle lists, polygon rings and a world grid.

Shape: M = 1, 64, 512 layers of 495 x 497 cells (resolution 0.2) at scattered centres over a 2048 x 2048 world of the same resolution; one shared 200-vertex FREE
ring around the site, two 12-vertex SOLID rings and 60 discs per layer (seeded).  Median of --reps timed calls after --warmup calls (the method of
tools/raster_bench.py, whose helpers this tool uses):
  (a) the route without the device rasteriser: numpy on one core — discs on their bounding windows, every ring edge on the rows it straddles inside the ring's
      bounding window, the world gathered through the definition's index arithmetic — + Engine.set_map_stack_occupancy of the M images; the two parts separately
  (b) Engine.set_map_stack_scene, host entry end to end (synchronous)
  (c) the device entries, events on the stream the handle enqueues on: set_map_stack_scene_device, and its two parts on the same data — rasterize_scene_batch_device
      alone (po_raster.hip's launch + the overlay launch) and set_map_stack_occupancy_device of the images it wrote; rasterize_batch_device alone for the overlay's share.
Every layer of every route is compared bitwise with route (a)'s in the run.  Numbers go to --out (default profiles/scene/scene_bench.json) and to stdout as one JSON line.
    python tools/scene_bench.py [--reps 30] [--warmup 5] [--out FILE] [--layers 1,64,512]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from raster_bench import N_DISCS, RES, SX, SY, event_ms, median_ms  # noqa: E402

WORLD, SOLID, FREE = 2048, 0, 1


def make_scene(M, seed=20):
    """centres [M, 2], discs [M, 60, 3], the shared FREE ring [200, 2], SOLID rings [M, 2, 12, 2], the world image [WORLD, WORLD] (0 = occupied)."""
    rng = np.random.default_rng(seed)
    lx, ly = SX * RES, SY * RES
    pos = rng.uniform(-110.0, 110.0, (M, 2))
    discs = np.stack([pos[:, :1] + rng.uniform(-0.45 * lx, 0.45 * lx, (M, N_DISCS)), pos[:, 1:] + rng.uniform(-0.45 * ly, 0.45 * ly, (M, N_DISCS)),
                      rng.uniform(0.5, 2.0, (M, N_DISCS))], axis=2)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 200))
    rad = rng.uniform(115.0, 175.0, 200)
    area = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    a12 = np.linspace(0, 2 * np.pi, 12, endpoint=False)
    blobs = np.empty((M, 2, 12, 2))
    for k in range(M):
        for b in range(2):
            r = rng.uniform(2.0, 7.0, 12)
            c = pos[k] + rng.uniform(-0.4, 0.4, 2) * (lx, ly)
            blobs[k, b] = np.stack([c[0] + r * np.cos(a12), c[1] + r * np.sin(a12)], axis=1)
    world = np.full((WORLD, WORLD), 255, dtype=np.uint8)
    for _ in range(3000):  # static clutter: small blocks
        i, j, w, h = rng.integers(0, WORLD - 12), rng.integers(0, WORLD - 12), rng.integers(2, 12), rng.integers(2, 12)
        world[i:i + w, j:j + h] = 0
    return pos, discs, area, blobs, world


def _ring_window(out, cx, cy, xy, solid):
    """Even-odd containment of ring xy on its bounding window: every edge on the rows it straddles.  solid: contained cells of `out` become 0; else returns the
    contained mask of the whole layer."""
    i0, i1 = np.searchsorted(-cx, -xy[:, 0].max()), np.searchsorted(-cx, -xy[:, 0].min(), side="right")
    j0, j1 = np.searchsorted(-cy, -xy[:, 1].max()), np.searchsorted(-cy, -xy[:, 1].min(), side="right")
    par = np.zeros((i1 - i0, j1 - j0), dtype=bool)
    X, Y = cx[i0:i1, None], cy[j0:j1]
    for e in range(len(xy)):
        (ax, ay), (bx, by) = xy[e], xy[(e + 1) % len(xy)]
        rows = np.nonzero((ay > Y) != (by > Y))[0]
        if len(rows) == 0 or i0 == i1:
            continue
        y = Y[None, rows]
        t = (bx - ax) * (y - ay) - (by - ay) * (X - ax)
        par[:, rows] ^= (t > 0) if by > ay else (t < 0)
    if solid:
        out[i0:i1, j0:j1][par] = 0
        return None
    full = np.zeros(out.shape, dtype=bool)
    full[i0:i1, j0:j1] = par
    return full


def numpy_rasterize(pos, discs, area, blobs, world):
    """uint8 [M, SX, SY] (0 = occupied), the definition of include/po_hip.h evaluated on windows."""
    M = len(pos)
    out = np.full((M, SY, SX), 255, dtype=np.uint8).transpose(0, 2, 1)  # (stored [M][size_y][size_x]: handed to the library without a transposing copy)
    wl = WORLD * RES
    for k in range(M):
        cx = (pos[k, 0] + (0.5 * (SX * RES) - 0.5 * RES)) + RES * (-np.arange(SX)).astype(np.float64)
        cy = (pos[k, 1] + (0.5 * (SY * RES) - 0.5 * RES)) + RES * (-np.arange(SY)).astype(np.float64)
        o = out[k]
        # world (centre (0, 0), outside = free)
        tx, ty = -((cx - 0.0) - 0.5 * wl), -((cy - 0.0) - 0.5 * wl)
        ix, iy = (-(((cx - 0.5 * wl) - 0.0) / RES)).astype(np.int64), (-(((cy - 0.5 * wl) - 0.0) / RES)).astype(np.int64)
        okx, oky = (tx >= 0) & (tx < wl) & (ix >= 0) & (ix < WORLD), (ty >= 0) & (ty < wl) & (iy >= 0) & (iy < WORLD)
        sub = world[np.ix_(ix[okx], iy[oky])]
        o[np.ix_(okx, oky)] = np.where(sub == 0, 0, 255)
        for x, y, r in discs[k]:
            i0, i1 = max(int((cx[0] - x - r) / RES) - 2, 0), min(int((cx[0] - x + r) / RES) + 3, SX)
            j0, j1 = max(int((cy[0] - y - r) / RES) - 2, 0), min(int((cy[0] - y + r) / RES) + 3, SY)
            if i0 >= i1 or j0 >= j1:
                continue
            dx, dy = cx[i0:i1, None] - x, cy[None, j0:j1] - y
            o[i0:i1, j0:j1][dx * dx + dy * dy <= r * r] = 0
        for b in blobs[k]:
            _ring_window(o, cx, cy, b, True)
        o[~_ring_window(o, cx, cy, area, False)] = 0
    return out


def measure(binding, torch, M, reps, warmup):
    pos, discs, area, blobs, world = make_scene(M)
    lay = binding.pack_obstacles([[binding.obstacle_disc(*d) for d in layer] for layer in discs])
    rings = binding.pack_rings([(area, FREE)], [[(b, SOLID) for b in blobs[k]] for k in range(M)])
    row = {"M": M, "ring_vertices": int(len(rings[0])), "table_bytes": int(lay[0].nbytes + lay[1].nbytes + rings[0].nbytes + rings[1].nbytes + rings[2].nbytes + rings[4].nbytes),
           "image_bytes": int(M * SX * SY)}
    eng = binding.Engine(0)
    eng.set_world_occupancy(world, RES, 0.0, 0.0, outside_occupied=False)
    img = {}

    def host_raster():
        img["occ"] = numpy_rasterize(pos, discs, area, blobs, world)

    a1_reps, a1_warm = (3, 0) if M > 64 else (max(5, reps // 4), 1)  # (seconds per call at M = 512: fewer calls, stated in the row)
    a2_reps, a2_warm = (max(10, reps // 3), 2) if M > 64 else (reps, warmup)
    a1 = median_ms(host_raster, a1_reps, a1_warm)
    a2 = median_ms(lambda: eng.set_map_stack_occupancy(img["occ"], RES, pos), a2_reps, a2_warm)
    row["a_numpy_rasterize_ms"] = dict(a1, what="numpy, one core, windows", reps=a1_reps, warmup=a1_warm)
    row["a_set_map_stack_occupancy_ms"] = dict(a2, what="host entry: M images of 1 byte per cell over PCIe, the transform, synchronous", reps=a2_reps, warmup=a2_warm)
    row["a_total_ms"] = a1["median"] + a2["median"]
    row["reps"], row["warmup"] = reps, warmup  # every other interval of the row
    want = [eng.get_map_layer(k)[0] for k in range(M)]  # EVERY layer of route (a); the other routes are compared with all of them
    row["layers_compared"] = M
    equal = lambda: bool(all(np.array_equal(eng.get_map_layer(k)[0].view(np.uint32), w.view(np.uint32)) for k, w in enumerate(want)))

    b = median_ms(lambda: eng.set_map_stack_scene(lay, rings, SX, SY, RES, pos, use_world=True), reps, warmup)
    row["b_set_map_stack_scene_ms"] = dict(b, what="host entry end to end: tables over PCIe, rasteriser + overlay + transform, synchronous")
    row["b_layers_equal_a_bitwise"] = equal()
    row["b_over_a"] = b["median"] / row["a_total_ms"]

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_obs, d_first = torch.from_numpy(lay[0].view(np.uint8).reshape(-1, 136).copy()).cuda(), t(lay[1])
    d_rings = (t(rings[0]), t(rings[1]), t(rings[2]), rings[3], t(rings[4]))
    d_pos = t(pos)
    stream = torch.cuda.Stream()  # (a stream of its own: the default stream's handle is NULL, which po_set_stream reads as "the handle's own stream")
    eng.set_stream(stream.cuda_stream)
    cells = torch.zeros((M, SY, SX), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ev = lambda fn: event_ms(torch, stream, fn, reps, warmup)
    row["c_set_map_stack_scene_device_ms"] = dict(ev(lambda: eng.set_map_stack_scene_device(d_obs, d_first, d_rings, SX, SY, RES, d_pos, use_world=True)),
                                                  what="events around one call: rasteriser, overlay and the two transform launches")
    row["c_layers_equal_a_bitwise"] = equal()
    row["c_rasterize_batch_device_ms"] = dict(ev(lambda: eng.rasterize_batch_device(d_obs, d_first, cells, RES, d_pos)), what="po_raster.hip's launch alone (discs)")
    row["c_rasterize_scene_batch_device_ms"] = dict(ev(lambda: eng.rasterize_scene_batch_device(d_obs, d_first, d_rings, cells, RES, d_pos, use_world=True)),
                                                    what="the scene rasteriser alone: po_raster.hip's launch + the overlay launch")
    row["c_set_map_stack_occupancy_device_ms"] = dict(ev(lambda: eng.set_map_stack_occupancy_device(cells, RES, d_pos)),
                                                      what="the transform pair alone, on the images the scene rasteriser wrote")
    row["c_layers_equal_a_bitwise_from_images"] = equal()
    row["c_scene_rasteriser_over_transform"] = row["c_rasterize_scene_batch_device_ms"]["median"] / row["c_set_map_stack_occupancy_device_ms"]["median"]
    eng.set_stream(None)
    eng.close()
    print(f"[scene_bench] M = {M}: (a) {a1['median']:.2f} + {a2['median']:.2f} ms  (b) {b['median']:.2f} ms  (c) scene raster "
          f"{row['c_rasterize_scene_batch_device_ms']['median'] * 1e3:.0f} us (discs alone {row['c_rasterize_batch_device_ms']['median'] * 1e3:.0f}), transform "
          f"{row['c_set_map_stack_occupancy_device_ms']['median'] * 1e3:.0f} us, all {row['c_set_map_stack_scene_device_ms']['median'] * 1e3:.0f} us; equal: "
          f"{row['b_layers_equal_a_bitwise']} {row['c_layers_equal_a_bitwise']} {row['c_layers_equal_a_bitwise_from_images']}", file=sys.stderr)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", default="1,64,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene", "scene_bench.json"))
    a = ap.parse_args()
    import torch

    from path_optimizer_amd import binding

    if not torch.cuda.is_available():
        raise SystemExit("scene_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    if a.reps < 20:
        raise SystemExit("scene_bench: at least 20 timed repetitions")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "size_x": SX, "size_y": SY, "resolution": RES, "world": [WORLD, WORLD],
           "discs_per_layer": N_DISCS, "layers": {str(M): measure(binding, torch, M, a.reps, a.warmup) for M in (int(v) for v in a.layers.split(","))}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
