"""Measurement (GPU): what it costs to fill the map stack from per-layer obstacle lists — the step in front of po_plan_batch.

Shape: 495 x 497 cells (the benchmark scene's size), resolution 0.2, 60 discs per layer (make_planning_scenes' density), M = 1, 64, 512 layers (seeded lists).
Median of --reps timed calls after --warmup calls (the method of tools/edt_bench.py):
  (a) the route without the device rasteriser: numpy rasterisation on one core — each disc evaluated on its own bounding window only, the definition's predicate —
      + Engine.set_map_stack_occupancy of the M images (host entry: 1 byte per cell over PCIe); the two parts separately
  (b) Engine.set_map_stack_obstacles, host entry end to end (136 bytes per obstacle over PCIe; synchronous)
  (c) the device entries, events on the stream the handle enqueues on: set_map_stack_obstacles_device (rasteriser + transform), and its two parts on the same data —
      rasterize_batch_device alone and set_map_stack_occupancy_device of the images it wrote.
`--device-only M` issues --reps calls of set_map_stack_obstacles_device and nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the per-kernel
split (a run of its own; nothing is written).
Nothing is asserted: numbers go to --out (default profiles/raster/raster_bench.json) and to stdout as one JSON line.
    python tools/raster_bench.py [--reps 30] [--warmup 5] [--out FILE] [--device-only M]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SX, SY, RES, N_DISCS = 495, 497, 0.2, 60


def disc_lists(M, seed=18):
    """M x 60 discs (x, y, r) inside the map, radii 0.5 .. 2 m: float64 [M, 60, 3]."""
    rng = np.random.default_rng(seed)
    lx, ly = SX * RES, SY * RES
    return np.stack([rng.uniform(-0.45 * lx, 0.45 * lx, (M, N_DISCS)), rng.uniform(-0.45 * ly, 0.45 * ly, (M, N_DISCS)), rng.uniform(0.5, 2.0, (M, N_DISCS))], axis=2)


def numpy_rasterize(discs):
    """uint8 [M, SX, SY] (0 = occupied): every disc on its bounding window (two cells of margin), the predicate of include/po_hip.h."""
    cx = (0.5 * (SX * RES) - 0.5 * RES) + RES * (-np.arange(SX)).astype(np.float64)
    cy = (0.5 * (SY * RES) - 0.5 * RES) + RES * (-np.arange(SY)).astype(np.float64)
    # (indexed [k, i, j], stored [M][size_y][size_x] like the library's images: the timed set_map_stack_occupancy then hands the buffer over without a transposing copy)
    out = np.full((len(discs), SY, SX), 255, dtype=np.uint8).transpose(0, 2, 1)
    for k, layer in enumerate(discs):
        for x, y, r in layer:
            i0, i1 = max(int((cx[0] - x - r) / RES) - 2, 0), min(int((cx[0] - x + r) / RES) + 3, SX)
            j0, j1 = max(int((cy[0] - y - r) / RES) - 2, 0), min(int((cy[0] - y + r) / RES) + 3, SY)
            if i0 >= i1 or j0 >= j1:
                continue
            dx, dy = cx[i0:i1, None] - x, cy[None, j0:j1] - y
            out[k, i0:i1, j0:j1][dx * dx + dy * dy <= r * r] = 0
    return out


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def event_ms(torch, stream, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def device_lists(binding, torch, discs):
    obs, first = binding.pack_obstacles([[binding.obstacle_disc(*d) for d in layer] for layer in discs])
    return torch.from_numpy(obs.view(np.uint8).reshape(-1, 136).copy()).cuda(), torch.from_numpy(first).cuda(), (obs, first)


def measure(binding, torch, M, reps, warmup):
    discs = disc_lists(M)
    row = {"M": M, "obstacles": int(M * N_DISCS), "list_bytes": int(M * N_DISCS * 136 + 4 * (M + 1)), "image_bytes": int(M * SX * SY)}
    eng = binding.Engine(0)
    img = {}

    def host_raster():
        img["occ"] = numpy_rasterize(discs)

    a1 = median_ms(host_raster, 5 if M > 64 else max(5, reps // 4), 1)
    a2 = median_ms(lambda: eng.set_map_stack_occupancy(img["occ"], RES), reps if M <= 64 else max(10, reps // 3), warmup if M <= 64 else 2)
    row["a_numpy_rasterize_ms"] = dict(a1, what="numpy, one core, each disc on its bounding window")
    row["a_set_map_stack_occupancy_ms"] = dict(a2, what="host entry: M images of 1 byte per cell over PCIe, the transform, synchronous")
    row["a_total_ms"] = a1["median"] + a2["median"]
    want = [eng.get_map_layer(k)[0] for k in (0, M - 1)]

    d_obs, d_first, packed = device_lists(binding, torch, discs)
    b = median_ms(lambda: eng.set_map_stack_obstacles(packed, SX, SY, RES), reps, warmup)
    row["b_set_map_stack_obstacles_ms"] = dict(b, what="host entry end to end: 136 bytes per obstacle over PCIe, rasteriser + transform, synchronous")
    row["b_layers_equal_a_bitwise"] = bool(all(np.array_equal(eng.get_map_layer(k)[0].view(np.uint32), w.view(np.uint32)) for k, w in zip((0, M - 1), want)))

    stream = torch.cuda.Stream()  # (a stream of its own: the default stream's handle is NULL, which po_set_stream reads as "the handle's own stream")
    eng.set_stream(stream.cuda_stream)
    cells = torch.zeros((M, SY, SX), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    row["c_set_map_stack_obstacles_device_ms"] = dict(event_ms(torch, stream, lambda: eng.set_map_stack_obstacles_device(d_obs, d_first, SX, SY, RES), reps, warmup),
                                                      what="events around one call: rasteriser + the two transform launches")
    row["c_rasterize_batch_device_ms"] = dict(event_ms(torch, stream, lambda: eng.rasterize_batch_device(d_obs, d_first, cells, RES), reps, warmup),
                                              what="events around the rasteriser alone (one launch)")
    row["c_set_map_stack_occupancy_device_ms"] = dict(event_ms(torch, stream, lambda: eng.set_map_stack_occupancy_device(cells, RES), reps, warmup),
                                                      what="events around the transform pair alone, on the images the rasteriser wrote")
    row["c_layers_equal_a_bitwise"] = bool(all(np.array_equal(eng.get_map_layer(k)[0].view(np.uint32), w.view(np.uint32)) for k, w in zip((0, M - 1), want)))
    row["c_rasteriser_over_transform"] = row["c_rasterize_batch_device_ms"]["median"] / row["c_set_map_stack_occupancy_device_ms"]["median"]
    row["b_over_a"] = b["median"] / row["a_total_ms"]
    eng.set_stream(None)
    eng.close()
    print(f"[raster_bench] M = {M}: (a) {a1['median']:.2f} + {a2['median']:.2f} ms  (b) {b['median']:.2f} ms  (c) raster {row['c_rasterize_batch_device_ms']['median'] * 1e3:.0f} us, "
          f"transform {row['c_set_map_stack_occupancy_device_ms']['median'] * 1e3:.0f} us, both {row['c_set_map_stack_obstacles_device_ms']['median'] * 1e3:.0f} us", file=sys.stderr)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster", "raster_bench.json"))
    ap.add_argument("--device-only", type=int, default=0, metavar="M")
    a = ap.parse_args()
    import torch

    from path_optimizer_amd import binding

    if not torch.cuda.is_available():
        raise SystemExit("raster_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    if a.device_only:
        eng = binding.Engine(0)
        d_obs, d_first, _ = device_lists(binding, torch, disc_lists(a.device_only))
        torch.cuda.synchronize()
        for _ in range(a.reps):
            eng.set_map_stack_obstacles_device(d_obs, d_first, SX, SY, RES)
        eng.get_map_layer(0)  # synchronises
        eng.close()
        return
    if a.reps < 20:
        raise SystemExit("raster_bench: at least 20 timed repetitions")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "size_x": SX, "size_y": SY, "resolution": RES, "discs_per_layer": N_DISCS,
           "layers": {str(M): measure(binding, torch, M, a.reps, a.warmup) for M in (1, 64, 512)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
