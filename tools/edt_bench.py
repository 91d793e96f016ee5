"""Measurement (GPU): what it costs to get a usable obstacle-distance map into a handle, from an occupancy image — the stage in front of po_plan_batch.

On the benchmark scene's 495 x 497 image (tests/golden/benchmark_scene.npz) and on a synthetic 2048 x 2048 one (seeded), median of --reps timed repetitions after warm-up:
  (a) the route without the device transform: scipy.ndimage.distance_transform_edt on one core (standing in for cv::distanceTransform) + Engine.set_map of the float
      layer; the two parts separately (perf_counter; set_map is synchronous)
  (b) Engine.set_map_occupancy, host entry end to end (perf_counter; synchronous: upload of 1 byte per cell, the two kernels, stream synchronise)
  (c) Engine.set_map_occupancy_device: device interval only (events on the stream the handle enqueues on), per call and as a train of back-to-back calls, and the
      kernels' achieved bytes/s against the compulsory 5 bytes per cell (1 read + 4 written)
  (d) for scale, plan_batch on one instance of the benchmark scene (bench.py's c1_real_scene: eps 1e-3, host pointers in and out), same run
Nothing is asserted: numbers go to --out (default profiles/edt/edt_bench.json) and to stdout as one JSON line.
    python tools/edt_bench.py [--reps 30] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_occupancy(n=2048, seed=2048):
    """A parking-lot-like image: free space, a 0.5 % sprinkle of occupied cells and forty occupied rectangles.  uint8 [n, n], 0 = occupied."""
    rng = np.random.default_rng(seed)
    occ = np.full((n, n), 255, dtype=np.uint8)
    occ[rng.random((n, n)) < 0.005] = 0
    for _ in range(40):
        i, j, h, w = rng.integers(0, n - 80), rng.integers(0, n - 80), rng.integers(8, 80), rng.integers(8, 80)
        occ[i:i + h, j:j + w] = 0
    occ[700:1300, 500:1400] = 255  # one open area some hundred cells across
    return occ


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def measure_image(binding, torch, name, occ, res, reps, warmup):
    from scipy import ndimage

    sx, sy = occ.shape
    cells = sx * sy
    row = {"size_x": sx, "size_y": sy, "cells": cells, "occupied_cells": int((occ == 0).sum())}
    free = occ != 0
    layer = {}

    def host_transform():
        layer["d"] = ndimage.distance_transform_edt(free).astype(np.float32) * np.float32(res)

    eng = binding.Engine(0)
    a1 = median_ms(host_transform, max(5, reps // 4), 1)
    # both host entries get their array in the library's own layout (x contiguous = Fortran order of [size_x, size_y]), as a C++ caller's Eigen matrix is: the timed
    # calls then hand the buffer over as it is (numpy's transposing copy is not part of either route)
    layer_f, occ = np.asfortranarray(layer["d"]), np.asfortranarray(occ)
    a2 = median_ms(lambda: eng.set_map(layer_f, res, 0.0, 0.0), reps, warmup)
    row["a_host_transform_ms"] = {"median": a1[0], "min": a1[1], "max": a1[2], "what": "scipy.ndimage.distance_transform_edt + float32 scale, one core"}
    row["a_set_map_ms"] = {"median": a2[0], "min": a2[1], "max": a2[2], "what": "Engine.set_map of the float layer (4 bytes per cell, synchronous)"}
    row["a_total_ms"] = a1[0] + a2[0]
    want = eng.get_map()[0]

    b = median_ms(lambda: eng.set_map_occupancy(occ, res, 0.0, 0.0), reps, warmup)
    row["b_set_map_occupancy_ms"] = {"median": b[0], "min": b[1], "max": b[2], "what": "Engine.set_map_occupancy, host entry end to end (1 byte per cell, synchronous)"}
    row["b_layer_equals_a_bitwise"] = bool(np.array_equal(eng.get_map()[0].view(np.uint32), want.view(np.uint32)))

    # (c): the handle enqueues on a torch stream, so torch events recorded on that stream bracket exactly its launches
    stream = torch.cuda.Stream()  # (a stream of its own: the default stream's handle is NULL, which po_set_stream reads as "the handle's own stream")
    eng.set_stream(stream.cuda_stream)
    img = torch.from_numpy(occ.T).cuda().t()  # (occ is in Fortran order: its transpose is the contiguous [size_y, size_x] image)
    for _ in range(warmup):
        eng.set_map_occupancy_device(img, res, 0.0, 0.0)
    torch.cuda.synchronize()
    single = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        eng.set_map_occupancy_device(img, res, 0.0, 0.0)
        e1.record(stream)
        e1.synchronize()
        single.append(e0.elapsed_time(e1))
    train, T = [], 20
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(T):
            eng.set_map_occupancy_device(img, res, 0.0, 0.0)
        e1.record(stream)
        e1.synchronize()
        train.append(e0.elapsed_time(e1) / T)
    c1, c2 = float(np.median(single)), float(np.median(train))
    row["c_device_interval_ms"] = {"median": c1, "min": float(np.min(single)), "max": float(np.max(single)), "what": "events around ONE set_map_occupancy_device (two launches)"}
    row["c_device_interval_in_a_train_ms"] = {"median": c2, "min": float(np.min(train)), "max": float(np.max(train)), "what": f"events around {T} calls back to back, per call"}
    row["c_compulsory_bytes"] = 5 * cells
    row["c_achieved_GBps_of_compulsory_bytes"] = {"single": 5 * cells / (c1 * 1e-3) / 1e9, "train": 5 * cells / (c2 * 1e-3) / 1e9}
    row["c_layer_equals_a_bitwise"] = bool(np.array_equal(eng.get_map()[0].view(np.uint32), want.view(np.uint32)))
    eng.set_stream(None)
    eng.close()
    print(f"[edt_bench] {name}: (a) {a1[0]:.3f} + {a2[0]:.3f} ms  (b) {b[0]:.3f} ms  (c) {c1 * 1e3:.1f} us single, {c2 * 1e3:.1f} us in a train", file=sys.stderr)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt", "edt_bench.json"))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("edt_bench: at least 20 timed repetitions")
    import torch

    from path_optimizer_amd import binding

    if not torch.cuda.is_available():
        raise SystemExit("edt_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    g = np.load(os.path.join(ROOT, "tests", "golden", "benchmark_scene.npz"))
    res = float(g["resolution"])
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "images": {}}
    out["images"]["benchmark_scene_495x497"] = measure_image(binding, torch, "495 x 497", (g["distance"] != 0).astype(np.uint8), res, a.reps, a.warmup)
    out["images"]["synthetic_2048x2048"] = measure_image(binding, torch, "2048 x 2048", synthetic_occupancy(), res, a.reps, a.warmup)
    # (d) bench.py's c1_real_scene: plan_batch on one instance, eps 1e-3, host pointers in and out — here on a map installed from the occupancy image
    p = binding.default_params()
    p.eps_abs = p.eps_rel = 1e-3
    eng = binding.Engine(0, p)
    eng.set_map_occupancy((g["distance"] != 0).astype(np.uint8), res, float(g["pos"][0]), float(g["pos"][1]))
    args = (g["way_x"][None], g["way_y"][None], g["start"][None], g["goal"][None])
    d = median_ms(lambda: eng.plan_batch(*args, N=512), a.reps, a.warmup)
    states, n, ok, stage, info = eng.plan_batch(*args, N=512)
    eng.close()
    out["d_c1_real_scene_plan_batch_ms"] = {"median": d[0], "min": d[1], "max": d[2], "ok": int(ok[0]), "states": int(n[0]),
                                            "max_abs_diff_vs_reference": float(np.abs(states[0, :n[0]] - g["path1_e3"]).max()) if n[0] == len(g["path1_e3"]) else None}
    s = out["images"]["benchmark_scene_495x497"]
    out["summary_495x497"] = {"a_ms": s["a_total_ms"], "b_ms": s["b_set_map_occupancy_ms"]["median"], "c_ms": s["c_device_interval_ms"]["median"], "d_ms": d[0],
                              "c_over_d": s["c_device_interval_ms"]["median"] / d[0]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
