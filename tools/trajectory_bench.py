"""Measurement (GPU): what the timed-trajectory stage costs behind po_plan_batch and po_speed_batch.

Shape: tools/select_bench.py's — 512 groups x 8 candidates = 4 096 planning instances from the 64 seeded scenes, one map, N = 320 rows per path.
po_plan_batch_device produces the paths and po_speed_batch_device (start speed 5 m/s, end speed 0, use_map = 0) their v and t once.  Then, on a stream of its
own with hipEvents around each call, --warmup calls of every variant and then --reps ROUNDS, each round timing every variant once (the variants alternate, so a
drift of the clock or a neighbour on the machine falls on all of them alike); the median, minimum and maximum over the rounds:
  trajectory K x D   po_trajectory_batch_device alone on the 4 096 paths, every output asked for, a horizon of 5 s (dt = 5 / K) from t0 = 0, for K = 50 and
                     K = 200 samples and D = 0 and D = 4 discs (the covering circles, 8 points each, the stride at its limit)
  speed              po_speed_batch_device on the same paths, t and total_time asked for: the stage of the same nature (a sweep over every row of every path)
and, outside the rounds because it blocks mid-way, plan: po_plan_batch_device of the 4 096 instances.  bytes_min is what the stage has to move, computed from the
shapes: the seven doubles of every row below n of the paths it samples, the outputs of all B paths; GB/s is that over the median.  Nothing is asserted and no
threshold is set: numbers go to --out (default profiles/trajectory/trajectory_bench.json) and to stdout as one JSON line.
    python tools/trajectory_bench.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HORIZON_S = 5.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory", "trajectory_bench.json"))
    a = ap.parse_args()
    import torch

    import select_bench
    from path_optimizer_amd import binding, synth
    from path_optimizer_amd.abi import INFO_BYTES

    if not torch.cuda.is_available():
        raise SystemExit("trajectory_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    if a.reps < 20:
        raise SystemExit("trajectory_bench: at least 20 timed repetitions")
    G, PER, N = select_bench.G, select_bench.PER, select_bench.N
    B = G * PER
    t_host, the_map = select_bench.candidates(synth)
    way_len = float(np.hypot(np.diff(t_host["way_x"], axis=1), np.diff(t_host["way_y"], axis=1)).sum(axis=1).max())
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    t = {k: dev(v) for k, v in t_host.items()}
    plan = dict(states=f64(B, N, 5), n_states=i32(B), ok=i32(B), stage=i32(B), info=torch.zeros((B, INFO_BYTES), dtype=torch.uint8, device="cuda"))
    stream = torch.cuda.Stream()  # (a stream of its own: the default stream's handle is NULL, which po_set_stream reads as "the handle's own stream")
    eng = binding.Engine(0)
    eng.set_map(*the_map)
    eng.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    row = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "groups": G, "candidates_per_group": PER, "B": B, "N": N, "horizon_s": HORIZON_S}
    row["plan_ms"] = dict(select_bench.event_ms(torch, stream, lambda: eng.plan_batch_device(t, plan, N, way_len), a.reps, a.warmup), what="po_plan_batch_device, 4 096 instances")
    sp = binding.default_speed_params()
    spd_in = dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], v0=torch.full((B,), 5.0, dtype=torch.float64, device="cuda"), v_end=f64(B))
    spd = dict(v=f64(B, N), a=f64(B, N), t=f64(B, N), total_time=f64(B), status=i32(B))
    eng.speed_batch_device(spd_in, spd, sp)
    torch.cuda.synchronize()
    n_states, ok = plan["n_states"].cpu().numpy(), plan["ok"].cpu().numpy()
    row["plan_ok"] = int(ok.sum()); row["mean_states"] = float(n_states[ok != 0].mean()) if ok.any() else 0.0
    total_time = spd["total_time"].cpu().numpy()
    row["mean_total_time_s"] = float(total_time[ok != 0].mean()) if ok.any() else 0.0

    off, rad = binding.covering_discs(binding.default_params())
    tr_in = dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], v=spd["v"], t=spd["t"])
    variants = {"speed": (lambda: eng.speed_batch_device(spd_in, spd, sp))}
    rows = []
    for K in (50, 200):
        for D in (0, 4):
            tp = binding.default_trajectory_params()
            tp.t0, tp.dt, tp.K, tp.n_discs, tp.agent_pts, tp.agent_stride = 0.0, HORIZON_S / K, K, D, 8, (K - 1) // 7
            for j in range(D):
                tp.disc_offset[j], tp.disc_radius[j] = off[j], rad
            out = dict(status=i32(B), states=f64(B, K, 5), v=f64(B, K), a=f64(B, K), t=f64(B, K), index=i32(B, K), first_held=i32(B))
            if D:
                out["agents"] = torch.zeros(B * D * binding.AGENT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            name = f"trajectory_K{K}_D{D}"
            variants[name] = (lambda tp=tp, out=out: eng.trajectory_batch_device(tr_in, out, tp))
            rows.append({"name": name, "K": K, "n_discs": D, "agent_pts": 8, "agent_stride": int(tp.agent_stride), "dt": float(tp.dt), "out": out})
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(a.reps):  # one round: every variant once
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    row["speed_ms"] = dict(stat(ts["speed"]), what="po_speed_batch_device, 4 096 paths, use_map = 0, both launches, in the same rounds")
    for r in rows:
        out = r.pop("out")
        status = out["status"].cpu().numpy()
        r["trajectory_ms"] = dict(stat(ts[r["name"]]), what="po_trajectory_batch_device, 4 096 paths, every output")
        r["status"] = {str(k): int((status == k).sum()) for k in (0, 1, 2, 3)}
        r["bytes_min"] = int(7 * 8 * int(n_states[status > 0].sum()) + B * (r["K"] * (8 * 8 + 4) + 8 + r["n_discs"] * binding.AGENT_DTYPE.itemsize))
        r["GB_per_s"] = r["bytes_min"] / (r["trajectory_ms"]["median"] * 1e-3) / 1e9
        r["trajectory_over_speed"] = r["trajectory_ms"]["median"] / row["speed_ms"]["median"]
        r["trajectory_over_plan"] = r["trajectory_ms"]["median"] / row["plan_ms"]["median"]
    row["rows"] = rows
    eng.set_stream(None)
    eng.close()
    for r in rows:
        print(f"[trajectory_bench] K {r['K']} D {r['n_discs']}: {r['trajectory_ms']['median'] * 1e3:.0f} us ({r['GB_per_s']:.0f} GB/s of its minimum traffic), speed "
              f"{row['speed_ms']['median'] * 1e3:.0f} us, plan {row['plan_ms']['median']:.2f} ms, statuses {r['status']}", file=sys.stderr)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
