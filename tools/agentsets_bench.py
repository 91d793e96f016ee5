"""Measurement (GPU): what composing agent sets on the device costs, and what it saves the stage behind it.

Scene: 4 096 egos as 64 worlds x 64 vehicles.  Every vehicle drives N = 320 states 0.3 m apart on a gently curved path from a random pose in a 300 m square of
its world; po_speed_batch_device (start speed 5 m/s, use_map = 0) gives v and t, po_trajectory_batch_device (5 s at 10 Hz, D = 4 covering discs of 8 points)
the fleet's 16 384 records, and every world has 32 perception agents (discs on straight 5 s tracks).  reach = binding.footprint_reach at po_dynamic_batch's default
margin, owner_div = 4, pool_of = the world.  On a stream of its own with hipEvents around each call, --warmup calls of every variant and then --reps ROUNDS, each
round timing every variant once (the variants alternate, so a drift of the clock or a neighbour on the machine falls on all of them alike); the median, minimum
and maximum over the rounds:
  agentsets            po_agentsets_batch_device alone, every output, capacity = the total of a counting call
  agentsets_count      the counting call (capacity 0: no gather launch)
  dynamic_composed     po_dynamic_batch_device on the composed sets (out->agents, out->first, out->set_of)
  dynamic_everybody    po_dynamic_batch_device on everybody-but-me sets built on the host: per ego the 252 records of the other vehicles of its world and its 32
                       perception agents
  host_build_upload    wall clock, not events: the fleet's records copied to the host, the 4 096 sets gathered with a precomputed index, the result uploaded,
                       the stream synchronised — what a caller without this stage does every cycle
Nothing is asserted and no threshold is set: numbers go to --out (default profiles/agentsets/agentsets_bench.json) and to stdout as one JSON line.
    python tools/agentsets_bench.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORLDS, VEHICLES, N, D, SEEN, SQUARE_M, STEP_M = 64, 64, 320, 4, 32, 300.0, 0.3


def scene(binding):
    rng = np.random.default_rng(20)
    B = WORLDS * VEHICLES
    s = STEP_M * np.arange(N)
    states = np.zeros((B, N, 5))
    for b in range(B):
        k = rng.uniform(-0.01, 0.01)
        z = rng.uniform(-math.pi, math.pi) + k * s
        x = rng.uniform(0, SQUARE_M) + np.concatenate(([0.0], np.cumsum(STEP_M * np.cos(z[:-1]))))
        y = rng.uniform(0, SQUARE_M) + np.concatenate(([0.0], np.cumsum(STEP_M * np.sin(z[:-1]))))
        states[b] = np.stack([x, y, z, np.full(N, k), s], axis=1)
    seen = np.zeros(WORLDS * SEEN, dtype=binding.AGENT_DTYPE)
    for g in seen:
        x0, y0, h, v = rng.uniform(0, SQUARE_M), rng.uniform(0, SQUARE_M), rng.uniform(-math.pi, math.pi), rng.uniform(0, 8)
        g["n_pts"], g["flags"], g["radius"] = 8, 2, rng.uniform(0.3, 1.5)
        g["t"] = np.linspace(0.0, 5.0, 8)
        g["x"], g["y"] = x0 + v * g["t"] * math.cos(h), y0 + v * g["t"] * math.sin(h)
    return states, seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agentsets", "agentsets_bench.json"))
    a = ap.parse_args()
    import torch

    from path_optimizer_amd import binding

    if not torch.cuda.is_available():
        raise SystemExit("agentsets_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    if a.reps < 20:
        raise SystemExit("agentsets_bench: at least 20 timed repetitions")
    B, REC = WORLDS * VEHICLES, binding.AGENT_DTYPE.itemsize
    states_h, seen_h = scene(binding)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()  # (a stream of its own: the default stream's handle is NULL, which po_set_stream reads as "the handle's own stream")
    eng = binding.Engine(0)  # no map: none of these stages reads one
    eng.set_stream(stream.cuda_stream)
    states = dev(states_h)
    sp = binding.default_speed_params()
    spd = dict(v=f64(B, N), a=f64(B, N), t=f64(B, N), total_time=f64(B), status=i32(B))
    eng.speed_batch_device(dict(states=states, v0=torch.full((B,), 5.0, dtype=torch.float64, device="cuda")), spd, sp)
    off, rad = binding.covering_discs(binding.default_params())
    tp = binding.default_trajectory_params()
    tp.n_discs = D
    for j in range(D):
        tp.disc_offset[j], tp.disc_radius[j] = off[j], rad
    K = int(tp.K)
    tr = dict(status=i32(B), states=f64(B, K, 5), agents=u8(B * D * REC))
    eng.trajectory_batch_device(dict(states=states, v=spd["v"], t=spd["t"]), tr, tp)
    dp = binding.default_dynamic_params()
    sets_p = binding.default_agentsets_params()
    sets_p.reach, sets_p.owner_div = binding.footprint_reach(binding.default_params(), dp.margin), D
    pool_of_h = (np.arange(B) // VEHICLES).astype(np.int32)
    sets_in = dict(states=states, t=spd["t"], agents=tr["agents"], first=dev((np.arange(WORLDS + 1) * VEHICLES * D).astype(np.int32)), pool_of=dev(pool_of_h),
                   agents1=dev(seen_h.view(np.uint8)), first1=dev((np.arange(WORLDS + 1) * SEEN).astype(np.int32)))
    count_out = dict(first=i32(B + 1), count=i32(B), status=i32(B), total=torch.zeros(1, dtype=torch.int64, device="cuda"))
    eng.agentsets_batch_device(sets_in, count_out, sets_p)
    torch.cuda.synchronize()
    total = int(count_out["total"].cpu()[0])
    sets = dict(agents=u8(max(total, 1) * REC), first=i32(B + 1), count=i32(B), status=i32(B), set_of=i32(B), src_index=i32(max(total, 1)),
                total=torch.zeros(1, dtype=torch.int64, device="cuda"))
    # everybody but me, built on the host: ego b takes the records of its world's other vehicles and its world's perception agents
    per_ego = (VEHICLES - 1) * D + SEEN
    index = np.zeros((B, per_ego), dtype=np.int64)  # into the concatenation [fleet records, perception records]
    for b in range(B):
        w, fleet = b // VEHICLES, np.arange(VEHICLES * D) + (b // VEHICLES) * VEHICLES * D
        index[b] = np.concatenate((fleet[fleet // D != b], B * D + w * SEEN + np.arange(SEEN)))
    index = index.reshape(-1)
    every_first = dev((np.arange(B + 1) * per_ego).astype(np.int32))
    every_set_of = dev(np.arange(B, dtype=np.int32))
    every = {"agents": None}

    def host_build_upload():
        fleet = tr["agents"].cpu().numpy().view(binding.AGENT_DTYPE)  # (synchronises: the records are on the host)
        built = np.concatenate((fleet, seen_h))[index]
        every["agents"] = torch.from_numpy(built.view(np.uint8)).cuda()
        torch.cuda.synchronize()

    with torch.cuda.stream(stream):
        host_build_upload()
    dyn_c = dict(status=i32(B), first_state=i32(B), first_agent=i32(B), v_limit=f64(B, N))
    dyn_e = dict(status=i32(B), first_state=i32(B), first_agent=i32(B), v_limit=f64(B, N))
    path = dict(states=states, t=spd["t"])
    variants = {
        "agentsets": lambda: eng.agentsets_batch_device(sets_in, sets, sets_p),
        "agentsets_count": lambda: eng.agentsets_batch_device(sets_in, count_out, sets_p),
        "dynamic_composed": lambda: eng.dynamic_batch_device(dict(path, agents=sets["agents"], first=sets["first"], set_of=sets["set_of"]), dyn_c, dp),
        "dynamic_everybody": lambda: eng.dynamic_batch_device(dict(path, agents=every["agents"], first=every_first, set_of=every_set_of), dyn_e, dp),
    }
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    ts["host_build_upload"] = []
    for _ in range(a.reps):  # one round: every variant once
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        with torch.cuda.stream(stream):
            host_build_upload()
        ts["host_build_upload"].append((time.perf_counter() - w0) * 1e3)
    torch.cuda.synchronize()
    stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    st_c, st_e = dyn_c["status"].cpu().numpy(), dyn_e["status"].cpu().numpy()
    row = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "worlds": WORLDS, "vehicles_per_world": VEHICLES, "B": B, "N": N,
           "records_per_vehicle": D, "perception_per_world": SEEN, "square_m": SQUARE_M, "step_m": STEP_M, "reach": float(sets_p.reach),
           "records_offered": B * per_ego, "records_kept": total, "kept_fraction": total / (B * per_ego), "mean_set": total / B,
           "largest_set": int(sets["count"].cpu().numpy().max()), "sets_status": {str(k): int((sets["status"].cpu().numpy() == k).sum()) for k in (0, 1, 2)},
           "agentsets_ms": dict(stat(ts["agentsets"]), what="po_agentsets_batch_device, 4 096 egos, every output, three launches"),
           "agentsets_count_ms": dict(stat(ts["agentsets_count"]), what="the counting call: capacity 0, two launches"),
           "dynamic_composed_ms": dict(stat(ts["dynamic_composed"]), what="po_dynamic_batch_device on the composed sets"),
           "dynamic_everybody_ms": dict(stat(ts["dynamic_everybody"]), what=f"po_dynamic_batch_device on host-built everybody-but-me sets, {per_ego} records each"),
           "host_build_upload_ms": dict(stat(ts["host_build_upload"]), what="wall clock: records to the host, 4 096 sets gathered by a precomputed index, upload, synchronise"),
           "everybody_bytes": int(B * per_ego * REC), "composed_bytes": int(total * REC),
           "dynamic_status_equal": bool((st_c == st_e).all()), "dynamic_first_state_equal": bool((dyn_c["first_state"].cpu().numpy() == dyn_e["first_state"].cpu().numpy()).all()),
           "dynamic_status": {str(k): int((st_c == k).sum()) for k in (0, 1, 2, 3)}}
    row["composed_chain_ms"] = row["agentsets_ms"]["median"] + row["dynamic_composed_ms"]["median"]
    row["everybody_chain_ms"] = row["host_build_upload_ms"]["median"] + row["dynamic_everybody_ms"]["median"]
    eng.set_stream(None)
    eng.close()
    print(f"[agentsets_bench] agent sets {row['agentsets_ms']['median'] * 1e3:.0f} us (count alone {row['agentsets_count_ms']['median'] * 1e3:.0f} us), kept "
          f"{100 * row['kept_fraction']:.1f} % ({row['mean_set']:.1f} a set); dynamic {row['dynamic_composed_ms']['median']:.2f} ms on the composed sets, "
          f"{row['dynamic_everybody_ms']['median']:.2f} ms on everybody-but-me; host build + upload {row['host_build_upload_ms']['median']:.1f} ms", file=sys.stderr)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
