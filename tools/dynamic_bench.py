"""Measurement (GPU): what the moving-obstacle stage costs behind po_plan_batch and po_speed_batch.

Shape: tools/select_bench.py's — 512 groups x 8 candidates = 4 096 planning instances from the 64 seeded scenes, one map, N = 320 rows per path.
po_plan_batch_device produces the paths and po_speed_batch_device their times once; every group gets an agent set of its own (set_of[b] = the group of b): agents
of 4 .. 8 points that walk across the group's first path within the path's own time span, half of them held before or after.  Then, on a stream of its own with
hipEvents around each call (median of --reps timed calls after --warmup calls), for 32 and for 4 agents per set:
  dynamic            po_dynamic_batch_device alone on the 4 096 timed paths, every output asked for
  yield_round        po_speed_batch_device -> po_dynamic_batch_device -> po_speed_batch_device(v_limit of the check), three enqueues and no synchronisation
and, in the same run, plan: po_plan_batch_device of the 4 096 instances.  checked_pairs counts the (interval, agent) pairs of the checked paths: the mapping
predicts a cost proportional to it.  Nothing is asserted and no threshold is set: numbers go to --out (default profiles/dynamic/dynamic_bench.json) and to stdout
as one JSON line.
    python tools/dynamic_bench.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def agent_sets(rng, states, n_states, total_time, G, PER, per_set):
    """One set per group: agents that cross the group's first path somewhere along it, at about the time the ego is there."""
    sets = []
    for g in range(G):
        b = g * PER
        n = max(int(n_states[b]), 2)
        T = max(float(total_time[b]), 1.0)
        agents = []
        for _ in range(per_set):
            npts = int(rng.integers(4, 9))
            i = int(rng.integers(0, n))
            cx, cy = states[b, i, 0], states[b, i, 1]
            hz = rng.uniform(0, 2 * np.pi)
            reach = rng.uniform(3.0, 12.0)
            u = np.linspace(-1.0, 1.0, npts)
            t0 = T * i / n + rng.uniform(-2.0, 2.0)
            tt = t0 + np.cumsum(np.concatenate(([0.0], rng.uniform(0.3, 1.5, npts - 1)))) - 2.0
            x = cx + reach * u * np.cos(hz) + rng.uniform(-0.5, 0.5, npts)
            y = cy + reach * u * np.sin(hz) + rng.uniform(-0.5, 0.5, npts) + rng.uniform(0.0, 6.0)
            agents.append((rng.uniform(0.3, 1.0), int(rng.integers(0, 4)), list(zip(tt, x, y))))
        sets.append(agents)
    return sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamic", "dynamic_bench.json"))
    a = ap.parse_args()
    import torch

    import select_bench
    from path_optimizer_amd import binding, synth
    from path_optimizer_amd.abi import INFO_BYTES

    if not torch.cuda.is_available():
        raise SystemExit("dynamic_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    if a.reps < 20:
        raise SystemExit("dynamic_bench: at least 20 timed repetitions")
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
    ev = lambda fn: select_bench.event_ms(torch, stream, fn, a.reps, a.warmup)
    row = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "groups": G, "candidates_per_group": PER, "B": B, "N": N}
    row["plan_ms"] = dict(ev(lambda: eng.plan_batch_device(t, plan, N, way_len)), what="po_plan_batch_device, 4 096 instances")
    sp = binding.default_speed_params()
    spd_in = dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], v0=torch.full((B,), 5.0, dtype=torch.float64, device="cuda"))
    spd = dict(v=f64(B, N), a=f64(B, N), t=f64(B, N), total_time=f64(B), status=i32(B))
    spd2 = dict(v=f64(B, N), a=f64(B, N), t=f64(B, N), total_time=f64(B), status=i32(B))
    eng.speed_batch_device(spd_in, spd, sp)
    torch.cuda.synchronize()
    states, n_states, ok = plan["states"].cpu().numpy(), plan["n_states"].cpu().numpy(), plan["ok"].cpu().numpy()
    row["plan_ok"] = int(ok.sum()); row["mean_states"] = float(n_states[ok != 0].mean()) if ok.any() else 0.0
    row["speed_ms"] = dict(ev(lambda: eng.speed_batch_device(spd_in, spd, sp)), what="po_speed_batch_device, 4 096 paths, use_map = 0, both launches")
    total_time = spd["total_time"].cpu().numpy()
    set_of = dev(np.repeat(np.arange(G, dtype=np.int32), PER))
    dp = binding.default_dynamic_params()
    rows = []
    for per_set in (32, 4):
        agents, first = binding.pack_agents(agent_sets(np.random.default_rng([25, per_set]), states, n_states, total_time, G, PER, per_set))
        d_in = dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], t=spd["t"], set_of=set_of, agents=dev(agents.view(np.uint8)), first=dev(first))
        out = dict(status=i32(B), ok_out=i32(B), gap_min=f64(B), first_state=i32(B), first_agent=i32(B), stop_state=i32(B), first_time=f64(B), gap=f64(B, N),
                   v_limit=f64(B, N))
        r = {"agents_per_set": per_set, "sets": G, "points_per_agent": "4 .. 8", "mean_points": float(agents["n_pts"].mean())}
        r["dynamic_ms"] = dict(ev(lambda: eng.dynamic_batch_device(d_in, out, dp)), what="po_dynamic_batch_device, 4 096 paths, every output")

        def yield_round():
            eng.speed_batch_device(spd_in, spd, sp)
            eng.dynamic_batch_device(d_in, out, dp)
            eng.speed_batch_device(dict(spd_in, v_limit=out["v_limit"]), spd2, sp)

        r["yield_round_ms"] = dict(ev(yield_round), what="speed -> dynamic -> speed(v_limit), three enqueues, no synchronisation")
        torch.cuda.synchronize()
        status = out["status"].cpu().numpy()
        r["status"] = {str(k): int((status == k).sum()) for k in (0, 1, 2, 3)}
        r["checked_pairs"] = int(np.maximum(n_states[status > 0] - 1, 0).sum()) * per_set
        r["ns_per_pair"] = r["dynamic_ms"]["median"] * 1e6 / max(r["checked_pairs"], 1)
        r["yield_round_over_plan"] = r["yield_round_ms"]["median"] / row["plan_ms"]["median"]
        rows.append(r)
    row["rows"] = rows
    row["dynamic_32_over_4"] = rows[0]["dynamic_ms"]["median"] / rows[1]["dynamic_ms"]["median"]
    eng.set_stream(None)
    eng.close()
    for r in rows:
        print(f"[dynamic_bench] {r['agents_per_set']} agents per set: dynamic {r['dynamic_ms']['median'] * 1e3:.0f} us, yield round {r['yield_round_ms']['median'] * 1e3:.0f} us "
              f"(plan {row['plan_ms']['median']:.2f} ms), statuses {r['status']}", file=sys.stderr)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
