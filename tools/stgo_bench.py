"""Measurement tool (GPU): what po_stgo_batch_device costs beside po_stplan_batch_device, on the measurement shape of DESIGN.md section 29.

The 4 096 planned paths of tools/stplan_bench.py (64 groups of 64 candidates, N = 320, v_cap from a speed profile, v0 = 5 m/s) against 32 and against 4 agents per
set, default parameters (po_default_stgo_params; its first ten fields are po_default_stplan_params').  Device events around each call, after --warmup calls of both
stages; the two stages are timed in ALTERNATING rounds of one run (stgo, stplan, stgo, ...), so whatever else the machine does meets both alike:
  stgo       po_stgo_batch_device, every output, Q = 81 (the default)
  stplan     po_stplan_batch_device, every output
  stgo_q1    po_stgo_batch_device with Q = 1, every output: what is left of the stage without the sampler (timed in rounds alternating with Q = 81)
and counts: the statuses of both stages, the paths whose plan resumes (n_resumes > 0), the paths on which the two stages chose different stations, the endings.
Results go to --out (default profiles/stgo/stgo_bench.json) and to stdout as one JSON line.
    python tools/stgo_bench.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def alternating_ms(torch, stream, fns, reps, warmup):
    """{name: median / min / max} of `reps` timed calls of every fn, one call of each per round, after `warmup` rounds."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stgo", "stgo_bench.json"))
    a = ap.parse_args()
    import torch

    import dynamic_bench
    import select_bench
    from path_optimizer_amd import binding, synth
    from path_optimizer_amd.abi import INFO_BYTES, PO_ST_MAX_STATIONS

    if not torch.cuda.is_available():
        raise SystemExit("stgo_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    if a.reps < 20:
        raise SystemExit("stgo_bench: at least 20 timed repetitions")
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
    eng.plan_batch_device(t, plan, N, way_len)
    sp, st, gp, g1 = binding.default_speed_params(), binding.default_stplan_params(), binding.default_stgo_params(), binding.default_stgo_params()
    g1.Q = 1
    Q = int(gp.Q)
    row = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "groups": G, "candidates_per_group": PER, "B": B, "N": N,
           "stgo_params": {f: getattr(gp, f) for f, _ in gp._fields_}}
    v0 = torch.full((B,), 5.0, dtype=torch.float64, device="cuda")
    spd = dict(v=f64(B, N), a=f64(B, N), t=f64(B, N), total_time=f64(B), status=i32(B))
    eng.speed_batch_device(dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], v0=v0), spd, sp)
    torch.cuda.synchronize()
    states, n_states, ok = plan["states"].cpu().numpy(), plan["n_states"].cpu().numpy(), plan["ok"].cpu().numpy()
    row["plan_ok"] = int(ok.sum()); row["mean_states"] = float(n_states[ok != 0].mean()) if ok.any() else 0.0
    total_time = spd["total_time"].cpu().numpy()
    set_of = dev(np.repeat(np.arange(G, dtype=np.int32), PER))
    shared = lambda: dict(status=i32(B), ok_out=i32(B), n_layers=i32(B), cost=f64(B), station=i32(B, 17), cells=i32(B, st.K, PO_ST_MAX_STATIONS))
    samples = lambda q: dict(n_resumes=i32(B), states=f64(B, q, 5), v=f64(B, q), a=f64(B, q), t=f64(B, q), index=i32(B, q), first_held=i32(B), end=i32(B))
    out_p, out_g, out_1 = dict(shared(), v_limit=f64(B, N)), dict(shared(), **samples(Q)), dict(shared(), **samples(1))
    base_in = dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], v0=v0, v_cap=spd["v"], set_of=set_of)
    rows = []
    for per_set in (32, 4):
        agents, first = binding.pack_agents(dynamic_bench.agent_sets(np.random.default_rng([25, per_set]), states, n_states, total_time, G, PER, per_set))
        p_in = dict(base_in, agents=dev(agents.view(np.uint8)), first=dev(first))
        r = {"agents_per_set": per_set, "sets": G, "mean_points": float(agents["n_pts"].mean())}
        ms = alternating_ms(torch, stream, {"stgo": lambda: eng.stgo_batch_device(p_in, out_g, gp), "stplan": lambda: eng.stplan_batch_device(p_in, out_p, st)},
                            a.reps, a.warmup)
        r["stgo_ms"] = dict(ms["stgo"], what=f"po_stgo_batch_device, 4 096 paths, every output, Q = {Q}")
        r["stplan_ms"] = dict(ms["stplan"], what="po_stplan_batch_device, 4 096 paths, every output; alternating with stgo")
        ms = alternating_ms(torch, stream, {"q": lambda: eng.stgo_batch_device(p_in, out_g, gp), "q1": lambda: eng.stgo_batch_device(p_in, out_1, g1)}, a.reps, a.warmup)
        r["stgo_again_ms"] = dict(ms["q"], what=f"po_stgo_batch_device, Q = {Q}; alternating with Q = 1")
        r["stgo_q1_ms"] = dict(ms["q1"], what="po_stgo_batch_device, Q = 1")
        r["sampler_ms_estimate"] = r["stgo_again_ms"]["median"] - r["stgo_q1_ms"]["median"]
        r["stgo_over_stplan"] = r["stgo_ms"]["median"] / r["stplan_ms"]["median"]
        torch.cuda.synchronize()
        sg, spn = out_g["status"].cpu().numpy(), out_p["status"].cpu().numpy()
        r["status_stgo"] = {str(k): int((sg == k).sum()) for k in (0, 1, 2, 3)}
        r["status_stplan"] = {str(k): int((spn == k).sum()) for k in (0, 1, 2, 3)}
        r["paths_that_resume"] = int((out_g["n_resumes"].cpu().numpy() > 0).sum())
        r["paths_with_other_stations"] = int((out_g["station"].cpu().numpy() != out_p["station"].cpu().numpy()).any(axis=1).sum())
        end = out_g["end"].cpu().numpy()
        r["end"] = {str(k): int((end == k).sum()) for k in range(5)}
        rows.append(r)
    row["rows"] = rows
    eng.set_stream(None)
    eng.close()
    for r in rows:
        print(f"[stgo_bench] {r['agents_per_set']} agents per set: stgo {r['stgo_ms']['median'] * 1e3:.0f} us, stplan {r['stplan_ms']['median'] * 1e3:.0f} us, "
              f"Q = 1 {r['stgo_q1_ms']['median'] * 1e3:.0f} us, resumes on {r['paths_that_resume']} paths, statuses {r['status_stgo']}", file=sys.stderr)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
