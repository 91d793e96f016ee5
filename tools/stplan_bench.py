"""Measurement (GPU): what the station-time planning stage costs behind po_plan_batch, po_speed_batch and po_dynamic_batch.

Shape: tools/dynamic_bench.py's — 512 groups x 8 candidates = 4 096 planning instances from the 64 seeded scenes, one map, N = 320 rows per path.
po_plan_batch_device produces the paths and po_speed_batch_device a profile without agents once (its v is the planner's v_cap, its total_time places the agents);
every group gets an agent set of its own (set_of[b] = the group of b), built by dynamic_bench.agent_sets.  Then, on a stream of its own with hipEvents around each
call (median of --reps timed calls after --warmup calls), for 32 and for 4 agents per set, with the default parameters (po_default_stplan_params):
  stplan             po_stplan_batch_device alone on the 4 096 paths, every output asked for
  stplan_no_agents   the same call against empty sets: phase 1 has nothing to do, what is left is the stations and the search (measured once)
  round              po_stplan_batch_device -> po_speed_batch_device(v_limit of the plan) -> po_dynamic_batch_device, three enqueues and no synchronisation
and, in the same run, plan: po_plan_batch_device of the 4 096 instances.  cell_agent_pairs counts K * M * agents over the planned paths and search_edges
K * M * (U + 1)^2: the mapping predicts phase 1 proportional to the first and phase 2 bounded by the second.  Nothing is asserted and no threshold is set: numbers
go to --out (default profiles/stplan/stplan_bench.json) and to stdout as one JSON line.
    python tools/stplan_bench.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stplan", "stplan_bench.json"))
    a = ap.parse_args()
    import torch

    import dynamic_bench
    import select_bench
    from path_optimizer_amd import binding, synth
    from path_optimizer_amd.abi import INFO_BYTES, PO_ST_MAX_STATIONS

    if not torch.cuda.is_available():
        raise SystemExit("stplan_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    if a.reps < 20:
        raise SystemExit("stplan_bench: at least 20 timed repetitions")
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
    sp, dp, st = binding.default_speed_params(), binding.default_dynamic_params(), binding.default_stplan_params()
    row["stplan_params"] = {f: getattr(st, f) for f, _ in st._fields_}
    v0 = torch.full((B,), 5.0, dtype=torch.float64, device="cuda")
    spd_in = dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], v0=v0)
    spd = dict(v=f64(B, N), a=f64(B, N), t=f64(B, N), total_time=f64(B), status=i32(B))
    spd2 = dict(v=f64(B, N), a=f64(B, N), t=f64(B, N), total_time=f64(B), status=i32(B))
    eng.speed_batch_device(spd_in, spd, sp)
    torch.cuda.synchronize()
    states, n_states, ok = plan["states"].cpu().numpy(), plan["n_states"].cpu().numpy(), plan["ok"].cpu().numpy()
    row["plan_ok"] = int(ok.sum()); row["mean_states"] = float(n_states[ok != 0].mean()) if ok.any() else 0.0
    row["speed_ms"] = dict(ev(lambda: eng.speed_batch_device(spd_in, spd, sp)), what="po_speed_batch_device, 4 096 paths, use_map = 0, both launches")
    total_time = spd["total_time"].cpu().numpy()
    set_of = dev(np.repeat(np.arange(G, dtype=np.int32), PER))
    out = dict(status=i32(B), ok_out=i32(B), n_layers=i32(B), cost=f64(B), station=i32(B, 17), cells=i32(B, st.K, PO_ST_MAX_STATIONS), v_limit=f64(B, N))
    dyn = dict(status=i32(B), ok_out=i32(B), gap_min=f64(B), first_state=i32(B), first_agent=i32(B), stop_state=i32(B), first_time=f64(B), gap=f64(B, N), v_limit=f64(B, N))
    base_in = dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], v0=v0, v_cap=spd["v"], set_of=set_of)
    empty = dict(base_in, agents=None, first=dev(np.zeros(G + 1, dtype=np.int32)))
    row["stplan_no_agents_ms"] = dict(ev(lambda: eng.stplan_batch_device(empty, out, st)), what="po_stplan_batch_device against empty sets: stations and search only")
    rows = []
    for per_set in (32, 4):
        agents, first = binding.pack_agents(dynamic_bench.agent_sets(np.random.default_rng([25, per_set]), states, n_states, total_time, G, PER, per_set))
        p_in = dict(base_in, agents=dev(agents.view(np.uint8)), first=dev(first))
        r = {"agents_per_set": per_set, "sets": G, "points_per_agent": "4 .. 8", "mean_points": float(agents["n_pts"].mean())}
        r["stplan_ms"] = dict(ev(lambda: eng.stplan_batch_device(p_in, out, st)), what="po_stplan_batch_device, 4 096 paths, every output")

        def round_():
            eng.stplan_batch_device(p_in, out, st)
            eng.speed_batch_device(dict(spd_in, v_limit=out["v_limit"]), spd2, sp)
            eng.dynamic_batch_device(dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], t=spd2["t"], set_of=set_of, agents=p_in["agents"],
                                          first=p_in["first"]), dyn, dp)

        r["round_ms"] = dict(ev(round_), what="stplan -> speed(v_limit) -> dynamic, three enqueues, no synchronisation")
        torch.cuda.synchronize()
        status, dstatus, layers = out["status"].cpu().numpy(), dyn["status"].cpu().numpy(), out["n_layers"].cpu().numpy()
        r["status"] = {str(k): int((status == k).sum()) for k in (0, 1, 2, 3)}
        r["dynamic_status_after"] = {str(k): int((dstatus == k).sum()) for k in (0, 1, 2, 3)}
        r["mean_layers"] = float(layers[status > 0].mean()) if (status > 0).any() else 0.0
        M = np.minimum((np.maximum(n_states[status > 0], 1) - 1) // st.stride + 1, PO_ST_MAX_STATIONS)
        r["cell_agent_pairs"] = int(M.sum()) * st.K * per_set
        r["search_edges"] = int(M.sum()) * st.K * (st.U + 1) ** 2
        r["phase1_ms_estimate"] = r["stplan_ms"]["median"] - row["stplan_no_agents_ms"]["median"]
        r["ns_per_cell_agent_pair"] = r["phase1_ms_estimate"] * 1e6 / max(r["cell_agent_pairs"], 1)
        r["round_over_plan"] = r["round_ms"]["median"] / row["plan_ms"]["median"]
        rows.append(r)
    row["rows"] = rows
    row["ns_per_search_edge"] = row["stplan_no_agents_ms"]["median"] * 1e6 / max(rows[0]["search_edges"], 1)
    eng.set_stream(None)
    eng.close()
    for r in rows:
        print(f"[stplan_bench] {r['agents_per_set']} agents per set: stplan {r['stplan_ms']['median'] * 1e3:.0f} us (no agents {row['stplan_no_agents_ms']['median'] * 1e3:.0f} us), "
              f"round {r['round_ms']['median'] * 1e3:.0f} us (plan {row['plan_ms']['median']:.2f} ms), statuses {r['status']}, dynamic after {r['dynamic_status_after']}",
              file=sys.stderr)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
