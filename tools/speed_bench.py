"""Measurement (GPU): what the speed-profile stage costs behind po_plan_batch and po_select_batch.

Shape: tools/select_bench.py's — 512 groups x 8 candidates = 4 096 planning instances from the 64 seeded scenes, one map, N = 320 rows per path.
po_plan_batch_device produces the candidates and po_select_batch_device the 512 winners once; then, on a stream of its own with hipEvents around each call
(median of --reps timed calls after --warmup calls):
  plan               po_plan_batch_device of the 4 096 instances (it synchronises its stream once mid-way, so this is events around a call that blocks)
  speed_all          po_speed_batch_device on all 4 096 candidate paths (n_states and ok of the plan call), use_map = 0
  speed_all_map      the same with the clearance cap (use_map = 1): six map samples per state more
  speed_winners      po_speed_batch_device on the 512 winners (sel_states / sel_n), use_map = 0
  speed_winners_map  the same with use_map = 1
  limits_all         po_limits_batch_device on v, a of the 4 096 paths
  limits_winners     po_limits_batch_device on v, a of the 512 winners
Start speed 5 m/s, end speed 0 for every path; t and total_time are asked for.  Nothing is asserted and no threshold is set: numbers go to --out (default
profiles/speed/speed_bench.json) and to stdout as one JSON line.
    python tools/speed_bench.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import ctypes
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speed", "speed_bench.json"))
    a = ap.parse_args()
    import torch

    import select_bench
    from path_optimizer_amd import binding, synth
    from path_optimizer_amd.abi import INFO_BYTES

    if not torch.cuda.is_available():
        raise SystemExit("speed_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    if a.reps < 20:
        raise SystemExit("speed_bench: at least 20 timed repetitions")
    G, PER, N = select_bench.G, select_bench.PER, select_bench.N
    B = G * PER
    t_host, the_map = select_bench.candidates(synth)
    way_len = float(np.hypot(np.diff(t_host["way_x"], axis=1), np.diff(t_host["way_y"], axis=1)).sum(axis=1).max())
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    t = {k: dev(v) for k, v in t_host.items()}
    plan = dict(states=f64(B, N, 5), n_states=i32(B), ok=i32(B), stage=i32(B), info=torch.zeros((B, INFO_BYTES), dtype=torch.uint8, device="cuda"))
    sel = dict(best=i32(G), sel_states=f64(G, N, 5), sel_n=i32(G))
    stream = torch.cuda.Stream()  # (a stream of its own: the default stream's handle is NULL, which po_set_stream reads as "the handle's own stream")
    eng = binding.Engine(0)
    eng.set_map(*the_map)
    eng.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ev = lambda fn: select_bench.event_ms(torch, stream, fn, a.reps, a.warmup)
    row = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "groups": G, "candidates_per_group": PER, "B": B, "N": N}
    row["plan_ms"] = dict(ev(lambda: eng.plan_batch_device(t, plan, N, way_len)), what="po_plan_batch_device, 4 096 instances")
    eng.select_batch_device(dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], goal=t["goal"],
                                 group_start=dev(np.arange(0, B + 1, PER, dtype=np.int32))), sel)
    torch.cuda.synchronize()
    n_states, ok = plan["n_states"].cpu().numpy(), plan["ok"].cpu().numpy()
    row["plan_ok"] = int(ok.sum()); row["mean_states"] = float(n_states[ok != 0].mean()) if ok.any() else 0.0
    row["groups_with_a_winner"] = int((sel["best"].cpu().numpy() >= 0).sum())

    def stage(n_paths, states, n_st, okk):
        inp = dict(states=states, n_states=n_st, ok=okk, v0=torch.full((n_paths,), 5.0, dtype=torch.float64, device="cuda"), v_end=f64(n_paths))
        out = dict(v=f64(n_paths, N), a=f64(n_paths, N), t=f64(n_paths, N), total_time=f64(n_paths), status=i32(n_paths))
        return inp, out, f64(n_paths, N), f64(n_paths, N)

    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    L = binding.lib()
    for tag, (inp, out, mk, mkp), n_paths in (("all", stage(B, plan["states"], plan["n_states"], plan["ok"]), B), ("winners", stage(G, sel["sel_states"], sel["sel_n"], None), G)):
        for suffix, use_map in (("", 0), ("_map", 1)):
            sp = binding.default_speed_params()
            sp.use_map = use_map
            row[f"speed_{tag}{suffix}_ms"] = dict(ev(lambda: eng.speed_batch_device(inp, out, sp)),
                                                 what=f"po_speed_batch_device, {n_paths} paths, use_map = {use_map}, both launches")
        torch.cuda.synchronize()
        status = out["status"].cpu().numpy()
        row[f"status_{tag}"] = {str(k): int((status == k).sum()) for k in (0, 1, 2)}
        row[f"mean_total_time_{tag}_s"] = float(out["total_time"].cpu().numpy()[status > 0].mean()) if (status > 0).any() else 0.0

        def limits():
            rc = L.po_limits_batch_device(eng._h, n_paths, N, ptr(inp["n_states"]), ptr(out["v"]), ptr(out["a"]), ptr(mk), ptr(mkp))
            assert rc == 0, rc

        row[f"limits_{tag}_ms"] = dict(ev(limits), what=f"po_limits_batch_device on v, a of the {n_paths} paths")
        torch.cuda.synchronize()
        row[f"limits_{tag}_nan"] = int(torch.isnan(mk).sum().item() + torch.isnan(mkp).sum().item())
    row["speed_all_map_over_plan"] = row["speed_all_map_ms"]["median"] / row["plan_ms"]["median"]
    eng.set_stream(None)
    eng.close()
    us = lambda k: row[k]["median"] * 1e3
    print(f"[speed_bench] plan {row['plan_ms']['median']:.2f} ms; speed on {B}: {us('speed_all_ms'):.0f} us (map: {us('speed_all_map_ms'):.0f} us), on {G} winners: "
          f"{us('speed_winners_ms'):.0f} us (map: {us('speed_winners_map_ms'):.0f} us); limits {us('limits_all_ms'):.0f} / {us('limits_winners_ms'):.0f} us", file=sys.stderr)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
