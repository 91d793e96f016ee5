"""Measurement (GPU): what the score-and-select stage costs behind po_plan_batch, and what it saves on PCIe.

Shape: 512 groups x 8 candidates = 4 096 planning instances.  The groups are the 64 scenes of synth.make_planning_scenes (seeded) taken round robin; the 8
candidates of a group are waypoint variants of its scene (the interior waypoints moved sideways by up to 0.3 m; variant 0 is the scene itself).  One map, N = 320
rows per path.  po_plan_batch_device produces the candidates once; then, on a stream of its own with hipEvents around each call (the method of
tools/raster_bench.py: median of --reps timed calls after --warmup calls):
  plan          po_plan_batch_device of the 4 096 instances (it synchronises its stream once mid-way, so this is events around a call that blocks)
  select        po_select_batch_device with goals and a previous path per group (the winners of a first call: Np = N)
  select_np0    the same call without previous paths (Np = 0): what the point-segment loop costs is the difference
  d2h_all       states [B][N][5] + n_states + ok to pinned host memory
  d2h_winners   sel_states [G][N][5] + sel_n + best to pinned host memory
Nothing is asserted: numbers go to --out (default profiles/select/select_bench.json) and to stdout as one JSON line.
    python tools/select_bench.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G, PER, SCENES, N = 512, 8, 64, 320


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


def candidates(synth):
    """way_x, way_y [B, W], start [B, 4], goal [B, 3] of the 4 096 instances, group-major, and the shared map."""
    scn = synth.make_planning_scenes(23, SCENES)
    rng = np.random.default_rng(24)
    idx = np.repeat(np.arange(G) % SCENES, PER)
    wx, wy = scn["way_x"][idx].copy(), scn["way_y"][idx].copy()
    jit = rng.uniform(-0.3, 0.3, wx.shape)
    jit[::PER] = 0.0; jit[:, 0] = 0.0; jit[:, -1] = 0.0
    hz = np.arctan2(np.gradient(wy, axis=1), np.gradient(wx, axis=1))
    return dict(way_x=wx - jit * np.sin(hz), way_y=wy + jit * np.cos(hz), start=scn["start"][idx].copy(), goal=scn["goal"][idx].copy()), scn["map"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select", "select_bench.json"))
    a = ap.parse_args()
    import torch

    from path_optimizer_amd import binding, synth
    from path_optimizer_amd.abi import INFO_BYTES

    if not torch.cuda.is_available():
        raise SystemExit("select_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    if a.reps < 20:
        raise SystemExit("select_bench: at least 20 timed repetitions")
    B = G * PER
    t_host, the_map = candidates(synth)
    way_len = float(np.hypot(np.diff(t_host["way_x"], axis=1), np.diff(t_host["way_y"], axis=1)).sum(axis=1).max())
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    t = {k: dev(v) for k, v in t_host.items()}
    plan = dict(states=torch.zeros((B, N, 5), dtype=torch.float64, device="cuda"), n_states=torch.zeros(B, dtype=torch.int32, device="cuda"),
                ok=torch.zeros(B, dtype=torch.int32, device="cuda"), stage=torch.zeros(B, dtype=torch.int32, device="cuda"),
                info=torch.zeros((B, INFO_BYTES), dtype=torch.uint8, device="cuda"))
    gs = dev(np.arange(0, B + 1, PER, dtype=np.int32))

    def outputs():
        return dict(best=torch.zeros(G, dtype=torch.int32, device="cuda"), best_cost=torch.zeros(G, dtype=torch.float64, device="cuda"),
                    n_feasible=torch.zeros(G, dtype=torch.int32, device="cuda"), sel_states=torch.zeros((G, N, 5), dtype=torch.float64, device="cuda"),
                    sel_n=torch.zeros(G, dtype=torch.int32, device="cuda"))

    first, out = outputs(), outputs()
    stream = torch.cuda.Stream()  # (a stream of its own: the default stream's handle is NULL, which po_set_stream reads as "the handle's own stream")
    eng = binding.Engine(0)
    eng.set_map(*the_map)
    eng.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    sel_in = dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], goal=t["goal"], group_start=gs)
    row = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "groups": G, "candidates_per_group": PER, "B": B, "N": N}
    row["plan_ms"] = dict(event_ms(torch, stream, lambda: eng.plan_batch_device(t, plan, N, way_len), a.reps, a.warmup), what="po_plan_batch_device, 4 096 instances")
    eng.select_batch_device(sel_in, first)  # cycle 0: its winners are the previous paths of the timed calls
    torch.cuda.synchronize()
    n_states, ok = plan["n_states"].cpu().numpy(), plan["ok"].cpu().numpy()
    row["plan_ok"] = int(ok.sum()); row["mean_states"] = float(n_states[ok != 0].mean()) if ok.any() else 0.0
    row["groups_with_a_winner"] = int((first["best"].cpu().numpy() >= 0).sum())
    with_prev = dict(sel_in, prev_states=first["sel_states"], prev_n=first["sel_n"])
    row["select_ms"] = dict(event_ms(torch, stream, lambda: eng.select_batch_device(with_prev, out), a.reps, a.warmup),
                            what="po_select_batch_device: goals and a previous path per group (Np = N), the three launches")
    row["select_np0_ms"] = dict(event_ms(torch, stream, lambda: eng.select_batch_device(sel_in, out), a.reps, a.warmup), what="the same without previous paths (Np = 0)")
    pin = lambda x: torch.empty(x.shape, dtype=x.dtype).pin_memory()
    h_all = [pin(plan[k]) for k in ("states", "n_states", "ok")]
    h_win = [pin(out[k]) for k in ("sel_states", "sel_n", "best")]

    def copy(dst, src):
        with torch.cuda.stream(stream):
            for d, s_ in zip(dst, src):
                d.copy_(s_, non_blocking=True)

    row["d2h_all_ms"] = dict(event_ms(torch, stream, lambda: copy(h_all, [plan[k] for k in ("states", "n_states", "ok")]), a.reps, a.warmup),
                             what="states [B][N][5] + n_states + ok to pinned memory", bytes=int(sum(x.numel() * x.element_size() for x in h_all)))
    row["d2h_winners_ms"] = dict(event_ms(torch, stream, lambda: copy(h_win, [out[k] for k in ("sel_states", "sel_n", "best")]), a.reps, a.warmup),
                                 what="sel_states [G][N][5] + sel_n + best to pinned memory", bytes=int(sum(x.numel() * x.element_size() for x in h_win)))
    row["select_over_plan"] = row["select_ms"]["median"] / row["plan_ms"]["median"]
    eng.set_stream(None)
    eng.close()
    print(f"[select_bench] plan {row['plan_ms']['median']:.2f} ms, select {row['select_ms']['median'] * 1e3:.0f} us (Np = 0: {row['select_np0_ms']['median'] * 1e3:.0f} us), "
          f"D2H all {row['d2h_all_ms']['median']:.2f} ms, winners {row['d2h_winners_ms']['median'] * 1e3:.0f} us", file=sys.stderr)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
