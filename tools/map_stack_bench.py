"""B planning instances over M obstacle maps: one call pair per map against one call pair for the whole batch.

For B = 4096 instances over M = 1, 8, 64, 512 maps of 495 x 497 cells (the size of the reference's benchmark scene):
  (a) M x (set_map_occupancy_device of map k + plan_batch_device of its B / M instances)   — what a caller with M scenes had to do before the map stack;
  (b) one set_map_stack_occupancy_device of the M images + one plan_batch_device of the B instances, the instance -> layer table installed once outside the
      timed loop (a same-M refresh keeps it).
Both on the device-pointer entries and on one stream, wall clock from the first enqueue to the end of a final synchronisation, median of --calls calls after
--warmup calls.  The outputs of (a) and (b) are compared once per M: ok / n_states / stage exactly, the states by their largest difference (a batch of B / M and
a batch of B instances take different launch shapes of the QP kernels, whose solutions agree to round-off, not bit for bit).  Writes profiles/map_stack/map_stack_bench.json (or --out).

The M layers are eight synthetic scenes (synth.make_planning_scenes, 64 instances each) reused cyclically, each layer at its own map centre with its instances
moved along; every instance therefore lies inside its own layer and, for M > 1, mostly outside layer 0."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SX, SY, NP, BASE = 495, 497, 320, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--maps", type=int, nargs="+", default=[1, 8, 64, 512])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_stack", "map_stack_bench.json"))
    a = ap.parse_args()
    import torch

    from path_optimizer_amd import binding, synth
    from path_optimizer_amd.abi import INFO_BYTES

    B = a.batch
    base = [synth.make_planning_scenes(100 + i, 64, map_kw=dict(size_x=SX, size_y=SY)) for i in range(BASE)]
    res = base[0]["map"][1]
    occ_base = np.stack([np.ascontiguousarray((s["map"][0] > 0).astype(np.uint8).T) for s in base])  # [BASE][size_y][size_x], 0 = occupied
    way_len = max(float(np.hypot(np.diff(s["way_x"], axis=1), np.diff(s["way_y"], axis=1)).sum(axis=1).max()) for s in base)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    stream = torch.cuda.current_stream()
    rows = []
    for M in a.maps:
        if B % M:
            raise SystemExit(f"--batch {B} is no multiple of {M}")
        per = B // M
        pos = np.array([[5.0 * (k % 7), -3.0 * (k % 5)] for k in range(M)])
        layer_of = np.repeat(np.arange(M, dtype=np.int32), per)  # the instances of a map are contiguous, so (a) can pass slices
        rng = np.random.default_rng(M)
        inst = {k: np.zeros((B,) + base[0][k].shape[1:]) for k in ("way_x", "way_y", "start", "goal")}
        for k in range(M):
            s = base[k % BASE]
            pick = rng.permutation(64 * (-(-per // 64)))[:per] % 64
            sl = slice(k * per, (k + 1) * per)
            inst["way_x"][sl] = s["way_x"][pick] + pos[k, 0]; inst["way_y"][sl] = s["way_y"][pick] + pos[k, 1]
            inst["start"][sl] = s["start"][pick]; inst["start"][sl, 0] += pos[k, 0]; inst["start"][sl, 1] += pos[k, 1]
            inst["goal"][sl] = s["goal"][pick]; inst["goal"][sl, 0] += pos[k, 0]; inst["goal"][sl, 1] += pos[k, 1]
        t = {k: dev(v) for k, v in inst.items()}
        imgs = dev(occ_base[np.arange(M) % BASE])  # [M][size_y][size_x]
        dpos, dtab = dev(pos), dev(layer_of)

        def outputs():
            return dict(states=torch.zeros((B, NP, 5), dtype=torch.float64, device="cuda"), n_states=torch.zeros(B, dtype=torch.int32, device="cuda"),
                        ok=torch.zeros(B, dtype=torch.int32, device="cuda"), stage=torch.zeros(B, dtype=torch.int32, device="cuda"),
                        info=torch.zeros((B, INFO_BYTES), dtype=torch.uint8, device="cuda"))

        oa, ob = outputs(), outputs()
        torch.cuda.synchronize()
        ea, eb = binding.Engine(torch.cuda.current_device()), binding.Engine(torch.cuda.current_device())
        ea.set_stream(stream.cuda_stream); eb.set_stream(stream.cuda_stream)

        def per_map():
            for k in range(M):
                sl = slice(k * per, (k + 1) * per)
                ea.set_map_occupancy_device(imgs[k].t(), res, pos[k, 0], pos[k, 1])
                ea.plan_batch_device({n: v[sl] for n, v in t.items()}, {n: v[sl] for n, v in oa.items()}, NP, way_len)

        def stacked():
            eb.set_map_stack_occupancy_device(imgs, res, dpos)
            eb.plan_batch_device(t, ob, NP, way_len)

        eb.set_map_stack_occupancy_device(imgs, res, dpos)
        eb.set_map_assignment_device(dtab)

        def timed(fn):
            ts = []
            for i in range(a.warmup + a.calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts)), float(min(ts)), float(max(ts))

        ma, mb = timed(per_map), timed(stacked)
        same_outcome = all(torch.equal(oa[n], ob[n]) for n in ("ok", "n_states", "stage"))
        max_diff = float((oa["states"] - ob["states"]).abs().max().item())
        rows.append({"maps": M, "instances": B, "instances_per_map": per, "per_map_calls_ms": {"median": ma[0], "min": ma[1], "max": ma[2]},
                     "stack_call_ms": {"median": mb[0], "min": mb[1], "max": mb[2]}, "stack_over_per_map": mb[0] / ma[0],
                     "same_ok_n_states_stage": bool(same_outcome), "max_abs_state_diff": max_diff, "ok_frac": float(ob["ok"].double().mean().item())})
        print(json.dumps(rows[-1]), flush=True)
        ea.close(); eb.close()
    out = {"tool": "tools/map_stack_bench.py", "device": torch.cuda.get_device_name(0), "map_cells": [SX, SY], "resolution": res, "states_capacity": NP,
           "calls": a.calls, "warmup": a.warmup, "timing": "wall clock per call sequence, enqueue to the end of a device synchronisation; engine at its default parameters",
           "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
