"""Measurement (GPU): what the corridor nudge costs between po_bounds_batch and the path QP.

Shape: tools/dynamic_bench.py's — 512 groups x 8 candidates = 4 096 planning instances from the 64 seeded scenes, one map, N = 320 rows per path.
po_plan_batch_device produces the paths and po_speed_batch_device their times once; the planned paths serve as reference lines (knots: every fifth state), and
po_bounds_batch_device writes their corridors; every group gets an agent set of its own (set_of[b] = the group of b), built by dynamic_bench.agent_sets.  Then, on
a stream of its own with hipEvents around each call (median of --reps timed calls after --warmup calls), with the default parameters (po_default_nudge_params):
  nudge              po_nudge_batch_device alone on the 4 096 lines, every output asked for, for 32 and for 4 agents per set
  nudge_no_agents    the same call against empty sets: what is left is the copy of the corridor, the finiteness sweep, the frames and width_min
  nudge_all_live     32 agents per set with windows of +-1e6 s: no agent is skipped by the time test (and more pieces are live), the stage without its prefilter
and, in the same run, plan: po_plan_batch_device of the 4 096 instances, and bounds: po_bounds_batch_device.  pair_agents counts 4 n * (agents of the set) over
the processed lines and live_pair_agents the same with the agents the time test lets through (the kernel's rule, evaluated on the host): the mapping predicts a
cost proportional to the second.  Nothing is asserted and no threshold is set: numbers go to --out (default profiles/nudge/nudge_bench.json) and to stdout as
one JSON line.
    python tools/nudge_bench.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
KNOT_EVERY = 5


def knots_of(states, n_states):
    """knot_s, knot_x, knot_y [B, K] and n_knots [B]: every fifth state of each path and its last one; a path too short for a spline gets a straight stub."""
    B, N = states.shape[0], states.shape[1]
    K = (N - 1) // KNOT_EVERY + 2
    ks, kx, ky = np.zeros((B, K)), np.zeros((B, K)), np.zeros((B, K))
    nk = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = int(n_states[b])
        idx = list(range(0, n, KNOT_EVERY))
        if n > 0 and idx[-1] != n - 1 and states[b, n - 1, 4] > states[b, idx[-1], 4]:
            idx.append(n - 1)
        if len(idx) < 3:
            ks[b] = 1.5 * np.arange(K); kx[b] = ks[b]; nk[b] = K
            continue
        nk[b] = len(idx)
        ks[b, :len(idx)], kx[b, :len(idx)], ky[b, :len(idx)] = states[b, idx, 4], states[b, idx, 0], states[b, idx, 1]
        ks[b, len(idx):] = ks[b, len(idx) - 1] + 1.5 * np.arange(1, K - len(idx) + 1)
        kx[b, len(idx):], ky[b, len(idx):] = kx[b, len(idx) - 1], ky[b, len(idx) - 1]
    return ks, kx, ky, nk


def live_agents(t, n, processed, agents, first, set_of, t_before, t_after):
    """(agents of the sets, agents the kernel's time test lets through) summed over the processed lines, each weighted with the line's 4 n pairs."""
    total = live = 0
    T = agents["t"]
    npts = agents["n_pts"]
    col = np.arange(T.shape[1])[None, :]
    t_lo = np.where(col < npts[:, None], T, np.inf).min(axis=1)
    t_hi = np.where(col < npts[:, None], T, -np.inf).max(axis=1)
    before, after = (agents["flags"] & 1) != 0, (agents["flags"] & 2) != 0
    for b in np.flatnonzero(processed):
        lo, hi = first[set_of[b]], first[set_of[b] + 1]
        tmin, tmax = (t[b, :n[b]] - t_before).min(), (t[b, :n[b]] + t_after).max()
        keep = ~((~before[lo:hi] & (tmax < t_lo[lo:hi])) | (~after[lo:hi] & (tmin > t_hi[lo:hi])))
        total += 4 * int(n[b]) * int(hi - lo)
        live += 4 * int(n[b]) * int(keep.sum())
    return total, live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nudge", "nudge_bench.json"))
    a = ap.parse_args()
    import torch

    import dynamic_bench
    import select_bench
    from path_optimizer_amd import binding, synth
    from path_optimizer_amd.abi import INFO_BYTES

    if not torch.cuda.is_available():
        raise SystemExit("nudge_bench: needs the GPU (no fallback: a CPU run cannot give these times)")
    if a.reps < 20:
        raise SystemExit("nudge_bench: at least 20 timed repetitions")
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
    sp, npar = binding.default_speed_params(), binding.default_nudge_params()
    row["nudge_params"] = {f: getattr(npar, f) for f, _ in npar._fields_}
    spd_in = dict(states=plan["states"], n_states=plan["n_states"], ok=plan["ok"], v0=torch.full((B,), 5.0, dtype=torch.float64, device="cuda"))
    spd = dict(v=f64(B, N), a=f64(B, N), t=f64(B, N), total_time=f64(B), status=i32(B))
    eng.speed_batch_device(spd_in, spd, sp)
    torch.cuda.synchronize()
    states, n_states, ok = plan["states"].cpu().numpy(), plan["n_states"].cpu().numpy(), plan["ok"].cpu().numpy()
    row["plan_ok"] = int(ok.sum()); row["mean_states"] = float(n_states[ok != 0].mean()) if ok.any() else 0.0
    total_time, times = spd["total_time"].cpu().numpy(), spd["t"].cpu().numpy()

    # the planned paths as reference lines, and their corridors from the map; an instance without a usable plan becomes a straight filler line (ok = 0 keeps the
    # nudge from processing it, the bounds stage just needs something finite to read)
    usable = (ok != 0) & (n_states >= 3 * KNOT_EVERY) & np.isfinite(states).all(axis=(1, 2))
    ref = states.copy()
    ref[~usable] = 0.0
    ref[~usable, :, 0] = ref[~usable, :, 4] = 0.3 * np.arange(N)
    n_ref = np.where(usable, n_states, N).astype(np.int32)
    ks, kx, ky, nk = knots_of(ref, n_ref)
    lines = dict(ref_x=dev(ref[:, :, 0]), ref_y=dev(ref[:, :, 1]), ref_z=dev(ref[:, :, 2]), ref_s=dev(ref[:, :, 4]), n_points=dev(n_ref),
                 knot_s=dev(ks), knot_x=dev(kx), knot_y=dev(ky), n_knots=dev(nk))
    row["usable_lines"] = int(usable.sum())
    bounds, n_valid = f64(B, N, 4, 2), i32(B)
    row["bounds_ms"] = dict(ev(lambda: eng.bounds_batch_device(lines, bounds, n_valid)), what="po_bounds_batch_device, 4 096 lines")
    torch.cuda.synchronize()
    nv = n_valid.cpu().numpy()
    row["mean_valid_states"] = float(nv[ok != 0].mean()) if ok.any() else 0.0

    set_of_host = np.repeat(np.arange(G, dtype=np.int32), PER)
    set_of = dev(set_of_host)
    base_in = dict(ref_x=lines["ref_x"], ref_y=lines["ref_y"], ref_z=lines["ref_z"], n_points=n_valid, ok=dev(usable.astype(np.int32)), t=spd["t"], bounds=bounds, set_of=set_of)

    def outputs(W):
        return dict(status=i32(B), ok_out=i32(B), bounds=f64(B, N, 4, 2), side=i32(B, W), first_blocked_state=i32(B), first_blocked_agent=i32(B), width_min=f64(B))

    out = outputs(32)
    empty = dict(base_in, agents=None, first=dev(np.zeros(G + 1, dtype=np.int32)))
    row["nudge_no_agents_ms"] = dict(ev(lambda: eng.nudge_batch_device(empty, out, npar)), what="po_nudge_batch_device against empty sets: copy, sweeps, frames")
    rows = []
    for per_set in (32, 4):
        agents, first = binding.pack_agents(dynamic_bench.agent_sets(np.random.default_rng([25, per_set]), states, n_states, total_time, G, PER, per_set))
        n_in = dict(base_in, agents=dev(agents.view(np.uint8)), first=dev(first))
        out = outputs(per_set)
        r = {"agents_per_set": per_set, "sets": G, "points_per_agent": "4 .. 8", "mean_points": float(agents["n_pts"].mean())}
        r["nudge_ms"] = dict(ev(lambda: eng.nudge_batch_device(n_in, out, npar)), what="po_nudge_batch_device, 4 096 lines, every output")
        torch.cuda.synchronize()
        status, side = out["status"].cpu().numpy(), out["side"].cpu().numpy()
        r["status"] = {str(k): int((status == k).sum()) for k in (0, 1, 2, 3)}
        r["sides"] = {str(k): int((side[status > 0] == k).sum()) for k in (-1, 0, 1, 2)}
        r["pair_agents"], r["live_pair_agents"] = live_agents(times, nv, status > 0, agents, first, set_of_host, npar.t_before, npar.t_after)
        r["agents_skipped_by_the_time_test"] = 1.0 - r["live_pair_agents"] / max(r["pair_agents"], 1)
        work = r["nudge_ms"]["median"] - row["nudge_no_agents_ms"]["median"]
        r["ns_per_pair_agent"] = work * 1e6 / max(r["pair_agents"], 1)
        r["ns_per_live_pair_agent"] = work * 1e6 / max(r["live_pair_agents"], 1)
        r["nudge_over_plan"] = r["nudge_ms"]["median"] / row["plan_ms"]["median"]
        if per_set == 32:
            wide = binding.default_nudge_params()
            wide.t_before = wide.t_after = 1e6
            r["nudge_all_live_ms"] = dict(ev(lambda: eng.nudge_batch_device(n_in, out, wide)), what="windows of +-1e6 s: no agent skipped, more pieces live")
            r["ns_per_pair_agent_all_live"] = (r["nudge_all_live_ms"]["median"] - row["nudge_no_agents_ms"]["median"]) * 1e6 / max(r["pair_agents"], 1)
        rows.append(r)
    row["rows"] = rows
    row["nudge_32_over_4"] = rows[0]["nudge_ms"]["median"] / rows[1]["nudge_ms"]["median"]
    eng.set_stream(None)
    eng.close()
    for r in rows:
        print(f"[nudge_bench] {r['agents_per_set']} agents per set: nudge {r['nudge_ms']['median'] * 1e3:.0f} us (no agents {row['nudge_no_agents_ms']['median'] * 1e3:.0f} us, "
              f"plan {row['plan_ms']['median']:.2f} ms), statuses {r['status']}, sides {r['sides']}, skipped {r['agents_skipped_by_the_time_test']:.2f}", file=sys.stderr)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
