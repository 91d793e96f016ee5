"""Dev tool (GPU box): the HANDLE contract of include/po_hip.h, used the way a caller at scale uses it.
    python tools/handle_contract_check.py <scenario>
prints one `SAME <scenario>: <detail>` or `DIFFER <scenario>: <detail>` line per check and exits 0 only if nothing differed.  Every comparison is BITWISE against the
serial result of the same call on a fresh engine in this process (determinism across runs and engines is a tested property of the library: no tolerance).  Scenarios:
    shared_handle_solve   4 threads on ONE engine, each solving its own 64-path batch of config 3 twenty times (OSQP-faithful default, then the headline setting with
                          refine_chain = 2: the call that spins on a pinned word)
    shared_handle_stages  4 threads on ONE engine with a map, each looping over a different host entry (postcheck / bounds / smoothing / resample + limits); then
                          plan_batch beside smooth_batch and bounds_batch (the plan chain uses the same smoothing and bounds scratch through its device entries)
    distinct_handles      6 threads, one engine each on device 0, mixed work (KP headline, KPC N = 400, K, ragged keep 3 / N = 231, TENSION2 smoothing, postcheck)
    handle_reuse          one engine walks its grow-only scratch blocks up and down through formulations, shapes, batch sizes, an infeasible + a NaN path, B = 0; every
                          call equals what a fresh engine returns for that call alone
    graph_capture         one solve_batch_device captured into a graph on a side stream, replayed on new inputs written in place
The entries added since (the agent stages, the map family, their device twins; inputs from stage_inputs / map_inputs, which need no GPU):
    shared_handle_agent_stages    4 threads on ONE engine, one host entry each, twenty times: select / speed / dynamic / stplan, then nudge / trajectory / postcheck /
                                  densify — eight Stage layouts in one block, post_buf, a different batch size for every thread
    shared_handle_map_entries     4 threads on ONE engine with a world grid and a map stack installed: distance_map_batch / rasterize_batch / rasterize_scene_batch /
                                  map_sample_layer, all staged in edt_io
    shared_handle_device_entries  4 threads on ONE engine whose stream is a torch side stream, one device-pointer entry each on tensors of its own: select (no cost
                                  array: cost [B] lives in select_buf) / speed / dynamic / trajectory; each call is followed by a synchronisation of the stream
    handle_reuse_stages           one engine walks its map stack (obstacle lists M 3 -> a scene with the world grid M 1 -> occupancy M 2 -> the first again) and then
                                  every agent stage and densify through B 72 -> 5 -> 0 -> 72; after the first call every optional input and output is a null
                                  pointer (bare_call: the C entries with their required arrays alone); every call equals a fresh engine's
    graph_capture_stages          the chain speed -> trajectory -> dynamic -> stplan -> nudge -> select of device entries captured into ONE graph on a side stream
                                  (one stream, no fork), replayed three times on inputs written in place
Before the threads of a shared_handle_* scenario start, the main thread makes one serial call of every shape on that engine: every grow-only block has its final size, no
call can free memory another still points into.  tests/test_handle_contract.py runs each scenario in a child process of its own."""
import contextlib
import os
import re
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HEAD = dict(refine=2, refine_rounds=5, refine_extra_rounds=2, refine_eps=1e-8, refine_chain=2)
BAD = 0


def report(ok, scenario, detail):
    global BAD
    BAD += not ok
    print(("SAME " if ok else "DIFFER ") + scenario + ": " + detail, flush=True)


def engine(kw=None, dmap=None):
    from path_optimizer_amd import binding

    p = binding.default_params()
    for k, v in (kw or {}).items():
        setattr(p, k, v)
    e = binding.Engine(0, p)
    if dmap is not None:
        e.set_map(*dmap)
    return e


def flat(r):
    """A call's result (array, None, tuple or dict of such) as a list of arrays."""
    if r is None:
        return []
    if isinstance(r, dict):
        return [a for k in sorted(r) for a in flat(r[k])]
    if isinstance(r, (tuple, list)):
        return [a for x in r for a in flat(x)]
    return [np.ascontiguousarray(r)]


def same(a, b):
    fa, fb = flat(a), flat(b)
    return len(fa) == len(fb) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(fa, fb))


def fresh(fn, kw=None, dmap=None, prepare=None):
    """fn(engine) on a fresh engine: the serial reference of a call."""
    e = engine(kw, dmap)
    try:
        if prepare:
            prepare(e)
        return fn(e)
    finally:
        e.close()


def run_threads(jobs, rounds):
    """jobs: (label, call, expected, others) — call() is repeated `rounds` times on a thread of its own, all threads released together.  Returns per job the number of calls
    that differed from `expected`, how many of those equalled another job's expected result (others: label -> result; what a swapped staging block looks like), and
    the first exception."""
    barrier = threading.Barrier(len(jobs), timeout=120)
    out = [None] * len(jobs)

    def work(i):
        label, call, expected, others = jobs[i]
        bad = swapped = 0
        err = None
        try:
            barrier.wait()
            for _ in range(rounds):
                r = call()
                if not same(r, expected):
                    bad += 1
                    swapped += any(same(r, o) for o in others.values())
        except Exception as ex:  # noqa: BLE001  (reported as a DIFFER line by the caller)
            err = repr(ex)
        out[i] = (label, bad, swapped, err)

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out


def report_threads(scenario, what, res, rounds):
    for label, bad, swapped, err in res:
        report(bad == 0 and err is None, scenario, f"{what}, {label}: {rounds - bad} of {rounds} calls equal the serial result" +
               (f" ({swapped} of the {bad} others equal ANOTHER thread's serial result)" if bad else "") + (f"; exception {err}" if err else ""))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def shared_handle_solve():
    from path_optimizer_amd import synth

    name, T, rounds = "shared_handle_solve", 4, 20
    batches = [synth.make_batch(3, B=64, first_path=64 * t) for t in range(T)]
    for what, kw in (("OSQP-faithful default", {}), ("headline setting, refine_chain 2", HEAD)):
        serial = [fresh(lambda e, b=b: e.solve_batch(b, want_x=True), kw) for b in batches]
        eng = engine(kw)
        try:
            report(same(eng.solve_batch(batches[0], want_x=True), serial[0]), name, f"{what}: the sizing call on the shared engine equals the serial result")
            jobs = [(f"thread {t}", (lambda b=batches[t]: eng.solve_batch(b, want_x=True)), serial[t], {u: serial[u] for u in range(T) if u != t}) for t in range(T)]
            report_threads(name, what, run_threads(jobs, rounds), rounds)
        finally:
            eng.close()


def _stage_inputs():
    from path_optimizer_amd import synth

    sc = synth.make_planning_scenes(7, 24, near=2)
    dmap = sc["map"]
    b = synth.make_batch(3, B=64)
    st, info, _ = fresh(lambda e: e.solve_batch(b))
    paths = synth.make_spline_paths(21, 32, 160, ds=0.3)
    smooth = synth.make_smooth_inputs(21, 48, P=100, kind=0)
    sp, length, _ = synth.make_search_inputs(7, 64)
    rng = np.random.default_rng(2)
    v = rng.uniform(0, 15, (8, 50)); a = rng.uniform(-4.5, 4.5, (8, 50))
    npts = np.array([50, 50, 20, 50, 3, 50, 50, 50], dtype=np.int32)
    calls = {
        "postcheck_batch": lambda e: e.postcheck_batch(st, info),
        "bounds_batch": lambda e: e.bounds_batch(paths),
        "smooth_batch kind 0": lambda e: e.smooth_batch(0, smooth, want_raw=True),
        "resample_batch + limits_batch": lambda e: (e.resample_batch(sp, length, 0.15, 0.3, 256), e.limits_batch(v, a, npts)),
        "plan_batch": lambda e: e.plan_batch(sc["way_x"], sc["way_y"], sc["start"], sc["goal"], N=512),
    }
    return dmap, calls


def shared_handle_stages():
    name = "shared_handle_stages"
    dmap, calls = _stage_inputs()
    serial = {k: fresh(f, dmap=dmap) for k, f in calls.items()}
    for what, keys, rounds in (("four host entries", ["postcheck_batch", "bounds_batch", "smooth_batch kind 0", "resample_batch + limits_batch"], 20),
                               ("plan_batch beside smoothing and bounds", ["plan_batch", "smooth_batch kind 0", "bounds_batch"], 10)):
        eng = engine(dmap=dmap)
        try:
            for k in keys:  # sizing calls: every block at its final size before the threads start
                report(same(calls[k](eng), serial[k]), name, f"{what}: the sizing call of {k} on the shared engine equals the serial result")
            jobs = [(k, (lambda f=calls[k]: f(eng)), serial[k], {}) for k in keys]
            report_threads(name, what, run_threads(jobs, rounds), rounds)
        finally:
            eng.close()


def distinct_handles():
    from path_optimizer_amd import synth

    name, rounds = "distinct_handles", 10
    sc = synth.make_planning_scenes(7, 4)
    dmap = sc["map"]
    rag = synth.make_batch(3, B=1024, N=231, ds=0.3)
    rag.n_points = np.random.default_rng(5).integers(60, 232, size=rag.B).astype(np.int32)
    assert rag.keep == 3
    pc = synth.make_batch(3, B=1024)
    pst, pinfo, _ = fresh(lambda e: e.solve_batch(pc))
    smooth = synth.make_smooth_inputs(24, 512, P=100, kind=0)
    kp, kpc, kk = synth.make_batch(3, B=2304), synth.make_batch(5, B=512), synth.make_batch(3, B=1024, formulation=2)
    work = [("KP keep 4, headline", HEAD, None, lambda e: e.solve_batch(kp, want_x=True)),
            ("KPC N 400", {}, None, lambda e: e.solve_batch(kpc, want_x=True)),
            ("K", {}, None, lambda e: e.solve_batch(kk, want_x=True)),
            ("KP keep 3 N 231 ragged", HEAD, None, lambda e: e.solve_batch(rag, want_x=True)),
            ("TENSION2 smoothing", {}, None, lambda e: e.smooth_batch(0, smooth, want_raw=True)),
            ("postcheck", {}, dmap, lambda e: e.postcheck_batch(pst, pinfo))]
    serial = [fresh(f, kw, dm) for _, kw, dm, f in work]
    engs = [engine(kw, dm) for _, kw, dm, _ in work]
    try:
        jobs = [(label, (lambda f=f, e=e: f(e)), s, {}) for (label, _, _, f), e, s in zip(work, engs, serial)]
        report_threads(name, "one engine per thread", run_threads(jobs, rounds), rounds)
    finally:
        for e in engs:
            e.close()


def handle_reuse():
    from path_optimizer_amd import synth

    name = "handle_reuse"
    rag = synth.make_batch(3, B=33, N=100, ds=0.2 * 0.999)
    assert rag.keep == 6
    rag.n_points = np.random.default_rng(6).integers(20, 101, size=rag.B).astype(np.int32)
    odd = synth.make_batch(2, B=4, N=30)
    odd.bounds[1, 10, :, :] = [0.9, 1.0]  # a corridor that jumps 1.9 m sideways in one step: infeasible (tests/test_gpu_parity.py)
    odd.bounds[1, 11, :, :] = [-1.0, -0.9]
    odd.ref_k[2, 5] = np.nan
    first = synth.make_batch(5, B=96)
    big = synth.make_batch(3, B=2304)
    # (label, batch, newton_slice to set before the call or None).  newton_slice = 0 stays set for the calls after it: all of them are below the auto-slicing threshold,
    # so they run the one-launch Newton phase either way, and the fresh engine of each comparison is given the same switch.
    seq = [("KPC N 400 B 96", first, None), ("KP keep 4 N 200 B 2304, auto-sliced", big, None), ("KP keep 4 N 200 B 2304, newton_slice 0", big, 0),
           ("K N 130 B 7", synth.make_batch(3, B=7, N=130, formulation=2), None), ("KP keep 6 N 100 B 33 ragged", rag, None), ("one infeasible + one NaN path", odd, None),
           ("KP keep 4 N 200 B 5", synth.make_batch(3, B=5), None), ("B 0", synth.make_batch(3, B=0), None), ("KPC N 400 B 96 again", first, None)]
    for what, kw in (("default", {}), ("headline", HEAD), ("headline + polish", dict(HEAD, polish=1))):
        eng = engine(kw)
        try:
            sliced_off, results = False, []
            for label, b, sl in seq:
                if sl is not None:
                    eng.debug_set("newton_slice", sl)
                    sliced_off = True
                r = eng.solve_batch(b, want_x=True)
                results.append(r)
                ref = fresh(lambda e: e.solve_batch(b, want_x=True), kw, prepare=(lambda e: e.debug_set("newton_slice", 0)) if sliced_off else None)
                report(same(r, ref), name, f"{what}: call {len(results)} ({label}) on the reused engine equals a fresh engine's")
            report(same(results[-1], results[0]), name, f"{what}: the repeated first entry equals its first result")
        finally:
            eng.close()
    dmap = synth.make_distance_map(3, size_x=600, size_y=600, resolution=0.2, pos=(1.0, -2.0), n_obstacles=40, r_range=(0.5, 2.0))[:4]
    eng = engine(dmap=dmap)
    try:
        results = []
        for kind, P in ((0, 250), (2, 19), (1, 100), (0, 250)):
            inp = synth.make_smooth_inputs(33, 48, P=P, kind=kind)
            r = eng.smooth_batch(kind, inp, want_raw=True)
            results.append(r)
            report(same(r, fresh(lambda e: e.smooth_batch(kind, inp, want_raw=True), dmap=dmap)), name, f"smooth_batch kind {kind} P {P} on the reused engine equals a fresh engine's")
        report(same(results[-1], results[0]), name, "smooth_batch: the repeated first entry equals its first result")
    finally:
        eng.close()


def graph_capture():
    import torch

    from path_optimizer_amd import binding, synth

    name = "graph_capture"
    batches = [synth.make_batch(3, B=256, first_path=256 * i) for i in range(4)]
    fields = ("ref_x", "ref_y", "ref_z", "ref_k", "ref_s", "bounds", "x0", "goal_z")

    def outputs(db):
        return db.out_states.cpu().numpy(), db.out_x.cpu().numpy(), db.out_info.cpu().numpy()

    for what, kw in (("OSQP-faithful default", {}), ("headline setting, refine_chain 2 (treated as 3 under capture)", HEAD)):
        ref = engine(dict(kw, refine_chain=3))  # the eager reference: fully asynchronous chain
        eager = []
        for b in batches:
            d = binding.DeviceBatch(b, want_x=True)
            ref.solve_batch_device(d)
            torch.cuda.synchronize()
            eager.append(outputs(d))
        ref.close()
        s = torch.cuda.Stream()
        eng = engine(kw)
        try:
            eng.set_stream(s.cuda_stream)
            db = binding.DeviceBatch(batches[0], want_x=True)
            torch.cuda.synchronize()
            eng.solve_batch_device(db)  # warm-up: sizes every block (a handle does not allocate during capture)
            s.synchronize()
            report(same(outputs(db), eager[0]), name, f"{what}: the eager warm-up call on the side stream equals the eager reference")
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                eng.solve_batch_device(db)
            for i in (1, 2, 3):
                for f in fields:  # new inputs written in place, outputs cleared: what comes back is what the replay computed
                    getattr(db, f).copy_(torch.from_numpy(np.ascontiguousarray(getattr(batches[i], f))))
                db.out_states.zero_(); db.out_x.zero_(); db.out_info.zero_()
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                report(same(outputs(db), eager[i]), name, f"{what}: replay {i} on batch {i} equals the eager result for those inputs")
            del g
        finally:
            torch.cuda.synchronize()
            eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The entries added since the contract was written: the agent stages (all staged in post_buf), the map family (staged in edt_io), their device twins.
# Inputs are built without a GPU (tests/test_handle_contract.py runs the numpy restatements on them: every thread's results differ, few paths are "not processed").
# (entry, seed, B, N) per thread: a different B for every thread, so every Stage layout has its own offsets; N = one and two waves' worth of stations plus one.
AGENT_GROUPS = ((("select_batch", 11, 24, 65), ("speed_batch", 12, 40, 130), ("dynamic_batch", 13, 56, 65), ("stplan_batch", 14, 72, 130)),
                (("nudge_batch", 15, 32, 130), ("trajectory_batch", 16, 48, 65), ("postcheck_batch", 17, 64, 130), ("densify_batch", 18, 36, 65)))
DEVICE_THREADS = (("select_batch_device", 21, 28, 130), ("speed_batch_device", 22, 44, 65), ("dynamic_batch_device", 23, 60, 130), ("trajectory_batch_device", 24, 72, 65))
REUSE_SIZES = ((31, 72, 130), (32, 5, 130), (33, 0, 130))  # (seed, B, N) of handle_reuse_stages: B 72 -> 5 -> 0 -> 72
CAPTURE_SEEDS, CAPTURE_N = (41, 42, 43, 44), 65
STAGE_MAP = dict(seed=1, size_x=64, size_y=64, resolution=0.5, pos=(2.0, -1.0), n_obstacles=10, r_range=(0.3, 1.2))  # 32 m x 32 m: the paths start near its centre
TRAJ_K, TRAJ_DISCS = 50, 2


def agent_chunk():
    """kAgentChunk of csrc/po_agents.hpp: agents per LDS chunk of the three stages that read agents."""
    src = open(os.path.join(ROOT, "path_optimizer_amd", "csrc", "po_agents.hpp")).read()
    return int(re.search(r"constexpr int kAgentChunk = (\d+);", src).group(1))


CAPTURE_B = agent_chunk() + 1  # 2 discs a path: the records po_trajectory_batch_device writes are two sets of kAgentChunk + 1

def stage_map():
    """(dist, resolution, pos_x, pos_y) of the map the select stage reads: Engine.set_map's arguments."""
    from path_optimizer_amd import synth

    return synth.make_distance_map(**STAGE_MAP)[:4]


def _clock(s, v, t_start):
    """po_speed_batch's t for one path (tests/test_trajectory.py: clock)."""
    t = np.zeros(len(s))
    if len(s):
        t[0] = t_start
    for i in range(len(s) - 1):
        d = max(s[i + 1] - s[i], 0.0)
        vs = v[i] + v[i + 1]
        t[i + 1] = t[i] + ((2 * d) / vs if vs > 0 else 0.0)
    return t


def _walkers(rng, count, centre, box=28.0, horizon=6.0):
    """Agents with 1 .. 8 points, every flag combination, radii 0.1 .. 0.6, walking about the box within the horizon (the random_agents of the stage tests)."""
    out = []
    for _ in range(count):
        npts = int(rng.integers(1, 9))
        tt = rng.uniform(-1.0, horizon / 2) + np.concatenate(([0.0], np.cumsum(rng.uniform(0.1, horizon / 8, npts - 1))))
        x = centre[0] + rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(rng.uniform(-2, 2, npts - 1))))
        y = centre[1] + rng.uniform(-box, box) + np.concatenate(([0.0], np.cumsum(rng.uniform(-2, 2, npts - 1))))
        out.append((rng.uniform(0.1, 0.6), int(rng.integers(0, 4)), list(zip(tt, x, y))))
    return out


def _holes(rng, a, p_off, p_nan):
    """A per-state limit row as the stage tests write them: negative (no limit) and NaN entries."""
    a[rng.random(a.shape) < p_off] = -1.0
    a[rng.random(a.shape) < p_nan] = np.nan
    return a


def stage_inputs(seed, B, N):
    """Host arrays of ONE self-consistent chain for B paths of ragged length <= N (numpy alone: no GPU, and libpo_hip.so is not loaded): smooth paths inside the map of stage_map() with a speed row v
    and the times t = po_speed_batch's clock over (s, v); a group table over the B candidates with goals and previous paths; start / end speeds and per-state limits;
    two agent sets of kAgentChunk + 1 walkers and a set per path; corridor bounds and the side hints of a previous nudge; the solve statuses and lengths the
    collision-check entries read; the trajectory parameters (K = 50 samples, 2 discs) as a dict of po_trajectory_params fields."""
    from path_optimizer_amd import abi, binding

    rng = np.random.default_rng([57, seed])
    centre, A = STAGE_MAP["pos"], agent_chunk() + 1
    st, v, t = np.zeros((B, N, 5)), np.zeros((B, N)), np.zeros((B, N))
    for b in range(B):
        step = 0.2 * rng.uniform(0.7, 1.3, N - 1)
        s = np.concatenate(([0.0], np.cumsum(step)))
        k = rng.uniform(0, 0.15) * np.sin(s / rng.uniform(3, 9) + rng.uniform(0, 6.28)) + rng.uniform(-0.03, 0.03)
        z = rng.uniform(-np.pi, np.pi) + np.concatenate(([0.0], np.cumsum(0.5 * (k[1:] + k[:-1]) * step)))
        x = centre[0] + rng.uniform(-3, 3) + np.concatenate(([0.0], np.cumsum(np.cos(z[:-1]) * step)))
        y = centre[1] + rng.uniform(-3, 3) + np.concatenate(([0.0], np.cumsum(np.sin(z[:-1]) * step)))
        st[b] = np.stack([x, y, z, k, s], axis=1)
        v[b] = rng.uniform(0.5, 6, N)
        v[b, rng.random(N) < 1 / 7] = 0.0
        t[b] = _clock(s, v[b], rng.uniform(-0.5, 0.5))
    n = rng.integers(0, N + 1, B).astype(np.int32)
    ok = (rng.random(B) >= 1 / 8).astype(np.int32)
    if B:
        n[rng.integers(0, B)] = N
    sizes = []
    while sum(sizes) < B:
        sizes.append(min(int(rng.integers(1, 10)), B - sum(sizes)))
    gs = np.concatenate(([0], np.cumsum(sizes or [0]))).astype(np.int32)
    G = len(gs) - 1
    prev = np.zeros((G, 7, 5))
    for g in range(G):
        if gs[g] < B:
            prev[g] = st[gs[g], ::max(N // 7, 1)][:7] + 0.1
    ends = [t[b, max(int(n[b]) - 1, 0)] for b in range(B)]
    t_lo = float(t[:, 0].min()) - 0.3 if B else 0.0
    return dict(
        B=B, N=N, states=st, n_states=n, ok=ok, v=v, t=t,
        group_start=gs, goal=st[:, N // 2, :3] + 0.3, prev_states=prev, prev_n=rng.integers(0, 8, G).astype(np.int32),
        v0=rng.uniform(0, 6, B), v_end=_holes(rng, rng.uniform(0, 4, B), 0.3, 0.1), v_limit=_holes(rng, rng.uniform(1, 9, (B, N)), 0.6, 0.1),
        v_cap=_holes(rng, rng.uniform(2, 9, (B, N)), 0.4, 0.1), v_limit_in=_holes(rng, rng.uniform(1, 9, (B, N)), 0.4, 0.1),
        agents=binding.pack_agents([_walkers(rng, A, centre), _walkers(rng, A, centre)]), set_of=rng.integers(0, 2, B).astype(np.int32),
        bounds=np.stack([-rng.uniform(1, 3, (B, N, 4)), rng.uniform(1, 3, (B, N, 4))], axis=-1), side_prev=rng.integers(-1, 3, (B, A)).astype(np.int32),
        solved=np.where(rng.random(B) >= 1 / 8, 1, -10).astype(np.int32), n_points=np.clip(n, 8, N).astype(np.int32),
        trajectory=dict(t0=t_lo, dt=max(1.2 * (float(np.median(ends)) - t_lo), 0.5) / (TRAJ_K - 1) if B else 0.1, K=TRAJ_K, n_discs=TRAJ_DISCS, disc_offset=[-0.5, 0.75],
                        disc_radius=[1.25, 1.0], agent_pts=8, agent_stride=(TRAJ_K - 1) // 7, agent_flags=abi.PO_AGENT_HOLD_AFTER))


def stage_params(c=None, full=True):
    """The parameter structs of the stages (the defaults come from libpo_hip.so, which must be built; no GPU), as the library fills them except where noted: select without a clearance threshold (tests/test_select.py does the same:
    most candidates stay feasible), the station-time search at the small size of tests/test_stplan.py, the trajectory of c (without `full`: no discs, so no records)."""
    from path_optimizer_amd import binding

    p = dict(select=binding.default_select_params(), speed=binding.default_speed_params(), dynamic=binding.default_dynamic_params(),
             stplan=binding.default_stplan_params(), nudge=binding.default_nudge_params(), trajectory=binding.default_trajectory_params())
    p["select"].min_clearance = -10.0
    for k, val in dict(dt=0.5, K=5, stride=2, U=6, margin=0.4).items():
        setattr(p["stplan"], k, val)
    for k, val in ((c or {}).get("trajectory") or {}).items():
        if k in ("disc_offset", "disc_radius"):
            for j, x in enumerate(val):
                getattr(p["trajectory"], k)[j] = x
        else:
            setattr(p["trajectory"], k, val)
    if not full:
        p["trajectory"].n_discs = 0
    return p


def _info(c):
    from path_optimizer_amd import abi

    info = np.zeros(c["B"], dtype=abi.INFO_DTYPE)
    info["status"] = c["solved"]
    return info


def bare_call(entry, e, c, P):
    """The C entry of a stage itself with its REQUIRED arrays alone (Engine.*_batch always hands over most optional outputs): every optional input and every
    optional output is a null pointer, so its Stage declares none of the slots the larger call declared.  Required, from the argument checks of po_capi.cpp:
    select: states, group_start -> best (without a cost array the device twin keeps cost [B] in select_buf); dynamic: states, t, the lists -> status; stplan:
    states, v0, the lists -> status; nudge: ref_x, ref_y, ref_z, t, bounds, the lists -> status, bounds (W = 0: no side columns); trajectory: states, v, t ->
    status, states (P has no discs then: with n_discs > 0 the records are required)."""
    import ctypes

    from path_optimizer_amd import abi, binding

    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    B, N, st = c["B"], c["N"], f64(c["states"])
    ag, first = c["agents"]
    lists = abi.PoAgentLists(p(ag), p(first), len(ag), len(first) - 1)
    status = np.full(B, -7, dtype=np.int32)
    stage = entry.split("_")[0]
    if stage == "select":
        gs = np.ascontiguousarray(c["group_start"], dtype=np.int32)
        r = {"best": np.full(len(gs) - 1, -7, dtype=np.int32)}
        held = (gs,)
        si, so = abi.PoSelectIn(B, N, p(st), None, None, None, 0, len(gs) - 1, p(gs), 0, None, None), abi.PoSelectOut(None, None, p(r["best"]), None, None, None, None)
    elif stage == "dynamic":
        r, held = {"status": status}, (f64(c["t"]),)
        si, so = abi.PoDynamicIn(B, N, p(st), None, None, p(held[0]), None, ctypes.pointer(lists), None), abi.PoDynamicOut(p(status), *[None] * 8)
    elif stage == "stplan":
        r, held = {"status": status}, (f64(c["v0"]),)
        si, so = abi.PoStplanIn(B, N, p(st), None, None, p(held[0]), None, None, ctypes.pointer(lists), None), abi.PoStplanOut(p(status), *[None] * 6)
    elif stage == "nudge":
        r = {"status": status, "bounds": np.full((B, N, 4, 2), -7.0)}
        held = x, y, z, t, bnd = f64(st[:, :, 0]), f64(st[:, :, 1]), f64(st[:, :, 2]), f64(c["t"]), f64(c["bounds"])
        si = abi.PoNudgeIn(B, N, 0, p(x), p(y), p(z), None, None, p(t), p(bnd), None, ctypes.pointer(lists), None)
        so = abi.PoNudgeOut(p(status), None, p(r["bounds"]), None, None, None, None)
    elif stage == "trajectory":
        assert P["trajectory"].n_discs == 0
        r = {"status": status, "states": np.full((B, int(P["trajectory"].K), 5), -7.0)}
        held = v, t = f64(c["v"]), f64(c["t"])
        si, so = abi.PoTrajectoryIn(B, N, p(st), None, None, p(v), p(t)), abi.PoTrajectoryOut(p(status), p(r["states"]), *[None] * 6)
    else:
        raise KeyError(entry)
    binding._check(getattr(binding.lib(), "po_" + entry)(e._h, ctypes.byref(P[stage]), ctypes.byref(si), ctypes.byref(so)))
    del held  # (the structs store bare addresses: the arrays live until the call has returned)
    return r


def host_call(entry, e, c, full=True):
    """One host-pointer entry on the inputs c.  full: every optional input and output.  Else none of them: the five stages with optional outputs that Engine.*_batch
    cannot leave out go through bare_call; speed keeps v, a and status, postcheck and densify have no optional output (their n_points is dropped)."""
    P = stage_params(c, full)
    o = (lambda *keys: {k: c[k] for k in keys}) if full else (lambda *keys: {})
    if not full and entry in ("select_batch", "dynamic_batch", "stplan_batch", "nudge_batch", "trajectory_batch"):
        return bare_call(entry, e, c, P)
    if entry == "select_batch":
        return e.select_batch(c["states"], c["group_start"], params=P["select"], **o("n_states", "ok", "goal", "prev_states", "prev_n"))
    if entry == "speed_batch":
        return e.speed_batch(c["states"], c["v0"], params=P["speed"], want_t=full, **o("n_states", "ok", "v_end", "v_limit"))
    if entry == "dynamic_batch":
        return e.dynamic_batch(c["states"], c["t"], c["agents"], params=P["dynamic"], **o("n_states", "ok", "set_of", "v_limit_in"))
    if entry == "stplan_batch":
        return e.stplan_batch(c["states"], c["v0"], c["agents"], params=P["stplan"], **o("n_states", "ok", "v_cap", "set_of", "v_limit_in"))
    if entry == "nudge_batch":
        st = c["states"]
        return e.nudge_batch(st[:, :, 0], st[:, :, 1], st[:, :, 2], c["t"], c["bounds"], c["agents"], params=P["nudge"], n_points=c["n_states"], ok=c["ok"], set_of=c["set_of"],
                             side_prev=c["side_prev"])
    if entry == "trajectory_batch":
        return e.trajectory_batch(c["states"], c["v"], c["t"], params=P["trajectory"], n_states=c["n_states"], ok=c["ok"])
    if entry == "postcheck_batch":
        return e.postcheck_batch(c["states"], _info(c), **o("n_points"))
    if entry == "densify_batch":
        return e.densify_batch(c["states"], _info(c), 2 * c["N"], **o("n_points"))
    raise KeyError(entry)


def shared_handle_agent_stages():
    name, rounds = "shared_handle_agent_stages", 20
    dmap = stage_map()
    for gi, group in enumerate(AGENT_GROUPS):
        what = f"group {gi + 1}"
        cases = {entry: stage_inputs(seed, B, N) for entry, seed, B, N in group}
        serial = {k: fresh(lambda e, k=k: host_call(k, e, cases[k]), dmap=dmap) for k in cases}
        eng = engine(dmap=dmap)
        try:
            for k in cases:  # sizing calls: post_buf at its final size before the threads start
                report(same(host_call(k, eng, cases[k]), serial[k]), name, f"{what}: the sizing call of {k} (B {cases[k]['B']}, N {cases[k]['N']}) on the shared engine equals the serial result")
            jobs = [(k, (lambda k=k: host_call(k, eng, cases[k])), serial[k], {u: serial[u] for u in cases if u != k}) for k in cases]
            report_threads(name, what, run_threads(jobs, rounds), rounds)
        finally:
            eng.close()


# ---- the map family: everything staged in edt_io ----
MAP_RES = 0.2


def map_inputs(seed, M, sx, sy):
    """Host inputs of the map entries for M layers of sx x sy cells (numpy and the binding's packers: no GPU, and libpo_hip.so is not loaded): layer centres, obstacle lists (6 discs + 3 boxes a layer, inside and across
    the borders: tests/test_scene.py small_lists), a base image, rings (one FREE star every layer shares, one SOLID star a layer), occupancy images with 3 % of
    the cells occupied, and sample points in and around the last layer."""
    from path_optimizer_amd import abi, binding

    rng = np.random.default_rng([58, seed])
    res, wx, wy = MAP_RES, sx * MAP_RES, sy * MAP_RES
    pos = rng.uniform(-1.5, 1.5, (M, 2))
    rmax = max(0.08 * max(wx, wy), 2.0 * res)

    def star(cx, cy, rmin, rmax_, n):
        ang, r = np.sort(rng.uniform(0, 2 * np.pi, n)), rng.uniform(rmin, rmax_, n)
        return np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], axis=1)

    layers, own = [], []
    for k in range(M):
        at = lambda: (pos[k][0] + rng.uniform(-0.55, 0.55) * wx, pos[k][1] + rng.uniform(-0.55, 0.55) * wy)
        layers.append([binding.obstacle_disc(*at(), rng.uniform(0.3 * res, rmax)) for _ in range(6)]
                      + [binding.obstacle_box(*at(), rng.uniform(0.3 * res, rmax), rng.uniform(0.3 * res, 0.6 * rmax), rng.uniform(-np.pi, np.pi)) for _ in range(3)])
        own.append([(star(*at(), 0.05 * wx, 0.2 * wx, int(rng.integers(5, 13))), abi.PO_RING_SOLID)])
    hub = pos.mean(axis=0)
    shared = [(star(hub[0], hub[1], 0.35 * max(wx, wy), 0.8 * max(wx, wy), 24), abi.PO_RING_FREE)]
    xy = pos[M - 1] + rng.uniform(-0.6, 0.6, (200, 2)) * (wx, wy)
    return dict(M=M, sx=sx, sy=sy, res=res, pos=pos, layers=layers, rings=binding.pack_rings(shared, own), base=(rng.random((sx, sy)) >= 0.03).astype(np.uint8) * 255,
                occ=(rng.random((M, sx, sy)) >= 0.03).astype(np.uint8) * 255, xy=xy)


def world_inputs():
    """The site's static grid of the scene entries: set_world_occupancy's arguments (another resolution and centre than any layer)."""
    rng = np.random.default_rng([59, 1])
    return (rng.random((64, 48)) >= 0.3).astype(np.uint8) * 255, 0.3, 0.3, -0.2, False


def map_call(entry, e, m):
    if entry == "distance_map_batch":
        return e.distance_map_batch(m["occ"], m["res"])
    if entry == "rasterize_batch":
        return e.rasterize_batch(m["layers"], m["sx"], m["sy"], m["res"], m["pos"], base=m["base"])
    if entry == "rasterize_scene_batch":
        return e.rasterize_scene_batch(m["layers"], m["rings"], m["sx"], m["sy"], m["res"], m["pos"], use_world=True)
    if entry == "map_sample_layer":
        return e.map_sample_layer(m["M"] - 1, m["xy"])
    if entry == "set_map_stack_obstacles":
        e.set_map_stack_obstacles(m["layers"], m["sx"], m["sy"], m["res"], m["pos"])
    elif entry == "set_map_stack_scene":
        e.set_map_stack_scene(m["layers"], m["rings"], m["sx"], m["sy"], m["res"], m["pos"], use_world=True)
    elif entry == "set_map_stack_occupancy":
        e.set_map_stack_occupancy(m["occ"], m["res"], m["pos"])
    else:
        raise KeyError(entry)
    return [e.get_map_layer(k) for k in range(m["M"])]


def shared_handle_map_entries():
    name, what, rounds = "shared_handle_map_entries", "the edt_io family", 20
    stack = map_inputs(5, 3, 64, 64)
    cases = {"distance_map_batch": map_inputs(1, 3, 64, 64), "rasterize_batch": map_inputs(2, 2, 63, 40), "rasterize_scene_batch": map_inputs(3, 3, 40, 64),
             "map_sample_layer": stack}

    def install(e):  # the world grid and the stack: before the threads start (installing either from a racing thread is outside the guarantee)
        e.set_world_occupancy(*world_inputs())
        map_call("set_map_stack_obstacles", e, stack)

    serial = {k: fresh(lambda e, k=k: map_call(k, e, cases[k]), prepare=install) for k in cases}
    eng = engine()
    try:
        install(eng)
        for k in cases:
            report(same(map_call(k, eng, cases[k]), serial[k]), name, f"{what}: the sizing call of {k} on the shared engine equals the serial result "
                   f"(distinct values per output array: {[len(np.unique(a)) for a in flat(serial[k])]})")
        jobs = [(k, (lambda k=k: map_call(k, eng, cases[k])), serial[k], {u: serial[u] for u in cases if u != k}) for k in cases]
        report_threads(name, what, run_threads(jobs, rounds), rounds)
    finally:
        eng.close()


# ---- the device-pointer entries of the stages ----
def _dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_out(shapes):
    import torch

    return {k: torch.zeros(shape, dtype=getattr(torch, ty), device="cuda") for k, (shape, ty) in shapes.items()}


def _records(c):
    ag, first = c["agents"]
    return {"agents": _dev(ag.view(np.uint8)), "first": _dev(first)}


def device_outputs(entry, c, P):
    """Zeroed output tensors of one device-pointer entry, every optional one included but the cost array of select: it keeps cost [B] in select_buf then."""
    B, N, G = c["B"], c["N"], len(c["group_start"]) - 1
    K, D, W = int(P["trajectory"].K), int(P["trajectory"].n_discs), agent_chunk() + 1
    f, i = "float64", "int32"
    rows = {"select": {"feat": ((B, 8), f), "best": ((G,), i), "best_cost": ((G,), f), "n_feasible": ((G,), i), "sel_states": ((G, N, 5), f), "sel_n": ((G,), i)},
            "speed": {"v": ((B, N), f), "a": ((B, N), f), "t": ((B, N), f), "total_time": ((B,), f), "status": ((B,), i)},
            "dynamic": {"status": ((B,), i), "ok_out": ((B,), i), "gap_min": ((B,), f), "first_state": ((B,), i), "first_agent": ((B,), i), "stop_state": ((B,), i),
                        "first_time": ((B,), f), "gap": ((B, N), f), "v_limit": ((B, N), f)},
            "stplan": {"status": ((B,), i), "ok_out": ((B,), i), "n_layers": ((B,), i), "cost": ((B,), f), "station": ((B, 17), i),
                       "cells": ((B, int(P["stplan"].K), 128), i), "v_limit": ((B, N), f)},
            "nudge": {"status": ((B,), i), "ok_out": ((B,), i), "bounds": ((B, N, 4, 2), f), "side": ((B, W), i), "first_blocked_state": ((B,), i),
                      "first_blocked_agent": ((B,), i), "width_min": ((B,), f)},
            "trajectory": {"status": ((B,), i), "states": ((B, K, 5), f), "v": ((B, K), f), "a": ((B, K), f), "t": ((B, K), f), "index": ((B, K), i),
                           "first_held": ((B,), i), "agents": ((B * D * 208,), "uint8")}}
    return _dev_out(rows[entry.split("_")[0]])


def device_tensors(entry, c, P):
    """(inputs, outputs) of one device-pointer entry as torch tensors on the current device."""
    keys = {"select": ("states", "group_start", "n_states", "ok", "goal", "prev_states", "prev_n"), "speed": ("states", "v0", "n_states", "ok", "v_end", "v_limit"),
            "dynamic": ("states", "t", "n_states", "ok", "set_of", "v_limit_in"), "trajectory": ("states", "v", "t", "n_states", "ok")}[entry.split("_")[0]]
    t = {k: _dev(c[k]) for k in keys}
    if entry == "dynamic_batch_device":
        t.update(_records(c))
    return t, device_outputs(entry, c, P)


def device_call(entry, e, t, out, P, stream=None):
    """Clear the outputs, enqueue the entry, synchronise, return host copies of the outputs: what comes back is what this call computed.  stream: the torch side
    stream the engine runs on (the clearing is ordered on it too); None: the engine's own stream, ordered by device-wide synchronisation."""
    import torch

    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        for o in out.values():
            o.zero_()
        if stream is None:
            torch.cuda.synchronize()
        getattr(e, entry)(t, out, P[entry.split("_")[0]])
        stream.synchronize() if stream is not None else torch.cuda.synchronize()
        return {k: o.cpu().numpy() for k, o in out.items()}


def shared_handle_device_entries():
    import torch

    name, what, rounds = "shared_handle_device_entries", "device entries on a side stream", 20
    dmap = stage_map()
    cases = {entry: stage_inputs(seed, B, N) for entry, seed, B, N in DEVICE_THREADS}
    params = {k: stage_params(cases[k]) for k in cases}

    def alone(e, k):
        t, out = device_tensors(k, cases[k], params[k])
        torch.cuda.synchronize()
        return device_call(k, e, t, out, params[k])

    serial = {k: fresh(lambda e, k=k: alone(e, k), dmap=dmap) for k in cases}
    s = torch.cuda.Stream()
    eng = engine(dmap=dmap)
    try:
        eng.set_stream(s.cuda_stream)
        tensors = {k: device_tensors(k, cases[k], params[k]) for k in cases}  # every thread's own tensors, complete before the barrier
        torch.cuda.synchronize()
        for k in cases:  # sizing calls: select_buf holds the group table and cost [B] before the threads start
            report(same(device_call(k, eng, *tensors[k], params[k], stream=s), serial[k]), name, f"{what}: the sizing call of {k} (B {cases[k]['B']}) on the shared engine equals the serial result")
        jobs = [(k, (lambda k=k: device_call(k, eng, *tensors[k], params[k], stream=s)), serial[k], {u: serial[u] for u in cases if u != k}) for k in cases]
        report_threads(name, what, run_threads(jobs, rounds), rounds)
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---- reuse: the blocks the newer entries grow, walked large -> small -> large ----
REUSE_STAGES = ("select_batch", "speed_batch", "dynamic_batch", "stplan_batch", "nudge_batch", "trajectory_batch", "densify_batch")


def handle_reuse_stages():
    name = "handle_reuse_stages"
    world = world_inputs()
    first, small, occ = map_inputs(6, 3, 64, 64), map_inputs(7, 1, 40, 24), map_inputs(8, 2, 64, 64)
    walk = [("the first stack: M 3, 64 x 64, from obstacle lists", "set_map_stack_obstacles", first), ("a smaller stack: M 1, 40 x 24, from a scene with the world grid", "set_map_stack_scene", small),
            ("an occupancy stack: M 2, 64 x 64", "set_map_stack_occupancy", occ), ("the first stack again", "set_map_stack_obstacles", first)]
    dmap = stage_map()
    eng = engine()
    try:
        eng.set_world_occupancy(*world)
        results = []
        for label, entry, m in walk:
            results.append(map_call(entry, eng, m))
            ref = fresh(lambda e: map_call(entry, e, m), prepare=lambda e: e.set_world_occupancy(*world))
            report(same(results[-1], ref), name, f"{label}: every layer read back from the reused engine equals a fresh engine's")
        report(same(results[-1], results[0]), name, "the repeated first stack equals its first result")
        eng.set_map(*dmap)  # the map the select stage reads (one layer again: the stack shrinks once more)
        big, five, none = (stage_inputs(*a) for a in REUSE_SIZES)
        steps = [("B 72", big, True), ("B 5, no optional array", five, False), ("B 0", none, False), ("B 72, no optional array", big, False), ("B 72 again", big, True)]
        firsts = {}
        for label, c, full in steps:  # size-major: every stage at one size, then every stage at the next: eight layouts follow one another in post_buf
            for k in REUSE_STAGES:
                r = host_call(k, eng, c, full)
                report(same(r, fresh(lambda e: host_call(k, e, c, full), dmap=dmap)), name, f"{k}, {label}: the reused engine equals a fresh engine's")
                if label == "B 72":
                    firsts[k] = r
                elif label == "B 72 again":
                    report(same(r, firsts[k]), name, f"{k}: the repeated first call equals its first result")
    finally:
        eng.close()


# ---- capture: a fleet cycle of the device entries as one graph ----
CAPTURE_MAP = dict(seed=3, size_x=64, size_y=64, resolution=1.0, pos=(10.0, -5.0), n_obstacles=10)  # 64 m x 64 m around the fleet
CAPTURE_PITCH = 7.0


def capture_inputs(seed):
    """stage_inputs as a FLEET (no GPU): the paths of stage_inputs(seed, kAgentChunk + 1, 65), about 13 m long, moved onto a 7 x 5 grid of starting areas 7 m apart inside the
    map of CAPTURE_MAP, so that some vehicles cross another's way and others meet nobody; every path at full length or nearly; a group table of threes.  The
    records po_trajectory_batch_device writes (2 discs a path) are read as two sets of kAgentChunk + 1: path b meets the set its own discs are not in (but for the
    path in the middle, whose discs straddle the two)."""
    c = stage_inputs(seed, CAPTURE_B, CAPTURE_N)
    B, N = c["B"], c["N"]
    assert B <= 35  # the grid below; a larger chunk needs a larger one (and a larger CAPTURE_MAP)
    b = np.arange(B)
    shift = np.stack([8.0 + CAPTURE_PITCH * (b % 7 - 3), -4.0 + CAPTURE_PITCH * (b // 7 - 2)], axis=1)
    st = c["states"].copy()
    st[:, :, :2] += shift[:, None, :]
    goal = c["goal"].copy()
    goal[:, :2] += shift
    first = np.array([0, B * TRAJ_DISCS // 2, B * TRAJ_DISCS], dtype=np.int32)
    return dict(c, states=st, goal=goal, n_states=np.maximum(c["n_states"], N - 8).astype(np.int32), group_start=np.arange(0, B + 1, 3, dtype=np.int32), first=first,
                set_of=(b * TRAJ_DISCS < first[1]).astype(np.int32))


def capture_params(c):
    """One horizon for every replay (the parameters are fixed at capture): 50 samples over 2.45 s from t = 0, where po_speed_batch starts its clock."""
    return stage_params(dict(trajectory=dict(c["trajectory"], t0=0.0, dt=0.05)))


def capture_tensors(c, P):
    """The tensors of the chain speed -> trajectory (records out) -> dynamic (against those records) -> stplan -> nudge -> select: inputs from c (capture_inputs),
    outputs zeroed."""
    st = c["states"]
    inp = {k: _dev(v) for k, v in dict(states=st, ref_x=st[:, :, 0], ref_y=st[:, :, 1], ref_z=st[:, :, 2], v0=c["v0"], n_states=c["n_states"], bounds=c["bounds"], goal=c["goal"],
                                       group_start=c["group_start"], first=c["first"], set_of=c["set_of"]).items()}
    return inp, {k: device_outputs(k, c, P) for k in CHAIN}


CHAIN = ("speed_batch_device", "trajectory_batch_device", "dynamic_batch_device", "stplan_batch_device", "nudge_batch_device", "select_batch_device")


def chain(e, inp, out, P):
    """Six device entries on the engine's stream, nothing in between: plan A's trajectory is plan B's agent; the yield limits of the conflict check go into the
    station-time search; the corridors are carved around the same records; the candidates whose corridor is blocked are not selected."""
    sp, tr, dy, stp, nd, sel = (out[k] for k in CHAIN)
    path = {"states": inp["states"], "n_states": inp["n_states"]}
    lists = {"agents": tr["agents"], "first": inp["first"], "set_of": inp["set_of"]}
    e.speed_batch_device(dict(path, v0=inp["v0"]), sp, P["speed"])
    e.trajectory_batch_device(dict(path, v=sp["v"], t=sp["t"]), tr, P["trajectory"])
    e.dynamic_batch_device(dict(path, **lists, t=sp["t"]), dy, P["dynamic"])
    e.stplan_batch_device(dict(path, **lists, v0=inp["v0"], v_limit_in=dy["v_limit"]), stp, P["stplan"])
    e.nudge_batch_device(dict(lists, ref_x=inp["ref_x"], ref_y=inp["ref_y"], ref_z=inp["ref_z"], t=sp["t"], bounds=inp["bounds"], n_points=inp["n_states"]), nd, P["nudge"])
    e.select_batch_device(dict(path, group_start=inp["group_start"], goal=inp["goal"], ok=nd["ok_out"]), sel, P["select"])


def graph_capture_stages():
    import torch

    name = "graph_capture_stages"
    from path_optimizer_amd import synth

    dmap = synth.make_distance_map(**CAPTURE_MAP)[:4]
    cases = [capture_inputs(seed) for seed in CAPTURE_SEEDS]
    P = capture_params(cases[0])
    host = lambda out: {k: {f: o.cpu().numpy() for f, o in out[k].items()} for k in CHAIN}
    eager = []
    ref = engine(dmap=dmap)  # the eager reference: the chain on a fresh engine's own stream
    for c in cases:
        inp, out = capture_tensors(c, P)
        torch.cuda.synchronize()
        chain(ref, inp, out, P)
        torch.cuda.synchronize()
        eager.append(host(out))
    ref.close()
    s = torch.cuda.Stream()
    eng = engine(dmap=dmap)
    try:
        eng.set_stream(s.cuda_stream)
        inp, out = capture_tensors(cases[0], P)
        torch.cuda.synchronize()
        chain(eng, inp, out, P)  # warm-up: select_buf gets its size (a handle does not allocate during capture)
        s.synchronize()
        got = host(out)
        for k in CHAIN:
            report(same(got[k], eager[0][k]), name, f"the eager warm-up chain on the side stream, {k}: equals the eager reference")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            chain(eng, inp, out, P)
        for i in (1, 2, 3):
            new, _ = capture_tensors(cases[i], P)
            for k in inp:  # new inputs written in place, outputs cleared: what comes back is what the replay computed
                inp[k].copy_(new[k])
            for o in out.values():
                for v in o.values():
                    v.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = host(out)
            for k in CHAIN:
                st = got[k].get("status")
                report(same(got[k], eager[i][k]), name, f"replay {i} on inputs {i}, {k}: equals the eager result for those inputs" +
                       (f" ({int((got[k]['best'] >= 0).sum())} of {len(got[k]['best'])} groups have a winner)" if st is None else f" (statuses {np.bincount(st, minlength=4).tolist()})"))
        del g
    finally:
        torch.cuda.synchronize()
        eng.close()


SCENARIOS = {f.__name__: f for f in (shared_handle_solve, shared_handle_stages, distinct_handles, handle_reuse, graph_capture, shared_handle_agent_stages,
                                     shared_handle_map_entries, shared_handle_device_entries, handle_reuse_stages, graph_capture_stages)}

if __name__ == "__main__":
    if len(sys.argv) != 2 or sys.argv[1] not in SCENARIOS:
        sys.exit("usage: handle_contract_check.py " + " | ".join(SCENARIOS))
    import torch  # noqa: F401  (one HIP runtime for both libraries)

    try:
        SCENARIOS[sys.argv[1]]()
    except Exception as ex:  # noqa: BLE001
        report(False, sys.argv[1], f"exception {ex!r}")
    print("checks that differ:", BAD)
    sys.exit(1 if BAD else 0)
