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
Before the threads of a shared_handle_* scenario start, the main thread makes one serial call of every shape on that engine: every grow-only block has its final size, no
call can free memory another still points into.  tests/test_handle_contract.py runs each scenario in a child process of its own."""
import os
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


SCENARIOS = {f.__name__: f for f in (shared_handle_solve, shared_handle_stages, distinct_handles, handle_reuse, graph_capture)}

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
