"""Newton refinement (po_params.refine = 2, round 4): semismooth Newton on the augmented Lagrangian with a line search on the merit (safeguarded Newton on its piecewise-linear derivative), from the point a SHORT
type-based ADMM run stops at (include/po_hip.h).  It replaced the activity-weighted ADMM continuation (refine = 1, removed in round 5) as the setting `value` is quoted at:
globally convergent (the merit falls monotonically), so the activity set cannot cycle — the failure mode that left ~0.3 % of BASELINE config 3 at
1 500 – 1 900 iterations and four KPC paths of config 5 uncertified.

CPU: the oracle's implementation (oracle/po_oracle.c, `refine == 2`) against the exact optima of every BASELINE shape (tests/golden/tight_full_*.npz).
GPU: the device's (csrc/po_fast.inc, refine_phase_newton in newton_kernel / newton_fallback_kernel) against the oracle's — same Newton step counts, same points —
and against the exact optima."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_tight_full import batch_of, e_y_of, load_tight_full  # noqa: E402

# the setting `value` is quoted at (bench.py HEADLINE): the Newton phase is entered as soon as OSQP's test holds at 1e4 x eps (= the first check, 25 iterations)
NEWTON = dict(refine=2, refine_rounds=5, refine_extra_rounds=2, refine_eps=1e-8, refine_chain=2)


def _set(p, **kw):
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _gold(name, nb):
    return load_tight_full(name)["e_y"].astype(np.float64)[:nb]


def _rms(batch, xs, gold):
    ey = np.stack([e_y_of(batch.formulation, batch.N, xs[b]) for b in range(len(xs))])
    return np.sqrt(np.mean((ey - gold) ** 2, axis=1))


def test_oracle_newton_defaults(oracle):
    p = oracle.default_params()
    assert (p.refine_newton_rho, p.refine_newton_rho_eq, p.refine_newton_rho_max, p.refine_ls_tol, p.refine_ls_max, p.refine_newton_max, p.refine_newton_final, p.refine_newton_rho_eq_max, p.refine_newton_escalate) == (100.0, 1e4, 1e5, 0.6, 30, 300, 3, 1e6, 12)


@pytest.mark.parametrize("name,B", [("c3", 512), ("c2", 256), ("c5", 96), ("k", 128), ("keep3", 128)])
def test_oracle_newton_certifies_every_path_at_the_exact_optimum(oracle, name, B):
    b = batch_of(name, B)
    p = _set(oracle.device_equivalent_params(), **NEWTON)
    _, info, xs = oracle.solve_batch(b, p)
    assert (info["status"] == 1).all() and (info["status_refine"] == 1).all()
    r = _rms(b, xs, _gold(name, B))
    assert r.max() < 5e-5, r.max()                       # the bar is 1e-4 m; measured on the whole batches: 2.1e-5 (config 3 and config 5)
    assert info["iters"].mean() < 70                     # 25 ADMM iterations + Newton steps (a step counts as one iteration)
    assert (info["r_prim"] < 1e-6).all() and (info["r_dual"] < 1e-5).all()


def test_oracle_newton_on_the_paths_the_activity_weighted_refinement_cycled_on(oracle):
    """BASELINE config 3, the paths on which round 3's refine = 1 cycled (1 500 - 1 900 iterations each; removed in round 5): tens of Newton steps."""
    hard = [2410, 3341, 2637, 539, 460, 3877, 1178, 3261, 1857]
    gold = load_tight_full("c3")["e_y"].astype(np.float64)
    p2 = _set(oracle.device_equivalent_params(), **NEWTON)
    for pid in hard:
        b = batch_of("c3", 1, pid)
        _, i2, x2 = oracle.solve_batch(b, p2)
        assert i2["status"][0] == 1 and i2["status_refine"][0] == 1 and i2["iters"][0] <= 100, (pid, i2)
        assert _rms(b, x2, gold[pid:pid + 1])[0] < 3e-5


def test_oracle_newton_failed_attempt_falls_back_to_the_rounds(oracle):
    """An attempt that runs out of its Newton budget hands the path back to the type-based iteration at the next round's eps, like refine = 1."""
    b = batch_of("c3", 8)
    p = _set(oracle.device_equivalent_params(), **NEWTON)
    p.refine_newton_max = 3  # (nothing certifies in 3 steps from the 25-iteration point)
    _, info, xs = oracle.solve_batch(b, p)
    assert (info["status"] == 1).all()
    q = _set(oracle.device_equivalent_params(), **NEWTON)
    _, i2, _ = oracle.solve_batch(b, q)
    assert (i2["iters"] <= info["iters"]).all() and info["iters"].mean() > 2 * i2["iters"].mean()  # went on through the rounds


def _host_bench_batch(B):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    from host_workload import host_batch
    return host_batch(B)


def test_oracle_newton_wide_corridor_batch_needs_the_equality_penalty_growth(oracle):
    """The synthetic batch of `host_test bench` (wide corridors, 0.2 m initial offset): once the inequality penalty sits at its cap the primal residual left on the
    dynamics rows falls by < 1 % per multiplier update; with refine_newton_rho_eq_max (default 1e6) the equality penalty grows instead, and on a long stall (the degenerate
    optima of this batch) refine_newton_escalate raises both caps: every path certifies within 80 iterations (whole batch of 4096, oracle: max 80; before: 548 and two uncertified)."""
    b = _host_bench_batch(128)
    p = _set(oracle.device_equivalent_params(), **NEWTON)
    _, info, _ = oracle.solve_batch(b, p)
    assert (info["status"] == 1).all() and (info["status_refine"] == 1).all() and info["iters"].max() < 120, (info["iters"].max(), (info["status_refine"] != 1).sum())
    q = _set(oracle.device_equivalent_params(), **NEWTON)
    q.refine_newton_rho_eq_max = 0.0  # (never grows: the behaviour before the two rules)
    q.refine_newton_escalate = 0
    _, i0, _ = oracle.solve_batch(b, q)
    assert (i0["status_refine"] != 1).sum() >= 1 and i0["iters"].max() > 400  # paths 2, 109: ~450 - 550 iterations, uncertified


@pytest.mark.gpu
def test_device_newton_wide_corridor_batch_matches_oracle(oracle):
    from path_optimizer_amd import binding

    b = _host_bench_batch(128)
    p = _set(binding.default_params(), **NEWTON)
    st, info, xs = binding.Engine(0, p).solve_batch(b, want_x=True)
    ost, oinfo, oxs = oracle.solve_batch(b, oracle.device_equivalent_params(p))
    assert (info["status"] == 1).all() and (info["status_refine"] == 1).all() and (oinfo["status_refine"] == 1).all()
    assert abs(info["iters"].mean() - oinfo["iters"].mean()) <= 0.05 * oinfo["iters"].mean() and info["iters"].max() < 250
    dx = np.abs(xs - oxs).max(axis=1)
    assert dx.max() < 1e-4 and np.median(dx) < 1e-7, (dx.max(), np.median(dx))


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,kw", [("c3", 256, {}), ("c2", 128, {}), ("c5", 32, {}), ("k", 64, {}), ("keep3", 64, {}),
                                       ("c3", 64, dict(refine_rounds=3)), ("c3", 64, dict(refine_chain=3)), ("c3", 64, dict(refine_chain=3, refine_newton_max=5)),
                                       ("c5", 32, dict(refine_chain=3)), ("k", 64, dict(refine_chain=3)), ("c3", 64, dict(refine_newton_max=5))])
def test_device_newton_matches_oracle_and_optimum(oracle, name, B, kw):
    """Both schedulings of the algorithm (fallback launch on demand = the headline, always issued = asynchronous) and starved step budgets (the fallback rounds) against the oracle.
    Newton step counts: the two implementations take the same steps until a decision falls inside the rounding noise of one of them — a row that sits on its
    bound to the last bits is in or out of the Newton matrix, the line search stops at |psi'| <= 0.3 |psi'(0)| one evaluation earlier or later, and the dual
    residual of a certified point (~1e-10, below what either implementation resolves: the device's block-tridiagonal solve leaves 1e-10 .. 1e-12, the oracle's
    sparse LDL' 1e-13) is or is not already 1e3 x below its tolerance, which decides whether a correction step follows.  Every such fork converges to the same
    certified point.  Measured on the whole batches (tools/newton_dev.py, final defaults): |difference in iterations| <= 1 on 99.3 % of config 3, 97.9 % of config 2, 96.7 % of K,
    99.9 % of keep 3, 81.7 % of config 5 (KPC: two more slack families on their bounds); <= 2 on 96 - 100 %; <= 3 on >= 99.6 %; equal counts on 86 % / 76 % / 81 % / 99 % / 45 %; equal means to 1 %."""
    from path_optimizer_amd import binding

    b = batch_of(name, B)
    p = _set(binding.default_params(), **NEWTON)
    _set(p, **kw)
    st, info, xs = binding.Engine(0, p).solve_batch(b, want_x=True)
    ost, oinfo, oxs = oracle.solve_batch(b, oracle.device_equivalent_params(p))
    assert np.array_equal(info["status"], oinfo["status"]) and (info["status"] == 1).all()
    assert (info["status_refine"] == oinfo["status_refine"]).mean() >= 0.98
    if "refine_newton_max" not in kw:
        assert (info["status_refine"] == 1).all() and (oinfo["status_refine"] == 1).all()
    di = np.abs(info["iters"].astype(int) - oinfo["iters"].astype(int))
    if "refine_newton_max" not in kw:
        # (KPC: measured on the round-6 tree 0.78 within one step, 0.97 within two, all within three, on 32 and on 96 paths — the forks are decisions inside rounding noise)
        assert (di <= 1).mean() >= (0.72 if name == "c5" else 0.88) and (di <= 2).mean() >= (0.93 if name == "c5" else 0.95), ((di <= 1).mean(), (di <= 2).mean(), info["iters"][di > 1], oinfo["iters"][di > 1])
    assert (di <= 3).mean() >= 0.9 and abs(info["iters"].mean() - oinfo["iters"].mean()) <= 0.05 * oinfo["iters"].mean()
    dx = np.abs(xs - oxs).max(axis=1)
    assert dx.max() < 1e-4 and np.median(dx) < 1e-8, (dx.max(), np.median(dx))
    assert np.abs(st - ost)[..., :3].max() < 1e-4
    r = _rms(b, xs, _gold(name, B))
    if "refine_newton_max" not in kw:
        assert r.max() < 5e-5, r.max()


@pytest.mark.gpu
def test_device_newton_ragged_and_mixed_batches(oracle):
    """Ragged batch (own point count per path), a batch in which some paths have non-uniform row classes (general launch) — same results as the oracle."""
    from path_optimizer_amd import binding, synth

    b = synth.make_batch(3, B=24)
    b.n_points = np.array([200 - 7 * (i % 9) for i in range(24)], dtype=np.int32)
    b.bounds[3, 50:60, 0, 1] = 1e30   # an infinite clearance on some stages only: non-uniform classes -> the general variant
    b.bounds[7, 20:25, 2, 0] = -1e30
    p = _set(binding.default_params(), **NEWTON)
    st, info, xs = binding.Engine(0, p).solve_batch(b, want_x=True)
    ost, oinfo, oxs = oracle.solve_batch(b, oracle.device_equivalent_params(p))
    assert np.array_equal(info["status"], oinfo["status"]) and np.array_equal(info["status_refine"], oinfo["status_refine"])
    assert (np.abs(info["iters"].astype(int) - oinfo["iters"].astype(int)) <= 6).all()
    assert np.abs(xs - oxs).max() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("keep,N,ds", [(1, 60, 1.0), (2, 128, 0.5), (3, 101, 0.3), (3, 190, 0.3), (4, 90, 0.25), (5, 100, 0.22), (6, 100, 0.19), (7, 100, 0.165), (8, 120, 0.149), (8, 200, 0.149),
                                         (9, 150, 0.133), (10, 150, 0.1199), (11, 120, 0.109), (12, 200, 0.0999), (13, 100, 0.0922), (14, 150, 0.0856), (15, 121, 0.0799), (16, 200, 0.0749)])
def test_device_newton_every_keep_value_matches_oracle(oracle, keep, N, ds):
    """Every chunk shape of the one-wave / two-wave mappings (keep_control_steps_ 1 .. 8: what the reference's pipeline produces; 9 .. 16: the wide role-split shapes) through the Newton refinement —
    a factorisation per step under penalties of 1e3 .. 1e5 — uniform and pinned-row (general kernel) batches; every path certified, the same point as the oracle."""
    import np_twin as T
    from path_optimizer_amd import binding, synth

    rng = np.random.default_rng(100 + keep)
    insts = [T.random_instance(rng, N, ds=ds) for _ in range(8)]
    stk = lambda k: np.ascontiguousarray(np.stack([i[k] for i in insts]))
    b = synth.Batch(0, 8, N, keep, stk("ref_x"), stk("ref_y"), stk("ref_z"), stk("ref_k"), stk("ref_s"), stk("bounds"), stk("x0"), np.array([i["goal_z"] for i in insts]))
    assert binding.keep_control_steps(0, b.ref_s[0]) == keep
    for pin in (False, True):
        if pin:
            b.bounds[:, N // 3, 1, :] = 0.25  # one covering circle pinned: an equality row -> non-uniform classes -> the general kernel
        p = _set(binding.default_params(), **NEWTON)
        st, info, xs = binding.Engine(0, p).solve_batch(b, want_x=True)
        ost, oinfo, oxs = oracle.solve_batch(b, oracle.device_equivalent_params(p))
        assert np.array_equal(info["status"], oinfo["status"]) and np.array_equal(info["status_refine"], oinfo["status_refine"])
        ok = info["status"] == 1
        assert (info["status_refine"][ok] == 1).all()
        assert (np.abs(info["iters"].astype(int) - oinfo["iters"].astype(int))[ok] <= 4).all(), (keep, N, pin, info["iters"], oinfo["iters"])
        assert np.abs(xs - oxs)[ok].max() < 1e-5, (keep, N, pin, np.abs(xs - oxs)[ok].max())


@pytest.mark.gpu
def test_device_newton_edge_cases_of_the_batch_interface(oracle):
    """The headline setting through the cases the plain solve is tested on: empty batch, B = 1, N = 2 / 3 / 10, an infeasible corridor and non-finite inputs inside a
    batch (never reported certified, the neighbours are unaffected), the caller's order hint (bit-identical), repeated solves (deterministic),
    every scheduling giving the same statuses and certificates."""
    import np_twin as T
    from path_optimizer_amd import binding, synth

    p = _set(binding.default_params(), **NEWTON)
    eng = binding.Engine(0, p)
    b0 = synth.make_batch(3, B=2); b0.B = 0
    assert eng.solve_batch(b0)[0].shape[0] == 0
    # B = 1 and tiny N, every formulation
    for form in (T.PO_KP, T.PO_KPC, T.PO_K):
        for N in (2, 3, 10):
            rng = np.random.default_rng(7 + N)
            i = T.random_instance(rng, N, ds=0.3)
            one = lambda k: np.ascontiguousarray(i[k][None])
            keep = 1 if form == T.PO_K else 4
            b = synth.Batch(form, 1, N, keep, one("ref_x"), one("ref_y"), one("ref_z"), one("ref_k"), one("ref_s"), one("bounds"), one("x0"), np.array([i["goal_z"]]),
                            one("max_k") if form == T.PO_KPC else None, one("max_kp") if form == T.PO_KPC else None)
            st, info, xs = eng.solve_batch(b, want_x=True)
            ost, oinfo, oxs = oracle.solve_batch(b, oracle.device_equivalent_params(p))
            assert np.array_equal(info["status"], oinfo["status"]) and np.array_equal(info["status_refine"], oinfo["status_refine"]), (form, N, info, oinfo)
            assert np.abs(xs - oxs).max() < 1e-6, (form, N, np.abs(xs - oxs).max())
    # an infeasible corridor and non-finite inputs inside a batch
    b = synth.make_batch(3, B=8)
    clean = eng.solve_batch(b, want_x=True)
    assert (clean[1]["status"] == 1).all() and (clean[1]["status_refine"] == 1).all()
    b.bounds[1, 10, :, :] = [0.9, 1.0]
    b.bounds[1, 11, :, :] = [-1.0, -0.9]
    b.ref_k[3, 50] = np.nan
    b.x0[6, 0] = np.inf
    st, info, xs = eng.solve_batch(b, want_x=True)
    ost, oinfo, oxs = oracle.solve_batch(b, oracle.device_equivalent_params(p))
    good = np.array([0, 2, 4, 5, 7])
    # (the infeasible path passes OSQP's test at 1e4 x eps, fails its Newton attempt and is found infeasible by the type-based iteration of a later round: -1, like the oracle)
    assert info["status"][1] == oinfo["status"][1] and info["status"][1] != 1 and info["status_refine"][1] == oinfo["status_refine"][1] and info["status_refine"][1] != 1
    assert (info["status"][[3, 6]] == -8).all() and (info["status_refine"][[3, 6]] == 0).all() and not np.isnan(st[3]).any()  # (a NaN input: outputs zeroed before any work; an Inf start state is caught in the iterate)
    assert (info["status"][good] == 1).all() and (info["status_refine"][good] == 1).all()
    assert np.array_equal(xs[good], clean[2][good]) and np.array_equal(info["iters"][good], clean[1]["iters"][good])
    # order hint: bit-identical; repeated solve: bit-identical; schedulings: same statuses / certificates, same points to rounding
    b = synth.make_batch(3, B=48)
    st0, info0, x0 = eng.solve_batch(b, want_x=True)
    order = np.argsort(-info0["iters"].astype(np.int64), kind="stable")
    st1, info1, x1 = eng.solve_batch(b, want_x=True, order=order)
    assert np.array_equal(x0, x1) and np.array_equal(info0["iters"], info1["iters"]) and np.array_equal(info0["n_refactor"], info1["n_refactor"])
    st2, info2, x2 = eng.solve_batch(b, want_x=True)
    assert np.array_equal(x0, x2) and np.array_equal(st0, st2)
    for chain in (3,):
        q = _set(binding.default_params(), **NEWTON); q.refine_chain = chain
        e2 = binding.Engine(0, q)
        st3, info3, x3 = e2.solve_batch(b, want_x=True)
        assert np.array_equal(info3["status"], info0["status"]) and np.array_equal(info3["status_refine"], info0["status_refine"])
        assert np.abs(x3 - x0).max() < 1e-5 and (np.abs(info3["iters"].astype(int) - info0["iters"].astype(int)) <= 3).all()


# ---- the rounds around the Newton phase (po_params.refine_rounds / refine_extra_rounds): what a starved phase hands back, and the rounds below eps ----
def _exhausted_case():
    """Config-3 paths 2400 .. 2415 with a Newton budget of 2 steps per attempt (nothing certifies in 2 steps): path 2410 meets eps in the last regular round (575 type-based
    iterations), its attempt fails, and the first round below eps (eps / 10) runs out of max_iter."""
    from path_optimizer_amd import synth

    return synth.make_batch(3, B=16, first_path=2400), dict(refine=2, refine_rounds=3, refine_extra_rounds=2, refine_newton_max=2)


def test_oracle_round_below_eps_never_unsolves_a_path(oracle):
    """A path that met the caller's eps in the last regular round is SOLVED whatever the rounds below eps do.  max_iter 700: the round below eps runs out of iterations on a
    point that still passes OSQP's test at eps -> that point, solved, status_refine -1, no further attempt.  max_iter 800 / 925: it runs out on a point that FAILS eps (ADMM
    residuals are not monotone) -> the point that round STARTED from, exactly what the path returns without rounds below eps."""
    b, kw = _exhausted_case()
    i = 10  # path 2410

    def run(**more):
        p = _set(oracle.device_equivalent_params(), **dict(kw, **more))
        return oracle.solve_batch(b, p, want_x=True)

    _, info, _ = run(max_iter=700)
    assert info["status"][i] == 1 and info["status_refine"][i] == -1 and info["iters"][i] > 700
    assert info["r_prim"][i] < 1e-3 and info["r_dual"][i] < 1e-1  # OSQP's relative test at eps held (norms of order 1 .. 1e3)
    for mi in (800, 925):
        _, info, xs = run(max_iter=mi)
        _, i0, x0 = run(max_iter=mi, refine_extra_rounds=0)
        assert (info["status"] == 1).all() and info["status_refine"][i] == -1 and i0["status_refine"][i] == -1 and i0["status"][i] == 1
        assert np.array_equal(xs[i], x0[i]) and info["r_prim"][i] == i0["r_prim"][i] and info["r_dual"][i] == i0["r_dual"][i]
        assert info["iters"][i] > i0["iters"][i]  # (the iterations of the failed round are counted)


@pytest.mark.gpu
def test_device_round_below_eps_matches_the_oracle(oracle):
    from path_optimizer_amd import binding

    b, kw = _exhausted_case()
    for chain, mi in ((2, 800), (3, 800), (2, 925), (2, 700)):
        p = _set(binding.default_params(), **dict(kw, refine_chain=chain, max_iter=mi))
        st, info, xs = binding.Engine(0, p).solve_batch(b, want_x=True)
        ost, oinfo, oxs = oracle.solve_batch(b, oracle.device_equivalent_params(p), want_x=True)
        assert np.array_equal(info["status"], oinfo["status"]) and info["status"][10] == 1, (chain, mi, info["status"], oinfo["status"])
        assert np.array_equal(info["status_refine"], oinfo["status_refine"]) and info["status_refine"][10] == -1
        same = info["iters"] == oinfo["iters"]
        assert same[10] and same.mean() >= 0.8 and np.abs(xs[same] - oxs[same]).max() < 1e-6
        assert abs(info["r_prim"][10] - oinfo["r_prim"][10]) < 1e-9 and abs(info["r_dual"][10] - oinfo["r_dual"][10]) < 1e-7


@pytest.mark.gpu
def test_device_status_refine_says_what_was_certified(oracle):
    """po_info.status_refine: 0 without the refinement, 1 exactly on the paths whose returned point satisfies OSQP's test at refine_eps (as the phase evaluated it ON THAT
    POINT), -1 on the others; same flags as the oracle; non-finite paths never carry a 1."""
    from path_optimizer_amd import binding, synth

    b = synth.make_batch(3, B=128)
    st, info, xs = binding.Engine(0).solve_batch(b, want_x=True)
    assert (info["status_refine"] == 0).all() and (info["reserved"] == 0).all()
    for kw in (dict(NEWTON), dict(NEWTON, refine_rounds=1, refine_extra_rounds=0), dict(NEWTON, refine_newton_max=6, refine_extra_rounds=0, refine_rounds=2)):
        p = _set(binding.default_params(), **kw)
        st, info, xs = binding.Engine(0, p).solve_batch(b, want_x=True)
        ost, oinfo, oxs = oracle.solve_batch(b, oracle.device_equivalent_params(p))
        assert set(np.unique(info["status_refine"])) <= {1, -1} and (info["status"] == 1).all()
        cert = info["status_refine"] == 1
        # certified <=> the residuals of the returned point satisfy the relative criteria at refine_eps (1e-8): in particular both are below 1e-8 (1 + norm) ~ 1e-6 ...
        assert (info["r_prim"][cert] < 1e-6).all() and (info["r_dual"][cert] < 1e-5).all()
        assert (info["status_refine"] == oinfo["status_refine"]).mean() >= 0.97
        if "refine_newton_max" in kw:
            assert (info["status_refine"] == -1).any()  # a 6-step budget leaves paths uncertified: that is what the flag is for
    with pytest.raises(binding.PoError):
        binding.Engine(0, _set(binding.default_params(), refine=1))  # removed with ABI 5
    bad = synth.make_batch(3, B=4)
    bad.bounds[1, 50, 2, 0] = np.nan
    st, info, xs = binding.Engine(0, _set(binding.default_params(), **NEWTON)).solve_batch(bad, want_x=True)
    assert info["status"][1] == -8
    assert info["status_refine"][1] == 0 and (st[1] == 0).all() and (xs[1] == 0).all()  # defined outputs (zeros), never the buffer's previous content
    assert (info["status"][[0, 2, 3]] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slice_", [0, 3, 8])
def test_failed_attempts_on_ragged_lengths_hand_back_finite_states(oracle, slice_):
    """Round 6: the single (unsliced) Newton launch handed the fall-back rounds a state block with Inf / NaN on the LAST lane of every path whose length is not a multiple of
    four whenever the attempt was not certified: a wave-uniform scalar kept one copy per lane (rho of the warm start, read at kernel entry, used by the phase's last pass) came
    back 0 on that lane, the re-expression of v divided by it, and the type-based iteration that followed went non-finite (status -8 where the oracle detects the infeasible
    corridor, -3) — on 9 of the 14 infeasible paths of this batch, the other 5 being the ones with 4 | n_points.  Which builds showed it depended on the register allocation
    (DESIGN.md section 12); the scalars the phase carries now live in scalar registers (uni(), csrc/po_device.hpp).  Device = oracle on every status, no path non-finite."""
    from path_optimizer_amd import binding, synth

    b = synth.make_batch(3, B=333)
    b.n_points = np.random.default_rng(5).integers(60, 201, size=333).astype(np.int32)
    p = _set(binding.default_params(), **NEWTON)
    e = binding.Engine(0, p)
    e.debug_set("newton_slice", slice_)
    st, info, xs = e.solve_batch(b, want_x=True)
    ost, oinfo, oxs = oracle.solve_batch(b, oracle.device_equivalent_params(p))
    bad = np.flatnonzero(oinfo["status"] != 1)
    assert len(bad) == 14 and (b.n_points[bad] % 4 != 0).sum() == 9  # the batch the bug was found on
    assert np.array_equal(info["status"], oinfo["status"]), (info["status"][bad].tolist(), oinfo["status"][bad].tolist())
    assert (info["status"] != -8).all() and np.isfinite(st).all() and np.isfinite(xs).all()
    # (an infeasible path: several Newton attempts and rounds of type-based iterations before the certificate fires; device and oracle fork on rounding in the attempts)
    assert (np.abs(info["iters"][bad] - oinfo["iters"][bad]) <= 0.35 * oinfo["iters"][bad] + 50).all(), (info["iters"][bad].tolist(), oinfo["iters"][bad].tolist())  # measured: 1 .. 55, one path 271 of 950


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["c3", "c3_ragged", "keep2", "keep6", "keep7", "keep12", "keep15", "c5", "k", "tiny",
                                  # (round 6, second session: every other mapping too, and ragged KPC / K batches — the long loops of the UNSLICED launch are the library's
                                  #  least-exercised code)
                                  "keep1", "keep3", "keep5", "keep8", "keep9", "keep10", "keep16", "c5_ragged", "k_ragged"])
def test_sliced_newton_launches_change_nothing_but_the_schedule(case):
    """The engine issues the Newton refinement as TWO launches (every path for 8 steps; the unfinished ones parked, sorted by expected remaining work, resumed longest
    first — po_debug_set "newton_slice").  Parking and resuming keep every number the phase carries: statuses and certificates are those of the single launch, the solutions
    agree to round-off."""
    from path_optimizer_amd import binding, synth
    import np_twin as T

    def rand(keep, N, B, seed):
        rng = np.random.default_rng(seed)
        insts = [T.random_instance(rng, N, ds=1.2 / keep * 0.999) for _ in range(B)]
        st = lambda k: np.ascontiguousarray(np.stack([i[k] for i in insts]))
        return synth.Batch(0, B, N, keep, st("ref_x"), st("ref_y"), st("ref_z"), st("ref_k"), st("ref_s"), st("bounds"), st("x0"), np.array([i["goal_z"] for i in insts]))

    if case == "c3":
        b = synth.make_batch(3, B=700)
    elif case == "c3_ragged":
        b = synth.make_batch(3, B=333)
        b.n_points = np.random.default_rng(5).integers(60, 201, size=333).astype(np.int32)
    elif case == "c5":
        b = synth.make_batch(5, B=96)
    elif case == "c5_ragged":
        b = synth.make_batch(5, B=80)
        b.n_points = np.random.default_rng(6).integers(150, 401, size=80).astype(np.int32)
    elif case == "k":
        b = synth.make_batch(3, B=130, formulation=2)
    elif case == "k_ragged":
        b = synth.make_batch(3, B=150, formulation=2)
        b.n_points = np.random.default_rng(7).integers(60, 201, size=150).astype(np.int32)
    elif case == "tiny":
        b = synth.make_batch(3, B=1)
    else:
        b = rand(int(case[4:]), 150, 64, 7)
    out = {}
    for sl in (0, 8, 3):
        p = binding.default_params()
        for k, v in NEWTON.items():
            setattr(p, k, v)
        e = binding.Engine(0, p)
        e.debug_set("newton_slice", sl)
        st, info, xs = e.solve_batch(b, want_x=True)
        out[sl] = (st.copy(), info.copy(), xs.copy(), e.debug_get("newton_parked"), e.debug_get("newton_list_ok"))
    assert out[0][3] == -1 and out[8][3] >= 0 and out[3][3] >= out[8][3]
    assert out[0][4] == -1 and out[8][4] == 1 and out[3][4] == 1  # the second launch's list: every parked path once, keys non-increasing, ties in path order (nw_sort_kernel)
    if case in ("c3", "c5", "k"):
        assert out[8][3] > 0.5 * b.B  # nearly every path needs more than 8 steps
    for sl in (8, 3):
        # the same operations in the same order; the kernels of the two launches are compiled separately and may contract multiply-adds differently, so the iterates
        # agree to round-off, not bit for bit (measured: identical on the KP keep 3 / 4 and K shapes, <= 7e-11 elsewhere)
        cert = (out[0][1]["status"] == 1) & (out[0][1]["status_refine"] == 1)  # (an uncertified path went through the rounds: hundreds of type-based iterations amplify the round-off)
        assert np.abs(out[sl][0] - out[0][0])[cert].max() < 1e-8 and np.abs(out[sl][2] - out[0][2])[cert].max() < 1e-8
        assert np.abs(out[sl][0] - out[0][0]).max() < 1e-6 and np.abs(out[sl][2] - out[0][2]).max() < 1e-6
        for f in ("status", "status_refine", "status_polish"):
            assert np.array_equal(out[sl][1][f], out[0][1][f]), f
        assert np.abs(out[sl][1]["iters"] - out[0][1]["iters"]).max() <= 3 and (out[sl][1]["iters"] != out[0][1]["iters"]).mean() <= 0.05
    if not case.endswith("_ragged"):  # (paths cut short at a random point: some are infeasible (14 of 333 of config 3) and go through the fallback rounds — the parked / resumed state feeds those as well)
        assert (out[0][1]["status_refine"] == 1).all()


def _fuzz_case_at_headline(make_params, seed):
    """The random case `seed` of tests/test_gpu_fuzz.py at the headline setting (same draws as test_random_case_newton_matches_oracle)."""
    import np_twin as T
    import test_gpu_fuzz as F
    from path_optimizer_amd import binding

    rng, form, b = F._case(seed)
    if form == T.PO_KP:
        b.keep = binding.keep_control_steps(form, b.ref_s[0])
    p = F._params(rng, make_params)
    if seed % 3 == 0:
        b.bounds = b.bounds * float(rng.choice([0.5, 0.7]))
    chain = int(rng.choice([2, 3]))
    for k, v in NEWTON.items():
        setattr(p, k, v)
    p.refine_chain = chain
    return b, p


def test_oracle_a_stagnating_attempt_gives_up_after_a_few_steps(oracle):
    """Cases 250 (KPC) and 214 (KP, keep 1) of the wider fuzz sweep (tools/fuzz_more.py): one path's dual residual sits on a floor above refine_eps (slack weights of 1e5 put the
    rounding of rho_eq (a.x - b) there; a flat valley damped by the proximal terms) while every step is a full step on an unchanged factorisation.  Such an attempt used to burn its
    300 steps in each of six rounds (2 275 / 5 800 iterations, ~80 ms of a device batch); now it ends after 8 stagnant steps: the path stays SOLVED and flagged -1, the others certified."""
    b, p = _fuzz_case_at_headline(oracle.default_params, 250)
    _, info, _ = oracle.solve_batch(b, oracle.device_equivalent_params(p), want_x=True)
    assert (info["status"] == 1).all() and list(info["status_refine"]) == [1, 1, -1, 1, 1]
    assert info["iters"][2] < 700 and info["iters"][[0, 1, 3, 4]].max() < 80
    b, p = _fuzz_case_at_headline(oracle.default_params, 214)
    _, info, _ = oracle.solve_batch(b, oracle.device_equivalent_params(p), want_x=True)
    assert (info["status"] == 1).all() and list(info["status_refine"]) == [-1, -1, 1, -1, 1]
    assert info["iters"][1] < 400 and info["iters"][3] < 400  # (2 275 each before; path 0's 4 096 are type-based iterations of the rounds)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [250, 214])
def test_device_stagnating_attempt_matches_the_oracle(oracle, seed):
    from path_optimizer_amd import binding

    b, p = _fuzz_case_at_headline(binding.default_params, seed)
    bo, po = _fuzz_case_at_headline(oracle.default_params, seed)
    st, info, xs = binding.Engine(0, p).solve_batch(b, want_x=True)
    _, oinfo, oxs = oracle.solve_batch(bo, oracle.device_equivalent_params(po), want_x=True)
    assert np.array_equal(info["status"], oinfo["status"]) and np.array_equal(info["status_refine"], oinfo["status_refine"])
    cert = info["status_refine"] == 1
    assert (np.abs(info["iters"].astype(int) - oinfo["iters"])[cert] <= 3).all(), (info["iters"], oinfo["iters"])
    # a path on a rounding floor: which round's attempt stagnates when is decided by noise — the outcome (SOLVED, flagged -1) is the same, the iteration count of the same order,
    # and far below what the unguarded attempts burned (2 275 / 5 800)
    assert (info["iters"][~cert] <= 2 * oinfo["iters"][~cert] + 100).all() and info["iters"].max() < 4500, (info["iters"], oinfo["iters"])
    assert np.abs(xs - oxs)[cert].max() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [250, 214])
def test_sliced_launches_count_stagnation_like_the_single_launch(seed):
    """a path parked in a `quiet` state used to have the stagnation counter advanced a second time when the second launch re-evaluated the residual of the park
    point (kNwStagnation - 1 non-halving steps instead of kNwStagnation before the attempt gives up).  The stagnating fuzz cases, sliced (8 and 3 steps: the park lands inside the
    stagnant stretch) against the single launch: the same iteration counts on the paths whose attempt ends on stagnation, the same statuses and flags."""
    from path_optimizer_amd import binding

    b, p = _fuzz_case_at_headline(binding.default_params, seed)
    out = {}
    for sl in (0, 8, 3):
        e = binding.Engine(0, p)
        e.debug_set("newton_slice", sl)
        st, info, xs = e.solve_batch(b, want_x=True)
        out[sl] = (info.copy(), xs.copy())
    flagged = out[0][0]["status_refine"] == -1
    assert flagged.any()
    for sl in (8, 3):
        assert np.array_equal(out[sl][0]["status"], out[0][0]["status"]) and np.array_equal(out[sl][0]["status_refine"], out[0][0]["status_refine"])
        # certified paths: the usual round-off forks (<= 3); the stagnating ones go through the rounds, where one step more or less in an attempt shifts everything after it —
        # what the double count produced was an attempt ending a step early in EVERY round
        cert = ~flagged
        assert (np.abs(out[sl][0]["iters"].astype(int) - out[0][0]["iters"])[cert] <= 3).all()
        assert np.abs(out[sl][1] - out[0][1])[cert].max() < 1e-7


@pytest.mark.gpu
def test_refinement_and_polish_on_a_shape_without_their_kernel_say_so():
    """VERDICT r5 missing 3 / ADVICE r5: refine = 2 (and polish) on a shape of the single-level mapping used to run the plain solve and return status_refine = 0 — the value that
    also means "off".  Now every path of such a batch carries PO_NOT_AVAILABLE (-2): KP keep 17 (any N), KP keep 4 at N = 600 (beyond the two-level limit of 512), keep 12 beyond
    N = 32 keep; the polish also on the role-split shapes (keep 6 .. 8).  The solve itself is the plain solve at eps: statuses and points equal those of refine = 0."""
    import np_twin as T
    from path_optimizer_amd import abi, binding, synth

    def rand(keep, N, B, seed):
        rng = np.random.default_rng(seed)
        insts = [T.random_instance(rng, N, ds=1.2 / keep * 0.999) for _ in range(B)]
        st = lambda k: np.ascontiguousarray(np.stack([i[k] for i in insts]))
        return synth.Batch(0, B, N, keep, st("ref_x"), st("ref_y"), st("ref_z"), st("ref_k"), st("ref_s"), st("bounds"), st("x0"), np.array([i["goal_z"] for i in insts]))

    for keep, N in ((17, 120), (4, 600), (12, 32 * 12 + 8)):
        b = rand(keep, N, 5, 40 + keep)
        assert binding.keep_control_steps(0, b.ref_s[0]) == keep
        st0, info0, xs0 = binding.Engine(0).solve_batch(b, want_x=True)
        assert (info0["status_refine"] == 0).all() and (info0["status_polish"] == 0).all()  # off: 0
        p = _set(binding.default_params(), **NEWTON)
        p.polish = 1
        st, info, xs = binding.Engine(0, p).solve_batch(b, want_x=True)
        assert (info["status_refine"] == abi.PO_NOT_AVAILABLE).all(), (keep, N, info["status_refine"])
        assert (info["status_polish"] == abi.PO_NOT_AVAILABLE).all(), (keep, N, info["status_polish"])
        # (headline setting: the warm start stops at 1e4 x eps, so the plain solve it ran is the one at THAT eps_mul? no: without the Newton kernel the call runs the caller's eps)
        assert np.array_equal(info["status"], info0["status"]) and np.array_equal(info["iters"], info0["iters"]) and np.array_equal(xs, xs0)
    # role-split shapes: the Newton refinement runs (certified), the polish has no kernel
    for keep in (6, 7, 8):
        b = rand(keep, 100, 5, 60 + keep)
        p = _set(binding.default_params(), **NEWTON)
        p.polish = 1
        st, info, xs = binding.Engine(0, p).solve_batch(b, want_x=True)
        assert (info["status_refine"] == 1).all() and (info["status_polish"] == abi.PO_NOT_AVAILABLE).all(), (keep, info)
    # and a shape that has both: neither field is -2
    b = rand(4, 100, 5, 64)
    p = _set(binding.default_params(), **NEWTON)
    p.polish = 1
    st, info, xs = binding.Engine(0, p).solve_batch(b, want_x=True)
    assert (info["status_refine"] == 1).all() and np.isin(info["status_polish"], (1, -1)).all()
