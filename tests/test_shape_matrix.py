"""Every kernel shape at its boundary lengths against the oracle (GPU).  One row of tests/shape_table.py MATRIX per reachable (formulation, shape): each two-level shape is
its own instance of the solve, Newton, fallback and polish kernels, with its own register allocation, and the two- and four-wave blocks are the only place where the
cross-wave combines run.  Per row and boundary length a small ragged batch: a path at N, one at N - 1, one that ends inside the block's first wave (the later waves own no
stage), one at the shape's smallest length, one whose length is a multiple of neither 4 nor keep, and on the full runs one more with an infeasible corridor jump.
Bars are those of the suite's existing tests for the same setting (test_gpu_parity.py, test_newton.py, test_polish.py).  Default set: the fixed-iteration iterates, the
OSQP-faithful run, the headline setting, the refusal limits; `slow`: the sliced Newton launches, the fallback kernel, the polish, the shapes without those kernels."""
import numpy as np
import pytest

import np_twin as T
import shape_table as S
from test_newton import NEWTON

pytestmark = pytest.mark.gpu

TWO = [r for r in S.MATRIX if r[2][0]]
POLISH = [r for r in S.MATRIX if S.has_polish_kernel(r[2])]
NO_KERNEL = [r for r in S.MATRIX if not S.has_polish_kernel(r[2])]  # single-level (no Newton, no polish kernel) and role-split (no polish kernel)
ids = S.row_id


def _ds(form, keep):
    return 1.2 / keep * 0.999 if form == S.KP else 1.2 / 4 * 0.999  # (KPC: keep 4; K: the spacing of the KPC rows)


def _lengths(row, N):
    """n_points of the ragged batch at batch length N: N, N - 1, inside the first wave, the shape's smallest, a multiple of neither 4 nor keep."""
    form, keep, shape, lengths = row
    lo, least = lengths[0], (keep + 2 if form == S.KP else 3)
    inside = S.first_wave_stages(shape, keep) - 3 if shape[1] > 64 else N // 2
    odd = (lo + N) // 2
    while odd > least and (odd % 4 == 0 or (keep > 1 and odd % keep == 0)):
        odd -= 1
    return [min(N, max(least, n)) for n in (N, N - 1, inside, lo, odd)]


def _batch(row, N, full):
    """The row's batch at length N (seeded by row and length); full: one more path with a corridor that jumps sideways within one step (primal infeasible)."""
    from path_optimizer_amd import binding, synth

    form, keep, shape, _ = row
    rng = np.random.default_rng(100000 * form + 1000 * keep + N)
    npts = _lengths(row, N) + ([N] if full else [])
    insts = [T.random_instance(rng, N, ds=_ds(form, keep), narrow=True) for _ in npts]
    stk = lambda k: np.ascontiguousarray(np.stack([i[k] for i in insts]))
    b = synth.Batch(form, len(npts), N, keep, stk("ref_x"), stk("ref_y"), stk("ref_z"), stk("ref_k"), stk("ref_s"), stk("bounds"), stk("x0"),
                    np.array([i["goal_z"] for i in insts]), stk("max_k") if form == S.KPC else None, stk("max_kp") if form == S.KPC else None,
                    np.array(npts, dtype=np.int32))
    b.goal_z = b.goal_z - b.ref_z[:, -1] + b.ref_z[np.arange(b.B), b.n_points - 1]  # (the end-heading window of a shortened path: its own last heading, not that of stage N - 1)
    if form == S.KP:
        assert binding.keep_control_steps(form, b.ref_s[0]) == keep
    bad = len(npts) - 1
    if full and N > 20:
        j = N // 2
        b.bounds[bad, j, :, :] = [0.9, 1.0]
        b.bounds[bad, j + 1, :, :] = [-1.0, -0.9]
    return b, (bad if full and N > 20 else None)


def _params(**kw):
    from path_optimizer_amd import binding

    p = binding.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _run(b, p, slice_=None, get=()):
    from path_optimizer_amd import binding

    e = binding.Engine(0, p)
    if slice_ is not None:
        e.debug_set("newton_slice", slice_)
    st, info, xs = e.solve_batch(b, want_x=True)
    extra = [e.debug_get(k) for k in get]
    e.close()
    return st.copy(), info.copy(), xs.copy(), extra


def _oracle(oracle, b, p):
    return oracle.solve_batch(b, oracle.device_equivalent_params(p))


def _kkt(oracle, b, i, x, p):
    pa = oracle.default_params()
    for f in ("w_curv", "w_curv_rate", "w_slack", "w_dev", "k_w_curv", "k_w_curv_rate", "k_w_dev", "w_k_slack", "w_kp_slack", "margin", "max_steer", "wheel_base", "constraint_end_heading"):
        setattr(pa, f, getattr(p, f))
    n_i = int(b.n_points[i])
    nv, _, _ = oracle.dims(b.formulation, n_i, b.keep)
    P, A, l, u = oracle.assemble(b.formulation, pa, n_i, b.keep, b.ref_k[i, :n_i], b.ref_s[i, :n_i], b.ref_z[i, n_i - 1], b.bounds[i, :n_i], b.x0[i], b.goal_z[i],
                                 None if b.max_k is None else b.max_k[i, :n_i], None if b.max_kp is None else b.max_kp[i, :n_i])
    return T.kkt_certificate(P, A, l, u, x[:nv])


# ---- a: fixed iterations (test_gpu_parity.py::test_every_keep_control_steps_value) ----
@pytest.mark.parametrize("row", S.MATRIX, ids=ids)
def test_fixed_iterations_match_oracle(oracle, row):
    for N in row[3]:
        b, _ = _batch(row, N, full=False)
        p = _params(max_iter=60, check_every=0, adapt_every=25)
        st, info, xs, _ = _run(b, p)
        ost, oinfo, oxs = _oracle(oracle, b, p)
        assert np.abs(xs - oxs).max() < 1e-8 and np.abs(st - ost).max() < 1e-8, (N, np.abs(xs - oxs).max(axis=1))
        assert np.array_equal(info["n_refactor"], oinfo["n_refactor"]), N


# ---- b: the OSQP-faithful full run (termination, adaptive rho, the infeasibility certificate) ----
def _osqp_faithful(oracle, row, N):
    b, bad = _batch(row, N, full=True)
    p = _params()
    st, info, xs, _ = _run(b, p)
    ost, oinfo, oxs = _oracle(oracle, b, p)
    assert np.array_equal(info["status"], oinfo["status"]), (N, info["status"], oinfo["status"])
    assert np.array_equal(info["iters"], oinfo["iters"]), (N, info["iters"], oinfo["iters"])
    assert np.array_equal(info["n_refactor"], oinfo["n_refactor"]), N
    if bad is not None:
        assert info["status"][bad] != 1
    ok = info["status"] == 1
    assert ok.sum() >= b.B - 1, (N, info["status"])
    assert np.abs(xs - oxs)[ok].max() < 1e-5 and np.abs(st - ost)[ok].max() < 1e-5, (N, np.abs(xs - oxs).max(axis=1))


@pytest.mark.parametrize("row", S.MATRIX, ids=ids)
def test_osqp_faithful_run_matches_oracle(oracle, row):
    for N in row[3]:
        _osqp_faithful(oracle, row, N)


# ---- c: the headline setting (test_newton.py::test_device_newton_every_keep_value_matches_oracle, test_gpu_fuzz.py::_newton_case) ----
@pytest.mark.parametrize("row", TWO, ids=ids)
def test_headline_newton_matches_oracle(oracle, row):
    for N in row[3]:
        b, bad = _batch(row, N, full=True)
        p = _params(**NEWTON)
        st, info, xs, _ = _run(b, p)
        ost, oinfo, oxs = _oracle(oracle, b, p)
        assert np.array_equal(info["status"], oinfo["status"]) and np.array_equal(info["status_refine"], oinfo["status_refine"]), (N, info, oinfo)
        ok = info["status"] == 1
        feas = np.ones(b.B, bool)
        if bad is not None:
            feas[bad] = False
            assert not ok[bad]
        assert ok[feas].all() and (info["status_refine"][feas] == 1).all(), (N, info["status"], info["status_refine"])
        di = np.abs(info["iters"].astype(int) - oinfo["iters"].astype(int))
        assert (di[ok] <= 4).all(), (N, info["iters"], oinfo["iters"])
        assert np.abs(xs - oxs)[ok].max() < 1e-5 and np.abs(st - ost)[ok].max() < 1e-5, (N, np.abs(xs - oxs).max(axis=1))
        if N == next(n for n in row[3] if n >= 20):
            # the device point is optimal for the QP, whatever either solver thinks: one path per row (the shape's smallest length, else the odd one; the certificate's
            # exact fallback takes up to a minute on a KPC path of 250 stages)
            i = 3 if b.n_points[3] >= 20 else 4
            k = _kkt(oracle, b, i, xs[i], p)
            assert k["primal_violation"] < 1e-6 and k["stationarity_rel"] < 1e-5, (N, int(b.n_points[i]), k)


# ---- d: the sliced Newton launches against the single one (test_newton.py::test_sliced_newton_launches_change_nothing_but_the_schedule) ----
@pytest.mark.slow
@pytest.mark.parametrize("row", TWO, ids=ids)
def test_sliced_newton_launches_change_nothing_but_the_schedule(row):
    differ = total = 0
    for N in row[3]:
        b, _ = _batch(row, N, full=True)
        p = _params(**NEWTON)
        out = {sl: _run(b, p, sl, get=("newton_list_ok",)) for sl in (0, 8, 3)}
        cert = (out[0][1]["status"] == 1) & (out[0][1]["status_refine"] == 1)
        assert out[0][3][0] == -1
        for sl in (8, 3):
            assert out[sl][3][0] == 1, (N, sl)
            for f in ("status", "status_refine", "status_polish"):
                assert np.array_equal(out[sl][1][f], out[0][1][f]), (N, sl, f)
            assert np.abs(out[sl][0] - out[0][0])[cert].max() < 1e-8 and np.abs(out[sl][2] - out[0][2])[cert].max() < 1e-8, (N, sl)
            assert np.abs(out[sl][0] - out[0][0]).max() < 1e-6 and np.abs(out[sl][2] - out[0][2]).max() < 1e-6, (N, sl)
            # iteration counts: equal on the certified paths (one in twenty may fork by a step or three); the infeasible path runs hundreds of type-based iterations in the
            # rounds after its failed attempts, where the round-off of the separately compiled launches moves the iteration the certificate fires at (multi-group keep 1:
            # 350 .. 405 iterations, up to 5 apart, the point equal to 1e-14) — the bound of test_newton.py::test_failed_attempts_on_ragged_lengths_hand_back_finite_states
            di = np.abs(out[sl][1]["iters"].astype(int) - out[0][1]["iters"].astype(int))
            assert di[cert].max() <= 3, (N, sl, di)
            assert (di[~cert] <= 0.35 * out[0][1]["iters"][~cert] + 50).all(), (N, sl, di)
            differ, total = differ + int((di[cert] != 0).sum()), total + int(cert.sum())
    assert differ <= 0.05 * total, (differ, total)


# ---- e: the fallback kernel with work on its list (the refine_newton_max legs of test_newton.py::test_device_newton_matches_oracle_and_optimum) ----
@pytest.mark.slow
@pytest.mark.parametrize("row", TWO, ids=ids)
def test_fallback_kernel_takes_every_failed_attempt(oracle, row):
    agree = total = 0
    dx = []
    for N in row[3]:
        b, _ = _batch(row, N, full=True)
        p = _params(**dict(NEWTON, refine_newton_max=2))  # (no attempt certifies in two steps: newton_kernel hands every path to the fallback launch)
        st, info, xs, (fb,) = _run(b, p, get=("fallback_paths",))
        ost, oinfo, oxs = _oracle(oracle, b, p)
        assert fb > 0, N
        assert np.array_equal(info["status"], oinfo["status"]), (N, info["status"], oinfo["status"])
        assert np.isfinite(st).all() and np.isfinite(xs).all() and (info["status"] != -8).all(), N
        agree, total = agree + int((info["status_refine"] == oinfo["status_refine"]).sum()), total + b.B
        ok = info["status"] == 1
        dx += np.abs(xs - oxs).max(axis=1)[ok].tolist()
    assert agree >= 0.98 * total, (agree, total)
    assert max(dx) < 1e-4 and np.median(dx) < 1e-8, (max(dx), np.median(dx))


# ---- f: the polish (test_polish.py::test_device_polish_on_ragged_batches_and_other_keep_values) ----
@pytest.mark.slow
@pytest.mark.parametrize("row", POLISH, ids=ids)
def test_polish_matches_oracle(oracle, row):
    polished = 0
    for N in row[3]:
        b, _ = _batch(row, N, full=True)
        p = _params(polish=1)
        st, info, xs, _ = _run(b, p)
        ost, oinfo, oxs = _oracle(oracle, b, p)
        assert np.array_equal(info["status"], oinfo["status"]), (N, info["status"], oinfo["status"])
        same = (info["iters"] == oinfo["iters"]) & (info["status"] == 1)
        ok, ook = info["status_polish"] == 1, oinfo["status_polish"] == 1
        assert np.array_equal(ok[same], ook[same]), (N, ok, ook)
        both = ok & ook & same
        if both.any():
            assert np.abs(xs[both] - oxs[both]).max() < 1e-6 and np.abs(st[both] - ost[both]).max() < 1e-6, N
        polished += int(both.sum())
    assert polished >= 3, polished


# ---- g: the shapes without a Newton or polish kernel say so (test_newton.py::test_refinement_and_polish_on_a_shape_without_their_kernel_say_so, every such row) ----
@pytest.mark.slow
@pytest.mark.parametrize("row", NO_KERNEL, ids=ids)
def test_shapes_without_their_kernel_say_so(row):
    from path_optimizer_amd import abi

    for N in row[3]:
        b, _ = _batch(row, N, full=True)
        st, info, xs, _ = _run(b, _params(**dict(NEWTON, polish=1)))
        assert (info["status_polish"] == abi.PO_NOT_AVAILABLE).all(), (N, info["status_polish"])
        if row[2][0]:  # role-split: the Newton refinement runs, the polish has no kernel: the results of the headline without polish
            st0, info0, xs0, _ = _run(b, _params(**NEWTON))
            assert np.isin(info["status_refine"], (1, -1)).all() and np.array_equal(info["status_refine"], info0["status_refine"]), N
        else:  # single-level: neither kernel; the plain solve at the caller's eps, as with refine = 0
            st0, info0, xs0, _ = _run(b, _params())
            assert (info["status_refine"] == abi.PO_NOT_AVAILABLE).all() and (info0["status_refine"] == 0).all(), (N, info["status_refine"])
        assert np.array_equal(info["status"], info0["status"]) and np.array_equal(info["iters"], info0["iters"]) and np.array_equal(xs, xs0), N


# ---- h: the largest accepted length of each formulation / keep solves like the oracle; one more is refused ----
@pytest.mark.parametrize("form,keep", sorted(S.N_MAX), ids=[f"{S.FORM_NAMES[f]}-keep{k}" for f, k in sorted(S.N_MAX)])
def test_largest_accepted_length_solves_and_one_more_is_refused(oracle, form, keep):
    from path_optimizer_amd import binding, synth

    n_max = S.N_MAX[(form, keep)]
    shape = S.shape_of(form, n_max, keep)
    row = next(r for r in S.MATRIX if r[0] == form and r[2] == shape)
    row = (form, keep, shape, row[3])
    _osqp_faithful(oracle, row, n_max)
    rng = np.random.default_rng(keep)
    i = T.random_instance(rng, n_max + 1, ds=_ds(form, keep))
    one = lambda k: np.ascontiguousarray(i[k][None])
    big = synth.Batch(form, 1, n_max + 1, keep, one("ref_x"), one("ref_y"), one("ref_z"), one("ref_k"), one("ref_s"), one("bounds"), one("x0"), np.array([i["goal_z"]]),
                      one("max_k") if form == S.KPC else None, one("max_kp") if form == S.KPC else None)
    with pytest.raises(binding.PoError, match="unsupported"):
        binding.Engine(0).solve_batch(big)
