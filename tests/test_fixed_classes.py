"""Constant-class Newton kernels of the fixed lengths (csrc/po_newton_kernel.inc, newton_kernel_std).

The two Newton launches of KP's headline shape (N = 200, keep 4) exist a third time with the row classes BY TYPE as compile-time constants: every stage-local row an
inequality, the control row free.  A small launch ahead of the Newton launches (newton_std_select_kernel) decides which paths have those classes; they go to the
constant-class kernels, a path with other classes (a degenerate corridor at one stage, margin = 0) to the kernels without the constants, which run right behind them on
device-side lists.  No floating-point expression differs, so every comparison here is EXACT equality of states, x and every po_info field against the same solve with
po_debug_set "fixed_classes" 0; po_debug_get "fixed_classes_used" counts the paths the constant-class kernels took."""
import numpy as np
import pytest

# the headline setting (bench.py HEADLINE; tests/test_newton.py NEWTON)
NEWTON = dict(refine=2, refine_rounds=5, refine_extra_rounds=2, refine_eps=1e-8, refine_chain=2)
FALLBACK_FACTOR = 0.2  # tests/test_fixed_length.py: paths 19 and 30 of config 3 infeasible, thirteen go through newton_fallback_kernel
DEGENERATE = (2, 5)    # the paths of the mixed batch whose circle 0 is pinned at one stage ...
STAGE = 100            # ... this one (interior; on the CPU oracle at the headline setting all eight paths still end certified, in 33 .. 41 iterations)


def _engine(classes, slice_=None, **kw):
    from path_optimizer_amd import binding

    p = binding.default_params()
    for k, v in dict(NEWTON, **kw).items():
        setattr(p, k, v)
    e = binding.Engine(0, p)
    e.debug_set("fixed_classes", classes)
    if slice_ is not None:
        e.debug_set("newton_slice", slice_)
    return e


def _solve(b, classes, slice_=None, engine=None, order=None, **kw):
    """states, info, x of one host-pointer solve and its engine (a fresh one unless one is given)."""
    e = engine or _engine(classes, slice_, **kw)
    st, info, xs = e.solve_batch(b, want_x=True, order=order)
    return st.copy(), info.copy(), xs.copy(), e


def _assert_bitwise(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: states differ on {int((a[0] != b[0]).sum())} elements, max {np.abs(a[0] - b[0]).max():.3e}"
    assert np.array_equal(a[2], b[2]), f"{what}: x differs on {int((a[2] != b[2]).sum())} elements, max {np.abs(a[2] - b[2]).max():.3e}"
    for f in a[1].dtype.names:
        assert np.array_equal(a[1][f], b[1][f]), f"{what}: po_info.{f} differs on paths {np.flatnonzero(a[1][f] != b[1][f]).tolist()[:16]}"


def _both(b, slice_=None, what="", **kw):
    """The solve without and with the constant-class kernels: equal bit for bit; returns the latter."""
    off, on = _solve(b, 0, slice_, **kw), _solve(b, 1, slice_, **kw)
    assert off[3].debug_get("fixed_length_used") == 1 and on[3].debug_get("fixed_length_used") == 1
    assert off[3].debug_get("fixed_classes_used") == 0
    _assert_bitwise(off, on, what)
    return on


def _mixed_batch():
    """B = 8; paths 2 and 5 get lb == ub on circle 0 at one interior stage, at the corridor's midpoint: row 2 of that stage is an equality."""
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=8)
    for p in DEGENERATE:
        b.bounds[p, STAGE, 0, :] = 0.5 * (b.bounds[p, STAGE, 0, 0] + b.bounds[p, STAGE, 0, 1])
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("B,slice_", [(1, 0), (5, 0), (64, 0), (64, 3), (64, 8)])
def test_a_standard_batch_runs_the_constant_class_kernels_on_every_path(B, slice_):
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=B)
    assert b.N == 200 and b.keep == 4 and b.formulation == 0
    on = _both(b, slice_, f"B {B}, newton_slice {slice_}")
    assert (on[1]["status_refine"] == 1).all()
    assert on[3].debug_get("fixed_classes_used") == B
    assert on[3].debug_get("newton_list_ok") == (1 if slice_ else -1)


@pytest.mark.gpu
def test_a_uniform_batch_with_other_classes_is_left_to_the_kernels_without_the_constants():
    """margin = 0: row 1 (0 <= s1 <= margin) is an equality on every stage of every path — uniform for the warm start, not standard here."""
    from path_optimizer_amd import synth

    on = _both(synth.make_batch(3, B=5), 0, "margin 0", margin=0.0)
    assert (on[1]["status"] == 1).all()
    assert on[3].debug_get("fixed_classes_used") == 0


@pytest.mark.gpu
@pytest.mark.parametrize("slice_", [0, 3])
def test_a_mixed_batch_splits_between_the_two_sets_of_kernels(slice_):
    on = _both(_mixed_batch(), slice_, f"mixed batch, newton_slice {slice_}")
    assert (on[1]["status"] == 1).all() and (on[1]["status_refine"] == 1).all()
    assert on[3].debug_get("fixed_classes_used") == 8 - len(DEGENERATE)
    if slice_:
        assert on[3].debug_get("newton_list_ok") == 1


@pytest.mark.gpu
def test_the_constant_class_kernels_hand_over_to_the_fallback_rounds():
    """Corridors scaled by 0.2, the first 64 paths of config 3: 13 hand-backs to newton_fallback_kernel, paths 19 and 30 infeasible."""
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=64)
    b.bounds = b.bounds * FALLBACK_FACTOR
    off, on = _solve(b, 0), _solve(b, 1)
    nfb = (off[3].debug_get("fallback_paths"), on[3].debug_get("fallback_paths"))
    bad = (off[1]["status"] != 1) | (off[1]["status_refine"] != 1)
    print("fallback paths without / with the constants:", nfb, "not certified or infeasible:", np.flatnonzero(bad).tolist(), off[1]["status"][bad].tolist())
    assert nfb == (13, 13)
    assert np.flatnonzero(bad).tolist() == [19, 30] and off[1]["status"][bad].tolist() == [-3, -3]  # (primal infeasible through every fall-back round)
    assert off[3].debug_get("fixed_classes_used") == 0 and on[3].debug_get("fixed_classes_used") == 64  # (narrow corridors are still inequalities)
    _assert_bitwise(off, on, "fall-back case")


@pytest.mark.gpu
@pytest.mark.parametrize("end_heading", [1, 0])
def test_the_end_rows_keep_their_run_time_class(end_heading):
    """The end-heading window on (a finite row) and off (a free row): the class of the two end rows is not among the constants, so both batches are standard."""
    from path_optimizer_amd import synth

    on = _both(synth.make_batch(3, B=5), 0, f"end heading {end_heading}", constraint_end_heading=end_heading)
    assert (on[1]["status"] == 1).all()
    assert on[3].debug_get("fixed_classes_used") == 5


@pytest.mark.gpu
def test_a_reused_handle_starts_every_solve_with_empty_leftover_lists():
    """One handle solves the mixed batch and then a standard one of the same size, sliced: an entry or a count the first solve left on either leftover list would run
    a path a second time (or count wrong) in the second."""
    from path_optimizer_amd import synth

    mixed, standard = _mixed_batch(), synth.make_batch(3, B=8)
    e = _engine(1, 3)
    first = _solve(mixed, 1, engine=e)
    assert e.debug_get("fixed_classes_used") == 8 - len(DEGENERATE)
    again = _solve(standard, 1, engine=e)
    assert e.debug_get("fixed_classes_used") == 8 and e.debug_get("newton_list_ok") == 1
    _assert_bitwise(_solve(mixed, 1, 3), first, "first solve of the handle")
    _assert_bitwise(_solve(standard, 1, 3), again, "second solve on a used handle")


@pytest.mark.gpu
def test_a_captured_sliced_solve_replays_the_eager_result():
    """B = 64, newton_slice 8, refine_chain = 3, captured on a side stream (tests/test_fixed_scalars.py) and replayed twice on cleared outputs: the resets of the
    leftover lists and of the count are a part of the captured scale_kernel."""
    import torch

    from path_optimizer_amd import binding, synth

    b = synth.make_batch(3, B=64)
    outputs = lambda d: (d.out_states.cpu().numpy(), d.info_numpy(), d.out_x.cpu().numpy())
    ref = _engine(1, 8, refine_chain=3)
    d0 = binding.DeviceBatch(b, want_x=True)
    ref.solve_batch_device(d0)
    torch.cuda.synchronize()
    eager = outputs(d0)
    assert (eager[1]["status_refine"] == 1).all() and ref.debug_get("fixed_classes_used") == 64
    s = torch.cuda.Stream()
    eng = _engine(1, 8, refine_chain=3)
    try:
        eng.set_stream(s.cuda_stream)
        db = binding.DeviceBatch(b, want_x=True)
        torch.cuda.synchronize()
        eng.solve_batch_device(db)  # warm-up: sizes every block (a handle does not allocate during capture)
        s.synchronize()
        _assert_bitwise(eager, outputs(db), "eager warm-up on the side stream")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            eng.solve_batch_device(db)
        for i in (1, 2):
            db.out_states.zero_(); db.out_x.zero_(); db.out_info.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            _assert_bitwise(eager, outputs(db), f"replay {i}")
            assert eng.debug_get("fixed_classes_used") == 64
        del g
    finally:
        torch.cuda.synchronize()
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slice_", [0, 3])
def test_a_callers_order_keeps_steering_the_first_launch_and_changes_nothing(slice_):
    b = _mixed_batch()
    order = np.array([7, 5, 3, 1, 0, 2, 4, 6], dtype=np.int32)
    plain, hinted = _solve(b, 1, slice_), _solve(b, 1, slice_, order=order)
    assert hinted[3].debug_get("fixed_classes_used") == 8 - len(DEGENERATE)
    _assert_bitwise(plain, hinted, f"caller's order, newton_slice {slice_}")
