"""The fixed-length kernels' scalars and the fills moved into scale_kernel (csrc/po_fast.inc, csrc/po_scale.hpp, csrc/po_solve.cpp).

The length-specialised kernels of KP's headline shape (N = 200, keep 4) take the number of controls as a constant and keep a pass's wave-uniform row steps in scalar
registers.  Neither touches an operation or its order, so the claim is EXACT equality with the generic kernels — stricter than tests/test_fixed_length.py on purpose.

scale_kernel, the first launch of every solve, resets the park keys of the sliced Newton launches (-1: not parked) and the count of the fall-back work list; the two fills
that did it between the warm start and the Newton launches are gone.  What could go stale is tested here: a path the first launch never reaches, a handle used again for a
smaller batch, a captured solve replayed, and a ragged batch (generic kernels, same key initialisation)."""
import numpy as np
import pytest

# the headline setting (bench.py HEADLINE; tests/test_newton.py NEWTON)
NEWTON = dict(refine=2, refine_rounds=5, refine_extra_rounds=2, refine_eps=1e-8, refine_chain=2)
FALLBACK_FACTOR = 0.2  # tests/test_fixed_length.py: paths 19 and 30 of config 3 infeasible, thirteen go through newton_fallback_kernel


def _engine(slice_=None, fixed=None, **kw):
    from path_optimizer_amd import binding

    p = binding.default_params()
    for k, v in dict(NEWTON, **kw).items():
        setattr(p, k, v)
    e = binding.Engine(0, p)
    if fixed is not None:
        e.debug_set("fixed_length", fixed)
    if slice_ is not None:
        e.debug_set("newton_slice", slice_)
    return e


def _solve(b, slice_=None, fixed=None, engine=None):
    """states, info, x of one host-pointer solve, on a fresh engine unless one is given."""
    e = engine or _engine(slice_, fixed)
    st, info, xs = e.solve_batch(b, want_x=True)
    return st.copy(), info.copy(), xs.copy(), e


def _assert_bitwise(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: states differ on {int((a[0] != b[0]).sum())} elements, max {np.abs(a[0] - b[0]).max():.3e}"
    assert np.array_equal(a[2], b[2]), f"{what}: x differs on {int((a[2] != b[2]).sum())} elements, max {np.abs(a[2] - b[2]).max():.3e}"
    for f in a[1].dtype.names:
        assert np.array_equal(a[1][f], b[1][f]), f"{what}: po_info.{f} differs on paths {np.flatnonzero(a[1][f] != b[1][f]).tolist()[:16]}"


# ---- fixed against generic, bit for bit ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("B,slice_", [(1, 0), (5, 0), (64, 0), (64, 3), (64, 8)])
def test_fixed_kernels_equal_the_generic_ones_bit_for_bit(B, slice_):
    """B = 1 and 5 unsliced: the long loop of the single Newton launch (the cases that caught every register-allocation hazard so far); B = 64 as one launch and as the
    sliced pair parked after 3 / 8 steps."""
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=B)
    assert b.N == 200 and b.keep == 4 and b.formulation == 0
    gen, fix = _solve(b, slice_, 0), _solve(b, slice_, 1)
    assert gen[3].debug_get("fixed_length_used") == 0 and fix[3].debug_get("fixed_length_used") == 1
    _assert_bitwise(gen, fix, f"B {B}, newton_slice {slice_}")


@pytest.mark.gpu
def test_fixed_kernels_equal_the_generic_ones_through_the_fallback_rounds():
    """Corridors scaled by 0.2, the first 64 paths of config 3: hand-backs to the generic newton_fallback_kernel and two infeasible paths."""
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=64)
    b.bounds = b.bounds * FALLBACK_FACTOR
    gen, fix = _solve(b, None, 0), _solve(b, None, 1)
    assert gen[3].debug_get("fixed_length_used") == 0 and fix[3].debug_get("fixed_length_used") == 1
    nfb = (gen[3].debug_get("fallback_paths"), fix[3].debug_get("fallback_paths"))
    bad = (gen[1]["status"] != 1) | (gen[1]["status_refine"] != 1)
    print("fallback paths generic / fixed:", nfb, "not certified or infeasible:", np.flatnonzero(bad).tolist(), gen[1]["status"][bad].tolist())
    assert nfb[0] > 0 and nfb[0] == nfb[1] and bad.any()
    _assert_bitwise(gen, fix, "fall-back case")


# ---- the fills moved into scale_kernel -------------------------------------------------------------------------------------------------------------------------------

def _device_solve(b, slice_, order):
    import torch

    from path_optimizer_amd import binding

    e = _engine(slice_)
    db = binding.DeviceBatch(b, want_x=True)
    db.order = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(db.out_states.device)  # (set_order's upload, without its promise of a permutation)
    e.solve_batch_device(db)
    torch.cuda.synchronize()
    return db.out_states.cpu().numpy(), db.info_numpy(), db.out_x.cpu().numpy(), e


@pytest.mark.gpu
def test_a_path_the_order_leaves_out_is_not_parked():
    """A caller-side order that lists path 0 twice and path 5 never (the device-pointer entry trusts its caller): no workgroup of the first sliced launch writes path 5's
    key, so it must read "not parked" from scale_kernel's reset — the second launch's list stays what nw_sort_kernel promises and path 5 comes back as unsliced."""
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=8)
    order = np.array([0, 1, 2, 3, 4, 0, 6, 7], dtype=np.int32)
    sl, un = _device_solve(b, 3, order), _device_solve(b, 0, order)
    assert sl[3].debug_get("newton_list_ok") == 1 and un[3].debug_get("newton_list_ok") == -1
    assert 0 < sl[3].debug_get("newton_parked") <= 7
    assert np.array_equal(sl[0][5], un[0][5]) and np.array_equal(sl[2][5], un[2][5])
    for f in sl[1].dtype.names:
        assert sl[1][f][5] == un[1][f][5], f
    assert sl[1]["status"][5] != 1  # (nobody solved it)
    others = [0, 1, 2, 3, 4, 6, 7]
    assert (sl[1]["status"][others] == 1).all() and (sl[1]["status_refine"][others] == 1).all()


@pytest.mark.gpu
def test_a_reused_handle_starts_every_solve_with_fresh_keys_and_an_empty_list():
    """B = 64, then B = 8 of other paths on the same handle, both sliced: keys or a work-list count left by the first solve would show in the second."""
    from path_optimizer_amd import synth

    big, small = synth.make_batch(3, B=64), synth.make_batch(3, B=8, first_path=1000)
    e = _engine(8)
    first = _solve(big, engine=e)
    assert e.debug_get("newton_parked") > 0 and (first[1]["status_refine"] == 1).all()
    again = _solve(small, engine=e)
    assert e.debug_get("newton_list_ok") == 1
    fresh = _solve(small, 8)
    assert again[3].debug_get("newton_parked") == fresh[3].debug_get("newton_parked") >= 0
    _assert_bitwise(fresh, again, "second solve on a used handle")


@pytest.mark.gpu
@pytest.mark.parametrize("slice_", [None, 8])
def test_a_captured_solve_replays_the_eager_result(slice_):
    """One solve_batch_device captured on a side stream at the headline setting with refine_chain = 3 (tools/handle_contract_check.py, graph_capture), replayed twice on
    cleared outputs.  slice_ None: the engine's own choice (unsliced at this size); 8: the sliced pair, whose key reset is then a part of the captured scale_kernel."""
    import torch

    from path_optimizer_amd import binding, synth

    b = synth.make_batch(3, B=64)
    outputs = lambda d: (d.out_states.cpu().numpy(), d.info_numpy(), d.out_x.cpu().numpy())
    ref = _engine(slice_, refine_chain=3)
    d0 = binding.DeviceBatch(b, want_x=True)
    ref.solve_batch_device(d0)
    torch.cuda.synchronize()
    eager = outputs(d0)
    assert (eager[1]["status_refine"] == 1).all()
    s = torch.cuda.Stream()
    eng = _engine(slice_, refine_chain=3)
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
        del g
    finally:
        torch.cuda.synchronize()
        eng.close()


@pytest.mark.gpu
def test_a_ragged_batch_is_sliced_on_the_generic_kernels_with_the_same_key_reset():
    """n_points set: the generic kernels (fixed_length_used 0), sliced and unsliced — the bars of test_sliced_newton_launches_change_nothing_but_the_schedule
    (tests/test_newton.py)."""
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=64)
    b.n_points = np.random.default_rng(5).integers(60, 201, size=64).astype(np.int32)
    out = {sl: _solve(b, sl) for sl in (0, 8, 3)}
    for sl in (0, 8, 3):
        assert out[sl][3].debug_get("fixed_length_used") == 0
    assert out[0][3].debug_get("newton_list_ok") == -1 and out[8][3].debug_get("newton_list_ok") == 1 and out[3][3].debug_get("newton_list_ok") == 1
    assert out[3][3].debug_get("newton_parked") >= out[8][3].debug_get("newton_parked") > 0
    cert = (out[0][1]["status"] == 1) & (out[0][1]["status_refine"] == 1)
    assert cert.any()
    for sl in (8, 3):
        d_st, d_x = np.abs(out[sl][0] - out[0][0]), np.abs(out[sl][2] - out[0][2])
        print(f"ragged, newton_slice {sl}: certified {int(cert.sum())} of 64, max |d states| {d_st.max():.3e}, max |d x| {d_x.max():.3e}")
        for f in ("status", "status_refine", "status_polish"):
            assert np.array_equal(out[sl][1][f], out[0][1][f]), f
        assert d_st[cert].max() < 1e-8 and d_x[cert].max() < 1e-8
        assert d_st.max() < 1e-6 and d_x.max() < 1e-6
        assert np.abs(out[sl][1]["iters"] - out[0][1]["iters"]).max() <= 3 and (out[sl][1]["iters"] != out[0][1]["iters"]).mean() <= 0.05
