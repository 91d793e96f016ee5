"""Length-specialised kernels (csrc/po_fast.inc, Fast's NFIX): the uniform warm start and the two Newton launches of KP's headline shape (keep 4, one
lane per chunk) are compiled a second time with the LDS layout of a given path length as a constant, for the lengths of the Makefile's PO_FIXED_N (200).  Same operations in
the same order on the same LDS layout, state block and parking block; what the compiler folds away is address arithmetic (N and C themselves stay run-time values, so that the
floating-point code is compiled from the same blocks as in the generic kernels).  A non-ragged batch of a listed
length runs them, everything else the generic kernels; po_debug_set "fixed_length" 0 forces the generic ones and po_debug_get "fixed_length_used" says what the last solve ran.

GPU: fixed against generic through that switch, with the bars test_sliced_newton_launches_change_nothing_but_the_schedule applies to separately compiled kernels."""
import numpy as np
import pytest

# the headline setting (bench.py HEADLINE; tests/test_newton.py NEWTON)
NEWTON = dict(refine=2, refine_rounds=5, refine_extra_rounds=2, refine_eps=1e-8, refine_chain=2)
# Corridors scaled down as a third of the fuzz cases do (tests/test_gpu_fuzz.py: 0.5 or 0.7), but further: chosen on the CPU oracle at the headline setting.  At 0.5 and
# 0.6 every one of the 4 096 paths of BASELINE config 3 still ends certified (at 0.7 the first 512), and so do the first 64 down to 0.3; at 0.25 paths 22 and 61 end solved but
# not certified (489 / 575 iterations), at 0.2 paths 19 and 30 are primal infeasible (status -3 after 1 454 / 666 iterations, through every fall-back round), at 0.15 eleven are.
# 0.2: the largest factor at which the outcome is a certificate of infeasibility, which does not hang on rounding as "certified or not" at 0.25 does.
FALLBACK_FACTOR = 0.2


def _solve(b, fixed, slice_=None, **kw):
    """One solve of `b` on a fresh engine with the length-specialised kernels allowed (fixed = 1) or switched off (0): states, info, x, fixed_length_used, fallback_paths."""
    from path_optimizer_amd import binding

    p = binding.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    e = binding.Engine(0, p)
    e.debug_set("fixed_length", fixed)
    if slice_ is not None:
        e.debug_set("newton_slice", slice_)
    st, info, xs = e.solve_batch(b, want_x=True)
    return st.copy(), info.copy(), xs.copy(), e.debug_get("fixed_length_used"), e.debug_get("fallback_paths")


def _assert_same(gen, fix):
    """The bars of test_sliced_newton_launches_change_nothing_but_the_schedule (tests/test_newton.py) for two separately compiled sets of kernels."""
    assert gen[3] == 0 and fix[3] == 1, (gen[3], fix[3])
    gi, fi = gen[1], fix[1]
    for f in ("status", "status_refine", "status_polish"):
        assert np.array_equal(fi[f], gi[f]), (f, fi[f].tolist(), gi[f].tolist())
    cert = (gi["status"] == 1) & (gi["status_refine"] == 1)
    d_st, d_x = np.abs(fix[0] - gen[0]), np.abs(fix[2] - gen[2])
    d_it = np.abs(fi["iters"].astype(np.int64) - gi["iters"].astype(np.int64))
    print(f"fixed vs generic: certified {int(cert.sum())} of {len(cert)}; max |d states| {d_st.max():.3e} (certified {d_st[cert].max() if cert.any() else 0.0:.3e}), "
          f"max |d x| {d_x.max():.3e} (certified {d_x[cert].max() if cert.any() else 0.0:.3e}); iters differ on {float((d_it != 0).mean()):.3f} of the paths, by at most {int(d_it.max())}")
    if cert.any():
        assert d_st[cert].max() < 1e-8 and d_x[cert].max() < 1e-8
    assert d_st.max() < 1e-6 and d_x.max() < 1e-6
    assert d_it.max() <= 3 and (d_it != 0).mean() <= 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("B,slice_", [(1, 0), (5, 0), (64, 0), (64, 3), (64, 8)])
def test_fixed_length_kernels_compute_what_the_generic_ones_do(B, slice_):
    """N = 200, keep 4 at the headline setting.  B = 1 and 5 unsliced: the long loop of the single Newton launch on a small batch (the cases that caught the register-allocation
    hazard of DESIGN.md section 13); B = 64 as one launch and as the sliced pair (park after 3 / 8 steps, resume in the second launch)."""
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=B)
    assert b.N == 200 and b.keep == 4 and b.formulation == 0
    gen = _solve(b, 0, slice_, **NEWTON)
    fix = _solve(b, 1, slice_, **NEWTON)
    _assert_same(gen, fix)


def _fallback_batch():
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=64)
    b.bounds = b.bounds * FALLBACK_FACTOR
    return b


@pytest.mark.gpu
def test_a_fixed_newton_launch_hands_over_to_the_generic_fallback_rounds():
    """Corridors scaled down until a path of the batch is not certified (or infeasible): the fixed Newton kernel puts it on the work list, the generic
    newton_fallback_kernel takes it through the later rounds from the state block the fixed kernels left."""
    b = _fallback_batch()
    gen = _solve(b, 0, **NEWTON)
    fix = _solve(b, 1, **NEWTON)
    bad = (gen[1]["status"] != 1) | (gen[1]["status_refine"] != 1)
    print("not certified or infeasible (generic):", np.flatnonzero(bad).tolist(), gen[1]["status"][bad].tolist(), "fallback paths generic / fixed:", gen[4], fix[4])
    assert bad.any()
    assert gen[4] > 0 and fix[4] > 0  # both went through newton_fallback_kernel
    _assert_same(gen, fix)


@pytest.mark.gpu
def test_fixed_warm_start_alone_matches_the_generic_one():
    """refine = 0, 25 iterations: only the warm-start kernel runs."""
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=64)
    gen = _solve(b, 0, refine=0, max_iter=25)
    fix = _solve(b, 1, refine=0, max_iter=25)
    assert gen[3] == 0 and fix[3] == 1
    d_x = np.abs(fix[2] - gen[2]).max()
    print(f"warm start alone: iters {np.unique(gen[1]['iters']).tolist()}, statuses {np.unique(gen[1]['status']).tolist()}, max |d x| {d_x:.3e}")
    assert np.array_equal(fix[1]["iters"], gen[1]["iters"]) and (gen[1]["iters"] == 25).all()
    for f in ("status", "status_refine", "status_polish"):
        assert np.array_equal(fix[1][f], gen[1][f]), f
    assert d_x < 1e-8


@pytest.mark.gpu
def test_only_listed_lengths_of_the_headline_shape_take_the_fixed_kernels():
    from path_optimizer_amd import synth

    used = lambda b, fixed=1: _solve(b, fixed, **NEWTON)[3]
    assert used(synth.make_batch(3, B=4)) == 1
    assert used(synth.make_batch(3, B=4, N=199)) == 0
    assert used(synth.make_batch(3, B=4, N=201)) == 0
    ragged = synth.make_batch(3, B=4)
    ragged.n_points = np.full(4, 200, dtype=np.int32)  # (every path full length, but the batch says lengths are per path)
    assert used(ragged) == 0
    k8 = synth.make_batch(3, B=4, ds=0.14)
    assert k8.keep == 8 and k8.N == 200
    assert used(k8) == 0
    assert used(synth.make_batch(3, B=4), fixed=0) == 0
    # without the refinement the warm start alone decides
    assert _solve(synth.make_batch(3, B=4), 1)[3] == 1 and _solve(synth.make_batch(3, B=4, N=199), 1)[3] == 0
