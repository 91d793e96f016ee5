"""CPU checks of the solve entry's schedule (csrc/po_solve.cpp: plan_solve, exported as po_plan_solve): what a solve will launch — split, state block, polish, sliced,
fixed-length kernels, the two PO_NOT_AVAILABLE marks, the read-back of the fallback count, the warm start's eps multiplier — as a function of the parameters, the
resolved shape, the batch size, raggedness, the two developer switches and the device's wave slots.  The expected values are written out from the conditions of
DESIGN.md section 34, not computed by a twin.  Every (formulation, keep, N) is one of a row of tests/shape_table.py: MATRIX, so the shape is a reachable one."""
import ctypes
import os
import sys

import pytest

import shape_table as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab_headline import HEADLINE  # noqa: E402  (refine 2, 5 rounds + 2 extra, refine_chain 2)

FIELDS = ("split", "state", "polish", "sliced", "fixed", "no_refine", "no_polish", "read_back", "warm_decades")
PO_ERR_UNSUPPORTED = -3


@pytest.fixture(scope="module")
def L():
    from path_optimizer_amd import binding

    lib = binding.lib()
    lib.po_plan_solve.restype = ctypes.c_int
    lib.po_plan_solve.argtypes = [ctypes.c_int] * 14 + [ctypes.POINTER(ctypes.c_int)]
    return lib


def shape_row(form, keep, shape, N=None):
    """(form, keep, N) of the MATRIX row of this shape: N itself when the row's lengths span it, else the row's middle boundary length."""
    (row,) = [r for r in S.MATRIX if r[0] == form and r[1] == keep and r[2] == shape]
    lengths = row[3]
    if N is None:
        N = lengths[1]
    assert lengths[0] <= N <= lengths[-1], (S.row_id(row), N)
    return form, keep, N


HEAD = shape_row(S.KP, 4, (True, 64, 4, 1), 200)         # the headline: one lane per chunk, one wave, a listed length
TWO_WAVE = shape_row(S.KP, 4, (True, 128, 4, 1))         # two-level on two waves
SINGLE = shape_row(S.KP, 17, (False, 64, 2, 1))          # the single-level mapping: no state block, neither Newton nor polish kernel
ROLE_SPLIT = shape_row(S.KP, 8, (True, 64, 4, 2))        # role-split: Newton kernels, no polish kernel


def plan(L, where, B=4096, ragged=0, polish=0, nw_slice=8, forced=0, fixed_on=1, wave_slots=1024, **params):
    form, keep, N = where
    p = dict(HEADLINE, **params)
    out = (ctypes.c_int * 9)(*([-1] * 9))
    rc = L.po_plan_solve(form, N, keep, B, ragged, p["refine"], p["refine_rounds"], p["refine_extra_rounds"], p["refine_chain"], polish, nw_slice, forced, fixed_on,
                         wave_slots, out)
    assert rc == 0, (where, rc)
    return dict(zip(FIELDS, out))


def want(**kw):
    base = dict(split=0, state=0, polish=0, sliced=0, fixed=0, no_refine=0, no_polish=0, read_back=1, warm_decades=4)
    assert set(kw) <= set(base)
    return dict(base, **kw)


def test_headline_is_split_sliced_and_fixed(L):
    passed_on = dict(refine=2, refine_rounds=5, refine_extra_rounds=2, refine_chain=2)  # what the expected values of this file were written for
    assert {k: HEADLINE[k] for k in passed_on} == passed_on
    assert plan(L, HEAD) == want(split=1, state=1, sliced=1, fixed=1)


def test_slicing_needs_two_rounds_of_one_wave_paths_or_the_switch(L):
    assert plan(L, HEAD, B=2048) == want(split=1, state=1, sliced=1, fixed=1)  # B >= 2 * wave_slots
    assert plan(L, HEAD, B=2047) == want(split=1, state=1, fixed=1)
    assert plan(L, HEAD, B=2047, forced=1) == want(split=1, state=1, sliced=1, fixed=1)
    assert plan(L, HEAD, B=2047, wave_slots=512) == want(split=1, state=1, sliced=1, fixed=1)
    assert plan(L, HEAD, nw_slice=0) == want(split=1, state=1, fixed=1)  # newton_slice = 0: one launch
    assert plan(L, HEAD, nw_slice=0, forced=1) == want(split=1, state=1, fixed=1)
    assert plan(L, TWO_WAVE) == want(split=1, state=1)  # nt == 128: not sliced unless forced (and no listed length)
    assert plan(L, TWO_WAVE, forced=1) == want(split=1, state=1, sliced=1)


def test_fixed_length_kernels_need_the_switch_a_uniform_batch_and_a_listed_length(L):
    assert plan(L, HEAD, ragged=1) == want(split=1, state=1, sliced=1)
    assert plan(L, HEAD, fixed_on=0) == want(split=1, state=1, sliced=1)
    assert plan(L, shape_row(S.KP, 4, (True, 64, 4, 1), 199)) == want(split=1, state=1, sliced=1)  # the same row, a length that is not listed
    assert plan(L, HEAD, refine=0) == want(fixed=1)  # (the plain solve runs the length's warm-start kernel too)


def test_shapes_without_a_kernel_get_the_marks(L):
    # single-level: no state block, so no split and no polish, and both marks
    assert plan(L, SINGLE, polish=1) == want(no_refine=1, no_polish=1)
    assert plan(L, SINGLE) == want(no_refine=1)
    assert plan(L, SINGLE, refine=0, polish=1) == want(no_polish=1)
    # role-split: the Newton kernels exist, the polish kernel does not
    assert plan(L, ROLE_SPLIT, polish=1) == want(split=1, state=1, sliced=1, no_polish=1)
    # a shape with both
    assert plan(L, HEAD, polish=1) == want(split=1, state=1, polish=1, sliced=1, fixed=1)


def test_state_block_only_when_something_reads_it(L):
    assert plan(L, HEAD, refine=0) == want(fixed=1)
    assert plan(L, HEAD, refine=0, polish=1) == want(state=1, polish=1, fixed=1)
    assert plan(L, ROLE_SPLIT, refine=0, polish=1) == want(state=1, no_polish=1)  # (wanted before the polish kernel is looked for, as the solve kernels write it)


def test_rounds_that_do_not_fit_the_status_switch_the_split_off(L):
    assert plan(L, HEAD, refine_rounds=29, refine_extra_rounds=2) == want(split=1, state=1, sliced=1, fixed=1, warm_decades=28)
    assert plan(L, HEAD, refine_rounds=30, refine_extra_rounds=2) == want(state=1, fixed=1, no_refine=1, warm_decades=29)
    assert plan(L, HEAD, refine_rounds=0, refine_extra_rounds=31) == want(state=1, fixed=1, no_refine=1, warm_decades=0)


def test_count_is_read_back_unless_the_chain_is_asynchronous(L):
    assert plan(L, HEAD, refine_chain=3) == want(split=1, state=1, sliced=1, fixed=1, read_back=0)
    assert plan(L, HEAD, refine_chain=2)["read_back"] == 1


@pytest.mark.parametrize("rounds, multiplier", [(0, 1.0), (1, 1.0), (5, 1e4)])
def test_warm_start_eps_multiplier(L, rounds, multiplier):
    got = plan(L, HEAD, refine_rounds=rounds)
    assert got == want(split=1, state=1, sliced=1, fixed=1, warm_decades=got["warm_decades"])
    assert 10.0 ** got["warm_decades"] == multiplier


def test_unsupported_length_is_refused(L):
    out = (ctypes.c_int * 9)()
    n_max = S.N_MAX[(S.KP, 4)]
    assert L.po_plan_solve(S.KP, n_max + 1, 4, 8, 0, 2, 5, 2, 2, 0, 8, 0, 1, 1024, out) == PO_ERR_UNSUPPORTED
    assert L.po_plan_solve(S.KP, n_max, 4, 8, 0, 2, 5, 2, 2, 0, 8, 0, 1, 1024, out) == 0
