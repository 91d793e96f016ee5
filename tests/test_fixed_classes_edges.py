"""The constant-class Newton split at every row, lane and list edge (csrc/po_fast.inc newton_std_select_kernel, csrc/po_kernels.hip
nw_sort_kernel, csrc/po_scale.hpp scale_kernel's resets, csrc/po_list_check.hpp).

Which compiled Newton kernel runs a path is decided per path on the device: a vote over the packed row classes (two bits a row, SPL = 4 stages a lane, 50 lanes), two
`order`-format lists for the first launch and a flagged split of the parked paths for the second.  newton_kernel_std on a path whose classes are not the standard ones is
SILENT: it computes with the wrong penalty class and returns a plausible point.  tests/test_fixed_classes.py holds the mechanism at one point of its input space (row 2
of lane 25, slot 0; B = 8); here the deviation visits every row, the first and the last lane, every slot, and the lists every length and the sort's uncached loops.

Every GPU case asserts (i) EXACT equality of states, x and every po_info field with the same solve under po_debug_set "fixed_classes" 0, (ii) the flag of every path,
read one by one (po_debug_get "fixed_classes_flag:<b>": a count cannot see two wrong flags that cancel), and, where the case says so, (iii) agreement with the CPU oracle
at the bars of tests/test_newton.py::test_device_newton_ragged_and_mixed_batches: equal status and status_refine, |iters difference| <= 6, max |x - x_oracle| < 1e-5.
Paths are independent, so the oracle's answer for a path is computed once per session and shared by every batch that holds the same path (_oracle)."""
import dataclasses
import functools
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_fixed_classes import DEGENERATE, FALLBACK_FACTOR, NEWTON, STAGE, _assert_bitwise, _engine, _mixed_batch, _solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N = 200, keep 4, one wave per path: lane = stage // 4, slot q = stage % 4, lanes 0 .. 49 hold stages
KINDS = ("eq0", "eq2", "free0", "free2", "free4", "free5", "free6", "free7")
FREE_STAGES = (0, 1, 3, 4, 100, 196, 199)         # lane 0 slots 0, 1, 3; lane 1; lane 25; lane 49 slots 0 and 3
EQ_STAGES = (100, 101, 102, 103, 197, 198, 199)   # every slot of lane 25, slots 1 .. 3 of lane 49 (a midpoint pin at stages 0 .. 5 is mostly primal infeasible)


# ---- batches ------------------------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _base(B):
    from path_optimizer_amd import synth

    b = synth.make_batch(3, B=B)
    assert b.N == 200 and b.keep == 4 and b.formulation == 0
    b.bounds.setflags(write=False)  # (shared: every user takes a copy of the bounds)
    return b


def _std(B):
    b = _base(B)
    return dataclasses.replace(b, bounds=b.bounds.copy())


def _take(b, idx):
    """The paths idx of b as a batch of their own (copies)."""
    idx = np.asarray(idx, dtype=np.int64)
    f = lambda a: None if a is None else np.ascontiguousarray(a[idx])
    return dataclasses.replace(b, B=len(idx), ref_x=f(b.ref_x), ref_y=f(b.ref_y), ref_z=f(b.ref_z), ref_k=f(b.ref_k), ref_s=f(b.ref_s), bounds=f(b.bounds), x0=f(b.x0),
                               goal_z=f(b.goal_z), max_k=f(b.max_k), max_kp=f(b.max_kp), n_points=f(b.n_points))


def _concat(*bs):
    f = lambda k: None if getattr(bs[0], k) is None else np.ascontiguousarray(np.concatenate([getattr(b, k) for b in bs], axis=0))
    return dataclasses.replace(bs[0], B=sum(b.B for b in bs), **{k: f(k) for k in ("ref_x", "ref_y", "ref_z", "ref_k", "ref_s", "bounds", "x0", "goal_z", "max_k", "max_kp", "n_points")})


def _deviate(b, p, stage, kind, at_x0=False):
    """One deviation from the standard row classes on one stage of path p (rows as in local_rows<F_KP>, csrc/po_device.hpp: row 2 is circle 0, row 3 circle 2, rows 4 / 5 the
    upper / lower side of circle 3, rows 6 / 7 of circle 1).  at_x0 (stage 0 only): the pin is where the fixed initial state puts the circle, 1e-3 inside the corridor."""
    from path_optimizer_amd import binding

    bd = b.bounds[p, stage]
    if kind in ("eq0", "eq2"):
        c = int(kind[2])
        v = 0.5 * (bd[c, 0] + bd[c, 1])
        if at_x0:
            assert stage == 0
            v = float(np.clip(b.x0[p, 0] + binding.default_params().d[c] * b.x0[p, 1], bd[c, 0] + 1e-3, bd[c, 1] - 1e-3))
        bd[c, :] = v
    elif kind in ("free0", "free2"):
        bd[int(kind[4]), :] = (-1e30, 1e30)
    else:
        c, side = {"free4": (3, 1), "free5": (3, 0), "free6": (1, 1), "free7": (1, 0)}[kind]
        bd[c, side] = 1e30 if side else -1e30


def _matrix_batch(kind):
    """B = 8: path i < 7 carries `kind` at the i-th stage of its list, path 7 stays standard."""
    b = _std(8)
    for p, stage in enumerate(EQ_STAGES if kind.startswith("eq") else FREE_STAGES):
        _deviate(b, p, stage, kind)
    return b, np.array([0] * 7 + [1])


def _lane0_pin_batch():
    """The equalities on lane 0: stage 0 of paths 0 .. 2 (circle 0) and 4 .. 6 (circle 2) pinned where x0 puts the circle — the row holds at the fixed initial state."""
    b = _std(8)
    for p in (0, 1, 2):
        _deviate(b, p, 0, "eq0", at_x0=True)
    for p in (4, 5, 6):
        _deviate(b, p, 0, "eq2", at_x0=True)
    return b, np.array([0, 0, 0, 1, 0, 0, 0, 1])


def _free_everywhere_batch():
    """Path 3: ub[3] = 1e30 on EVERY stage — row 4 free on every lane and slot: uniform classes (the uniform warm start takes it), not the standard ones."""
    b = _std(8)
    b.bounds[3, :, 3, 1] = 1e30
    return b, np.array([1, 1, 1, 0, 1, 1, 1, 1])


def _all_deviate_batch():
    """Every path deviates, path i by KINDS[i] at stage 100: nothing for the constant-class kernels."""
    b = _std(8)
    for p, kind in enumerate(KINDS):
        _deviate(b, p, 100, kind)
    return b, np.zeros(8, dtype=int)


MATRIX = dict({k: functools.partial(_matrix_batch, k) for k in KINDS}, lane0_pin=_lane0_pin_batch, free4_everywhere=_free_everywhere_batch, all_deviate=_all_deviate_batch)


def _pattern(B, pattern):
    """flag [B] of a list-edge batch: 0 = the path gets eq0 at stage 100."""
    f = np.ones(B, dtype=int)
    if pattern == "first":
        f[0] = 0
    elif pattern == "last":
        f[B - 1] = 0
    elif pattern == "alternating":
        f[0::2] = 0
    elif pattern == "odd":          # the complement of "alternating"
        f[1::2] = 0
    elif pattern == "all_but_first":
        f[1:] = 0
    elif pattern == "seventeenth":  # the 17th path of every sort thread's range when each owns 17 (B = 4097: 256 threads x 17 paths)
        f[16::17] = 0
    else:
        raise KeyError(pattern)
    return f


def _list_batch(B, pattern):
    b, flags = _std(B), _pattern(B, pattern)
    for p in np.flatnonzero(flags == 0):
        b.bounds[p, STAGE, 0, :] = 0.5 * (b.bounds[p, STAGE, 0, 0] + b.bounds[p, STAGE, 0, 1])
    return b, flags


MIXED_FLAGS = np.array([0 if p in DEGENERATE else 1 for p in range(8)])


def _skipped_batch():
    """_mixed_batch() and two paths the Newton launches skip: path 8 with a NaN bound (status -8), path 9 = path 19 of config 3 with its corridor scaled by
    FALLBACK_FACTOR as a whole (tests/test_fixed_classes.py: primal infeasible through every fall-back round)."""
    from path_optimizer_amd import synth

    nan = _take(_std(10), [8])
    nan.bounds[0, 50, 2, 0] = np.nan
    narrow = synth.make_batch(3, B=1, first_path=19)
    narrow.bounds = narrow.bounds * FALLBACK_FACTOR
    return _concat(_mixed_batch(), nan, narrow)


# ---- the oracle, once per path --------------------------------------------------------------------------------------------------------------------------------------------

_ORACLE = {}


def _oracle(b, paths=None):
    """status, status_refine, iters, x of the CPU oracle at the headline setting for the paths `paths` of b (default: all).  A path's answer depends on its own inputs
    only; it is computed the first time any batch holds these inputs and never changed."""
    from oracle import oracle_py
    from path_optimizer_amd import binding

    paths = np.arange(b.B) if paths is None else np.asarray(paths)
    keys = [hashlib.sha1(b"".join(np.ascontiguousarray(a[p]).tobytes() for a in (b.bounds, b.x0, b.ref_k, b.ref_s, b.ref_z, b.goal_z))).digest() for p in paths]
    first = {}
    for i, k in enumerate(keys):
        if k not in _ORACLE:
            first.setdefault(k, i)
    todo = list(first.values())
    if todo:
        p = binding.default_params()
        for k, v in NEWTON.items():
            setattr(p, k, v)
        _, info, xs = oracle_py.solve_batch(_take(b, paths[todo]), oracle_py.device_equivalent_params(p), want_x=True)
        for n, i in enumerate(todo):
            r = (int(info["status"][n]), int(info["status_refine"][n]), int(info["iters"][n]), xs[n].copy())
            r[3].setflags(write=False)
            _ORACLE[keys[i]] = r
    got = [_ORACLE[k] for k in keys]
    return dict(status=np.array([g[0] for g in got]), status_refine=np.array([g[1] for g in got]), iters=np.array([g[2] for g in got]), x=np.stack([g[3] for g in got]))


def _assert_oracle(out, b, what, paths=None, certified=True):
    """(iii): the device's paths `paths` against the oracle.  certified: each of them must be certified on the oracle too (the premise of the case)."""
    paths = np.arange(b.B) if paths is None else np.asarray(paths)
    o, info, xs = _oracle(b, paths), out[1][paths], out[2][paths]
    if certified:
        assert (o["status"] == 1).all() and (o["status_refine"] == 1).all(), (what, o["status"].tolist(), o["status_refine"].tolist())
    assert np.array_equal(info["status"], o["status"]), (what, info["status"].tolist(), o["status"].tolist())
    assert np.array_equal(info["status_refine"], o["status_refine"]), (what, info["status_refine"].tolist(), o["status_refine"].tolist())
    ok = o["status"] == 1
    d_it = np.abs(info["iters"].astype(int) - o["iters"].astype(int))[ok]
    err = np.abs(xs - o["x"])[ok].max() if ok.any() else 0.0
    print(f"{what}: oracle iterations {o['iters'][ok].min() if ok.any() else '-'} .. {o['iters'][ok].max() if ok.any() else '-'}, |iters difference| max {d_it.max() if ok.any() else '-'}, max |x - x_oracle| {err:.3e}")
    assert (d_it <= 6).all(), (what, info["iters"].tolist(), o["iters"].tolist())
    assert err < 1e-5, (what, err)


# ---- (i) and (ii) ---------------------------------------------------------------------------------------------------------------------------------------------------------

def _flags(e, B):
    return np.array([e.debug_get(f"fixed_classes_flag:{p}") for p in range(B)])


def _assert_flags(e, flags, what):
    got = _flags(e, len(flags))
    assert np.array_equal(got, flags), f"{what}: flags differ on paths {np.flatnonzero(got != flags).tolist()[:16]} (got {got[got != flags].tolist()[:16]})"
    assert e.debug_get("fixed_classes_used") == int(flags.sum()), what


def _both(b, flags, slice_, what, **kw):
    """The solve without and with the constant-class kernels: (i) equal bit for bit, (ii) every path's flag, the same paths parked, the lists in order and split as the
    flags say.  Returns the solve with them."""
    off, on = _solve(b, 0, slice_, **kw), _solve(b, 1, slice_, **kw)
    assert off[3].debug_get("fixed_length_used") == 1 and on[3].debug_get("fixed_length_used") == 1
    assert off[3].debug_get("fixed_classes_used") == 0 and off[3].debug_get("fixed_classes_flag:0") == -1
    _assert_bitwise(off, on, what)
    _assert_flags(on[3], flags, what)
    parked = (off[3].debug_get("newton_parked"), on[3].debug_get("newton_parked"))
    assert parked[0] == parked[1] and (parked[0] >= 0) == bool(slice_), (what, parked)
    assert off[3].debug_get("newton_list_ok") == on[3].debug_get("newton_list_ok") == (1 if slice_ else -1), what
    return on


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_every_deviating_path_of_the_vote_matrix_is_certified_by_the_oracle(oracle):
    """The premise of (a) and (b): each deviation leaves a path the oracle certifies at the headline setting (status 1, status_refine 1), so a device result that differs
    is the device's.  Measured: the vote matrix 34 .. 41 iterations (the stage-0 pins at the x0 value 36 .. 41), the 65 paths with and without the pin at stage 100 32 .. 51."""
    for name, make in MATRIX.items():
        b, flags = make()
        o = _oracle(b)
        print(name, "oracle iterations", o["iters"].tolist())
        assert (o["status"] == 1).all() and (o["status_refine"] == 1).all(), (name, o["status"].tolist(), o["status_refine"].tolist())
    for pattern in ("alternating", "odd"):
        b, flags = _list_batch(65, pattern)
        o = _oracle(b)
        assert (o["status"] == 1).all() and (o["status_refine"] == 1).all(), (pattern, np.flatnonzero(o["status_refine"] != 1).tolist())


def test_the_list_check_rejects_every_kind_of_bad_list(tmp_path):
    """csrc/po_list_check.hpp (what po_debug_get "newton_list_ok" runs) in a stand-alone program built by the host compiler with -fsanitize=address,undefined: correct
    single lists and pairs pass; a duplicate, a missing parked path, a listed path that is not parked, ascending keys, a tie in the wrong path order, a count above B, a
    negative id, a path on the list its flag does not name and a path on both lists are each rejected FOR THAT REASON (the program compares the named fault)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "list_check_test")
    src = os.path.join(ROOT, "path_optimizer_amd", "host", "test", "list_check_test.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("0 failed") and "FAIL" not in r.stdout and not r.stderr.strip()
    for case in ("a correct single list", "a correct pair", "a duplicate", "a missing parked path", "a listed path that is not parked", "descending order violated",
                 "a tie in the wrong path order", "a count above B", "a negative id", "a flag-0 path on the first list", "a flag-1 path on the second list",
                 "the same path on both lists"):
        assert any(l.startswith("ok") and case in l for l in r.stdout.splitlines()), case


# ---- (a) the vote matrix ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MATRIX))
def test_the_vote_reads_every_row_lane_and_slot(oracle, name):
    """One deviation on one stage of one path must take that path, and only it, away from the constant-class kernels: rows 2 and 3 as equalities and as free rows, rows
    4 .. 7 free, on the first lane, the second, lane 25 and the last, in every slot; a path with row 4 free on every stage; a batch in which every path deviates.  A vote
    that dropped a row's two bits, a slot or a lane, or took one lane's verdict for the wave's, flags a deviating path 1 here."""
    b, flags = MATRIX[name]()
    for slice_ in (0, 3):
        on = _both(b, flags, slice_, f"{name}, newton_slice {slice_}")
        _assert_oracle(on, b, f"{name}, newton_slice {slice_}")


# ---- (b) list edges -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("slice_", [0, 3, 8])
@pytest.mark.parametrize("B", [63, 64, 65, 257])
def test_the_split_at_list_lengths_of_zero_one_and_all_but_one(oracle, B, slice_):
    """eq0 at stage 100 on path 0 only, on path B - 1 only, on every other path, on every path but path 0: either list empty, of one entry, of half the batch, of all
    but one.  B below, at and above 64, and 257, where a sort thread owns two paths (256 threads).  Oracle: the whole batch up to B = 65, the first and the last 32 paths at 257."""
    ends = np.arange(B) if B <= 65 else np.r_[0:32, B - 32:B]
    for pattern in ("first", "last", "alternating", "all_but_first"):
        b, flags = _list_batch(B, pattern)
        what = f"B {B}, {pattern}, newton_slice {slice_}"
        on = _both(b, flags, slice_, what)
        _assert_oracle(on, b, what, ends)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["alternating", "seventeenth"])
def test_the_uncached_loops_of_the_sort_filter_by_the_flag(oracle, pattern):
    """B = 4097, newton_slice 3: each of nw_sort_kernel's 256 threads owns 17 paths, one more than it caches, so the count and the scatter loops behind the cache run
    (b >= lo + kCache) — with mixed flags, and in "seventeenth" with the non-standard paths exactly the ones only those loops see (17 t + 16).  A loop that read the key
    without the flag filter puts such a path on both lists."""
    b, flags = _list_batch(4097, pattern)
    on = _both(b, flags, 3, f"B 4097, {pattern}")
    assert on[3].debug_get("newton_parked") > 2048  # (nearly every path needs more than 3 steps: both lists are long)
    _assert_oracle(on, b, f"B 4097, {pattern}", np.r_[0:32, 4097 - 32:4097])


# ---- (c) one handle -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_one_handle_through_changing_sizes_and_the_switch(oracle):
    """The offsets of the lists depend on B (3B + 1, 5B + 2): one handle solves 64 alternating, the mixed 8, 65 standard, 64 alternating with the switch off, 64 with only
    path 0 standard with the switch on again, all sliced after 3 steps.  Every result and every read-back is a fresh engine's."""
    from path_optimizer_amd import binding

    steps = [(1, *_list_batch(64, "alternating")), (1, _mixed_batch(), MIXED_FLAGS), (1, _std(65), np.ones(65, dtype=int)), (0, *_list_batch(64, "alternating")),
             (1, *_list_batch(64, "all_but_first"))]
    e = _engine(1, 3)
    with pytest.raises(binding.PoError):
        e.debug_get("fixed_classes_flag:")
    assert e.debug_get("fixed_classes_flag:0") == -1  # (no solve yet)
    getters = lambda h: (h.debug_get("fixed_classes_used"), h.debug_get("newton_parked"), h.debug_get("newton_list_ok"))
    for n, (classes, b, flags) in enumerate(steps, 1):
        e.debug_set("fixed_classes", classes)
        used = _solve(b, classes, engine=e)
        fresh = _solve(b, classes, 3)
        _assert_bitwise(fresh, used, f"step {n} on the used handle")
        assert getters(e) == getters(fresh[3]) and getters(e)[2] == 1, (n, getters(e), getters(fresh[3]))
        if classes:
            _assert_flags(e, flags, f"step {n}")
            _assert_flags(fresh[3], flags, f"step {n}, fresh engine")
            for bad in (b.B, b.B + 1, 1 << 40):
                with pytest.raises(binding.PoError):
                    e.debug_get(f"fixed_classes_flag:{bad}")
            with pytest.raises(binding.PoError):
                e.debug_get("fixed_classes_flag:-1")
        else:
            assert e.debug_get("fixed_classes_used") == 0 and e.debug_get("fixed_classes_flag:0") == -1
        _assert_oracle(used, b, f"step {n}")


# ---- (d) capture --------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_captured_solve_splits_by_the_inputs_of_the_replay(oracle):
    """B = 64, newton_slice 8, refine_chain = 3, captured on the alternating batch (even paths pinned); between the two replays the bounds on the device are overwritten
    with those of the complement (odd paths pinned).  The select launch is a node of the graph: replay 2 is the eager solve of the second batch bit for bit, 32 paths
    flagged both times, the flags the complement."""
    import torch

    from path_optimizer_amd import binding

    outputs = lambda d: (d.out_states.cpu().numpy(), d.info_numpy(), d.out_x.cpu().numpy())
    batches = [_list_batch(64, "alternating"), _list_batch(64, "odd")]
    eager = []
    for b, flags in batches:
        per = []
        for classes in (0, 1):
            ref = _engine(classes, 8, refine_chain=3)
            d0 = binding.DeviceBatch(b, want_x=True)
            ref.solve_batch_device(d0)
            torch.cuda.synchronize()
            per.append(outputs(d0))
            if classes:
                _assert_flags(ref, flags, "eager")
            ref.close()
        _assert_bitwise(per[0], per[1], "eager, fixed_classes 0 against 1")
        _assert_oracle(per[1], b, "eager")
        eager.append(per[1])
    assert not np.array_equal(eager[0][0], eager[1][0])
    s = torch.cuda.Stream()
    eng = _engine(1, 8, refine_chain=3)
    try:
        eng.set_stream(s.cuda_stream)
        db = binding.DeviceBatch(batches[0][0], want_x=True)
        torch.cuda.synchronize()
        eng.solve_batch_device(db)  # warm-up: sizes every block (a handle does not allocate during capture)
        s.synchronize()
        _assert_bitwise(eager[0], outputs(db), "eager warm-up on the side stream")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            eng.solve_batch_device(db)
        for i in (0, 1):
            if i:
                db.bounds.copy_(torch.from_numpy(batches[1][0].bounds).to(db.bounds.device))
            db.out_states.zero_(); db.out_x.zero_(); db.out_info.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            _assert_bitwise(eager[i], outputs(db), f"replay {i + 1}")
            _assert_flags(eng, batches[i][1], f"replay {i + 1}")
            assert eng.debug_get("fixed_classes_used") == 32 and eng.debug_get("newton_list_ok") == 1
        del g
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---- (e) paths the Newton launches skip -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("slice_", [0, 3])
def test_skipped_paths_inside_a_mixed_batch(oracle, slice_):
    """The mixed batch and two paths no Newton launch works on to the end: path 8 has a NaN bound — status -8, status_refine 0, zero outputs —, path 9 (path 19 of config 3,
    corridor x 0.2) is primal infeasible on the oracle, status -3 and status_refine -1, through every fall-back round.  Statuses are the oracle's, the eight others are held
    to the full bars.  Path 9's narrow rows are still inequalities (flag 1); the class of a NaN bound is whatever the comparisons of a build without NaN semantics give, so
    path 8's flag is only required to be a flag."""
    b = _skipped_batch()
    off, on = _solve(b, 0, slice_), _solve(b, 1, slice_)
    what = f"skipped paths, newton_slice {slice_}"
    _assert_bitwise(off, on, what)
    got = _flags(on[3], 10)
    assert np.array_equal(got[:8], MIXED_FLAGS) and got[9] == 1 and got[8] in (0, 1), got.tolist()
    assert on[3].debug_get("fixed_classes_used") == int(got.sum())
    assert off[3].debug_get("newton_parked") == on[3].debug_get("newton_parked")
    assert on[3].debug_get("newton_list_ok") == (1 if slice_ else -1)
    o = _oracle(b)
    print(what, "oracle status", o["status"].tolist(), "status_refine", o["status_refine"].tolist(), "device", on[1]["status"].tolist(), on[1]["status_refine"].tolist())
    assert o["status"][8] == -8 and o["status"][9] == -3  # (what the docstring says the oracle reported)
    assert on[1]["status"][8] == -8 and on[1]["status_refine"][8] == 0 and (on[0][8] == 0).all() and (on[2][8] == 0).all()
    _assert_oracle(on, b, what, certified=False)
    _assert_oracle(on, b, what, np.arange(8))


# ---- (f) a malformed caller order -----------------------------------------------------------------------------------------------------------------------------------------

def _device_solve(b, classes, slice_, order, engine=None):
    import torch

    from path_optimizer_amd import binding

    e = engine or _engine(classes, slice_)
    db = binding.DeviceBatch(b, want_x=True)
    if order is not None:
        db.order = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(db.out_states.device)  # (set_order's upload, without its promise of a permutation)
    e.solve_batch_device(db)
    torch.cuda.synchronize()
    return db.out_states.cpu().numpy(), db.info_numpy(), db.out_x.cpu().numpy(), e


@pytest.mark.gpu
@pytest.mark.parametrize("handle", ["fresh", "used"])
def test_a_malformed_order_that_repeats_and_drops_non_standard_paths(oracle, handle):
    """The device entry trusts its caller: the order gives the non-standard path 2 twice and never reaches the non-standard path 5.  Path 5's key and flag are what
    scale_kernel's resets left (not parked, flag 0), the lists stay what the sort promises, path 5 comes back as from the unsliced solve and nobody solved it.
    "used": the handle has just solved the standard batch, in which path 5's flag was 1 — a reset that skipped the flags shows here."""
    b = _mixed_batch()
    order = np.array([0, 1, 2, 3, 4, 2, 6, 7], dtype=np.int32)
    flags = MIXED_FLAGS.copy()  # (path 5: flag 0 because nobody voted on it)
    others = [0, 1, 2, 3, 4, 6, 7]
    out = {}
    for classes, slice_ in ((1, 3), (1, 0), (0, 3), (0, 0)):
        e = None
        if handle == "used":
            e = _engine(classes, slice_)
            first = _device_solve(_std(8), classes, slice_, None, engine=e)
            assert (first[1]["status_refine"] == 1).all() and e.debug_get("fixed_classes_used") == (8 if classes else 0)
        out[classes, slice_] = _device_solve(b, classes, slice_, order, engine=e)
    for slice_ in (3, 0):
        on, off = out[1, slice_], out[0, slice_]
        _assert_bitwise(off, on, f"malformed order, newton_slice {slice_}")
        _assert_flags(on[3], flags, f"malformed order, newton_slice {slice_}")
        assert on[3].debug_get("fixed_classes_flag:5") == 0
        assert on[3].debug_get("newton_list_ok") == off[3].debug_get("newton_list_ok") == (1 if slice_ else -1)
        assert on[3].debug_get("newton_parked") == off[3].debug_get("newton_parked")
        _assert_oracle(on, b, f"malformed order, newton_slice {slice_}", others)
    sl, un = out[1, 3], out[1, 0]
    assert 0 < sl[3].debug_get("newton_parked") <= 7
    assert np.array_equal(sl[0][5], un[0][5]) and np.array_equal(sl[2][5], un[2][5])
    for f in sl[1].dtype.names:
        assert sl[1][f][5] == un[1][f][5], f
    assert sl[1]["status"][5] != 1  # (nobody solved it)
    assert (sl[1]["status"][others] == 1).all() and (sl[1]["status_refine"][others] == 1).all()
