"""CPU checks of the kernel-shape table (tests/shape_table.py): the Python twin of pick_shape / resolve_shape agrees with the library's host-side queries at every
length, the table PO_SHAPE_ROWS instantiates exactly the reachable two-level shapes and every reachable shape equals exactly one of its rows, the size and capability
queries answer what they answered before the table, MATRIX (the rows tests/test_shape_matrix.py runs on the GPU) has a row for every reachable shape, and the largest
accepted length of each formulation / keep is pinned."""
import ctypes
import functools
import os
import re

import pytest

import shape_table as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from path_optimizer_amd import binding

    lib = binding.lib()
    for name in ("po_shape_threads", "po_polish_state_doubles", "po_newton_park_doubles", "po_has_polish_kernel"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [ctypes.c_int] * 4
    lib.po_lds_bytes.restype = ctypes.c_size_t
    lib.po_lds_bytes.argtypes = [ctypes.c_int] * 4
    return lib


@pytest.fixture(scope="module")
def lds(L):
    return functools.lru_cache(maxsize=None)(S.lds_bytes)


@pytest.fixture(scope="module")
def reach(lds):
    return S.reachable(lds)


def test_twin_agrees_with_the_library_at_every_length(L, lds):
    n = 0
    for form, keeps in S.KEEPS.items():
        for keep in keeps:
            accepted = []
            for N in S.N_GRID:
                C = S.problem_C(form, N, keep)
                s = S.shape_of(form, N, keep, lds)
                where = (S.FORM_NAMES[form], keep, N, s)
                threads = L.po_shape_threads(form, N, C, keep)
                nbytes = L.po_lds_bytes(form, N, C, keep)
                if s is None:
                    # refused: no candidate (the library answers 0 threads and 1 GB), or the resolved shape needs more than 160 KB of LDS
                    assert nbytes > S.LDS_LIMIT, where
                    assert (threads == 0) == (S.pick_shape(form, N, C, keep) is None), where
                    continue
                accepted.append(N)
                two, nt, spl, nwx = s
                assert threads == nt, (where, threads)
                assert nbytes <= S.LDS_LIMIT, (where, nbytes)
                assert (L.po_polish_state_doubles(form, N, C, keep) > 0) == two, where
                assert (L.po_newton_park_doubles(form, N, C, keep) > 0) == two, where
                assert bool(L.po_has_polish_kernel(form, N, C, keep)) == S.has_polish_kernel(s), where
                n += 1
            # the accepted lengths are one interval 2 .. N_max: a longer path never fits again
            assert accepted == list(range(2, accepted[-1] + 1)), (S.FORM_NAMES[form], keep)
    assert n > 15000


def _instances():
    """{form: [(two, spl, nt, nwx, group), ...]}: the rows of PO_SHAPE_ROWS (po_solve_common.hpp), the table of the shapes the library instantiates."""
    src = open(os.path.join(ROOT, "path_optimizer_amd", "csrc", "po_solve_common.hpp")).read().replace("\\\n", " ")
    body, = re.findall(r"^#define PO_SHAPE_ROWS\(X\)(.*)$", src, flags=re.M)
    rows = re.findall(r"X\(F_(KPC|KP|K), (true|false), (\d+), (\d+), (\d+), (kGrp\w+)\)", body)
    assert len(rows) == body.count("X(") and rows, body
    out = {}
    for form, two, spl, nt, nwx, group in rows:
        out.setdefault({"KP": S.KP, "KPC": S.KPC, "K": S.K}[form], []).append((two == "true", int(spl), int(nt), int(nwx), group))
    return out


def test_two_level_instances_are_exactly_the_reachable_shapes(reach):
    inst = _instances()
    assert set(inst) == {S.KP, S.KPC, S.K}
    for form, rows in inst.items():
        have = {(spl, nt, nwx) for two, spl, nt, nwx, _ in rows if two}
        want = {(spl, nt, nwx) for (f, (two, nt, spl, nwx)) in reach if f == form and two}
        assert have - want == set(), (S.FORM_NAMES[form], "instantiated but never reached (dead kernels in every kind of object):", sorted(have - want))
        assert want - have == set(), (S.FORM_NAMES[form], "reachable but not instantiated (the launch answers not-supported):", sorted(want - have))
        # the dispatch is by equality: every reachable shape, single-level ones included, equals exactly one row, and no row appears twice
        keys = [(two, nt, spl, nwx) for two, spl, nt, nwx, _ in rows]
        assert len(set(keys)) == len(keys), (S.FORM_NAMES[form], sorted(k for k in set(keys) if keys.count(k) > 1))
        for (f, s) in reach:
            if f == form:
                assert keys.count(s) == 1, (S.FORM_NAMES[form], s)
        # the single-level rows are pick_shape's five candidates
        assert {(nt, spl) for two, nt, spl, nwx in keys if not two} == {(64, 2), (64, 4), (128, 4), (256, 2), (256, 4)}, S.FORM_NAMES[form]


def test_size_and_capability_queries_are_pinned(L):
    """The library's answers at every MATRIX row's boundary lengths and at the headline (KP, keep 4, N = 200) equal tests/golden/shape_queries.json, recorded with
    tools/shape_query_dump.py from the library as it was before the shape table replaced the dispatch chains.  po_polish_state_doubles and po_newton_park_doubles size
    device buffers: a value that comes out smaller is an out-of-bounds write on the GPU."""
    import json
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shape_query_dump as D

    want = json.load(open(os.path.join(ROOT, "tests", "golden", "shape_queries.json")))
    points = D.golden_points()
    assert [tuple(r[:3]) for r in want] == points and (S.KP, 4, 200) in points
    got = D.query(L, points)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


def test_matrix_has_a_row_for_every_reachable_shape(reach, lds):
    rows = {(form, shape) for form, _, shape, _ in S.MATRIX}
    assert len(rows) == len(S.MATRIX), "one row per (formulation, shape)"
    assert rows == set(reach), ("shapes without a row:", sorted(set(reach) - rows), "rows of no reachable shape:", sorted(rows - set(reach)))
    for row in S.MATRIX:
        form, keep, shape, lengths = row
        assert keep in reach[(form, shape)], S.row_id(row)
        assert lengths == S.boundary_lengths(form, keep, shape, lds), (S.row_id(row), lengths, S.boundary_lengths(form, keep, shape, lds))
        assert all(S.shape_of(form, N, keep, lds) == shape for N in lengths), S.row_id(row)
        m = [N for N in lengths if N % 4 and (keep == 1 or N % keep)]
        assert m, (S.row_id(row), "a length that is a multiple of neither 4 nor keep")
    assert len({S.row_id(r) for r in S.MATRIX}) == len(S.MATRIX)


def test_refusal_limits_are_pinned(lds):
    # keep 1 / 2: C <= NT of the largest block (512 chunks of one / two stages: the single-level (256, 4) block holds keep 2 at 513 only); every other limit is the LDS of the
    # single-level (256, 4) block (keep 4: 875, not 1024)
    assert set(S.N_MAX) >= {(S.KP, k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 17)} | {(S.KPC, 4), (S.K, 1)}
    for (form, keep), n_max in S.N_MAX.items():
        assert S.largest_accepted(form, keep, lds) == n_max, (S.FORM_NAMES[form], keep)
        assert S.shape_of(form, n_max, keep, lds) is not None and S.shape_of(form, n_max + 1, keep, lds) is None, (S.FORM_NAMES[form], keep)
