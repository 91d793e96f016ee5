"""CPU checks of the kernel-shape table (tests/shape_table.py): the Python twin of pick_shape / resolve_shape agrees with the library's host-side queries at every
length, PO_TWO_SHAPES instantiates exactly the reachable two-level shapes and routes each one to its own instance, MATRIX (the rows tests/test_shape_matrix.py runs
on the GPU) has a row for every reachable shape, and the largest accepted length of each formulation / keep is pinned."""
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
    """{form: [(guard, (spl, nt, nwx)), ...]} in dispatch order, parsed from the full build's PO_TWO_SHAPES (po_solve_common.hpp) with every shape group's macros expanded."""
    src = open(os.path.join(ROOT, "path_optimizer_amd", "csrc", "po_solve_common.hpp")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S).replace("\\\n", " ")
    defs = {}
    for name, args, body in re.findall(r"^#define (PO_\w+)\(([^)]*)\)(.*)$", src, flags=re.M):
        if "X(" in body or "PO_" in body:
            defs.setdefault(name, []).append(([a.strip() for a in args.split(",")], body))
    # PO_TWO_SHAPES: the full build's definition (the dev build's one-shape variant has no `if constexpr`); the group macros: their non-empty definitions
    two = [b for _, b in defs.pop("PO_TWO_SHAPES") if "if constexpr" in b]
    assert len(two) == 1

    def expand(text, depth=0):
        assert depth < 5
        def sub(m):
            name, actual = m.group(1), [a.strip() for a in m.group(2).split(",")]
            if name not in defs:
                return m.group(0)
            (formal, body), = defs[name]
            for f, a in zip(formal, actual):
                body = re.sub(rf"\b{f}\b", a, body)
            return expand(body, depth + 1)
        return re.sub(r"\b(PO_\w+)\(([^()]*)\)", sub, text)

    out = {}
    for cond, body in re.findall(r"if constexpr \(([^)]*)\)\s*\{([^{}]*)\}", two[0]):
        body = expand(body)
        stmts = re.findall(r"if \(([^)]*)\)\s*X\((\d+),\s*(\d+),\s*(\d+)\)\s*;", body)
        assert len(stmts) == body.count("X("), body
        for form in (S.KP, S.KPC, S.K):
            if eval(cond, {"F": form, "F_KP": S.KP, "F_KPC": S.KPC, "F_K": S.K}):
                out.setdefault(form, []).extend((g, tuple(int(v) for v in x)) for g, *x in stmts)
    return out


def _routes(guard, shape):
    _, nt, spl, nwx = shape
    return eval(guard.replace("&&", " and ").replace("s.", ""), {"nt": nt, "spl": spl, "nwx": nwx})


def test_two_level_instances_are_exactly_the_reachable_shapes(reach):
    inst = _instances()
    assert set(inst) == {S.KP, S.KPC, S.K}
    for form, stmts in inst.items():
        have = {(spl, nt, nwx) for _, (spl, nt, nwx) in stmts}
        want = {(spl, nt, nwx) for (f, (two, nt, spl, nwx)) in reach if f == form and two}
        assert have - want == set(), (S.FORM_NAMES[form], "instantiated but never reached (dead kernels in every kind of object):", sorted(have - want))
        assert want - have == set(), (S.FORM_NAMES[form], "reachable but not instantiated (the launch answers not-my-shape):", sorted(want - have))
        # the dispatch: the first guard a reachable shape satisfies names that very shape
        for (f, s) in reach:
            if f == form and s[0]:
                first = next((x for g, x in stmts if _routes(g, s)), None)
                assert first == (s[2], s[1], s[3]), (S.FORM_NAMES[form], s, first)


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
