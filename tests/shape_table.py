"""The kernel shapes of the QP solve, restated in Python (csrc/po_solve_common.hpp: pick_shape / resolve_shape).

A shape is (two, nt, spl, nwx): two-level or single-level mapping, threads per path, stages per lane and lane mapping (1 one lane per chunk, 2 / 3 role-split,
4 / 5 multi-group; 1 on the single-level mapping).  Every two-level shape is its own instance of the solve, Newton, fallback and polish kernels, with its own
register allocation, so every reachable shape needs a test that runs it.  The library states the shapes it instantiates as data (PO_SHAPE_ROWS in
po_solve_common.hpp: one row per shape, matched by equality, with the group of objects that holds it).  tests/test_shape_table.py checks this twin against the
library's host-side queries over every length, and that table against the shapes the twin can reach; MATRIX below lists one row per reachable (formulation, shape)
with its boundary lengths, and tests/test_shape_matrix.py runs every row against the oracle on the GPU.

The LDS bytes of a shape are not restated: `lds_bytes` asks the library (po_lds_bytes, the size of the shape it resolved).  Where the library keeps the
two-level shape that is the size of the candidate, which is what resolve_shape's fallback tests; at the lengths tested (2 .. 1100) the fallback to the
single-level mapping never fires (the NT x SPL and chunk limits come first), and a change that makes it fire shows up as a disagreement in the grid test."""
import ctypes

KP, KPC, K = 0, 1, 2
FORM_NAMES = {KP: "KP", KPC: "KPC", K: "K"}
LDS_LIMIT = 160 * 1024
N_GRID = range(2, 1101)
KEEPS = {KP: range(1, 21), KPC: (4,), K: (1,)}


def problem_C(form, N, keep):
    """C of po_problem_dims: the number of held controls (K: N - 1 steering variables, none held)."""
    return N - 1 if form == K else (N + keep - 2) // keep


def lds_bytes(form, N, keep):
    from path_optimizer_amd import binding

    L = binding.lib()
    L.po_lds_bytes.restype = ctypes.c_size_t
    L.po_lds_bytes.argtypes = [ctypes.c_int] * 4
    return L.po_lds_bytes(form, N, problem_C(form, N, keep), keep)


def pick_shape(form, N, C, keep):
    no_u = form == K
    if no_u:
        C = 0
    keep_max = 16 if form == KP else 4
    if no_u or 1 <= keep <= keep_max:
        if not no_u and keep >= 6:
            spl, chunks = (keep + 1) // 2, (N + keep - 1) // keep
            if chunks <= 32:
                return (True, 64, spl, 2 + (keep & 1))
            if chunks <= 64 and keep <= 8:
                return (True, 128, spl, 2 + (keep & 1))
        else:
            if form == KP and keep in (1, 2):
                chunks = (N + 3) // 4
                if chunks <= 64:
                    return (True, 64, 4, 4 if keep == 1 else 5)
                if chunks <= 128:
                    return (True, 128, 4, 4 if keep == 1 else 5)
            spl = (2 if N <= 128 else 4) if no_u else keep
            for nt in (64, 128):
                if nt == 128 and spl > 4:
                    break
                if N <= nt * spl and C <= nt:
                    return (True, nt, spl, 1)
    for nt, spl in ((64, 2), (64, 4), (128, 4), (256, 2), (256, 4)):
        if N <= nt * spl and C <= nt:
            return (False, nt, spl, 1)
    return None


def shape_of(form, N, keep, lds=lds_bytes):
    """(two, nt, spl, nwx) of the kernels a batch of length N runs in, None where the library refuses the batch (no candidate, or over 160 KB of LDS)."""
    C = problem_C(form, N, keep)
    s = pick_shape(form, N, C, keep)
    if s is None:
        return None
    if s[0] and lds(form, N, keep) > LDS_LIMIT:
        s = pick_shape(form, N, C, 0)  # resolve_shape: keep 0 forces the single-level candidates (K re-enters its own two-level mapping)
        if s is None:
            return None
    if lds(form, N, keep) > LDS_LIMIT:  # po_solve.cpp validate(): PO_ERR_UNSUPPORTED
        return None
    return s


def has_polish_kernel(shape):
    return shape is not None and shape[0] and shape[3] not in (2, 3)


def first_wave_stages(shape, keep):
    """Stages the first 64 lanes of a block own (role-split: two lanes per chunk)."""
    _, _, spl, nwx = shape
    return 32 * keep if nwx in (2, 3) else 64 * spl


def reachable(lds=lds_bytes):
    """{(form, shape): {keep: [N, ...]}} over KEEPS x N_GRID."""
    out = {}
    for form, keeps in KEEPS.items():
        for keep in keeps:
            for N in N_GRID:
                s = shape_of(form, N, keep, lds)
                if s is not None:
                    out.setdefault((form, s), {}).setdefault(keep, []).append(N)
    return out


def largest_accepted(form, keep, lds=lds_bytes):
    return max(N for N in N_GRID if shape_of(form, N, keep, lds) is not None)


def boundary_lengths(form, keep, shape, lds=lds_bytes):
    """The lengths a MATRIX row runs: the shape's smallest N (at least 3; keep + 2 for KP), its largest, one below the largest that is a multiple of neither
    4 nor keep, and on multi-wave blocks the first N that needs the second wave (first_wave_stages + 1, or the smallest N if that is larger; on 256-thread blocks also the third and fourth)."""
    ns = [N for N in N_GRID if shape_of(form, N, keep, lds) == shape]
    lo, hi = max(ns[0], keep + 2 if form == KP else 3), ns[-1]
    out = {lo, hi}
    m = hi - 1
    while m > lo and (m % 4 == 0 or (keep > 1 and m % keep == 0)):
        m -= 1
    if m >= lo:
        out.add(m)
    for w in range(1, shape[1] // 64):  # (256-thread blocks: the first N of each further wave that falls in the range)
        out.add(max(lo, min(hi, w * first_wave_stages(shape, keep) + 1)))
    return tuple(sorted(out))


# one row per reachable (formulation, shape): (form, keep, shape, boundary lengths).  Two-level rows first, then the single-level mapping as (form, NT, SPL) with one keep
# that reaches it.  tests/test_shape_table.py checks that every reachable shape has a row and that the lengths are those boundary_lengths derives.
MATRIX = [
    # KP, multi-group (keep 1 / 2)
    (KP, 1, (True, 64, 4, 4), (3, 255, 256)),
    (KP, 1, (True, 128, 4, 4), (257, 511, 512)),
    (KP, 2, (True, 64, 4, 5), (4, 255, 256)),
    (KP, 2, (True, 128, 4, 5), (257, 511, 512)),
    # KP, one lane per chunk (keep 3 .. 5)
    (KP, 3, (True, 64, 3, 1), (5, 191, 192)),
    (KP, 3, (True, 128, 3, 1), (193, 383, 384)),
    (KP, 4, (True, 64, 4, 1), (6, 255, 256)),
    (KP, 4, (True, 128, 4, 1), (257, 511, 512)),
    (KP, 5, (True, 64, 5, 1), (7, 319, 320)),
    # KP, role-split (keep 6 .. 8: one or two waves; 9 .. 16: one wave)
    (KP, 6, (True, 64, 3, 2), (8, 191, 192)),
    (KP, 6, (True, 128, 3, 2), (193, 383, 384)),
    (KP, 7, (True, 64, 4, 3), (9, 223, 224)),
    (KP, 7, (True, 128, 4, 3), (225, 447, 448)),
    (KP, 8, (True, 64, 4, 2), (10, 255, 256)),
    (KP, 8, (True, 128, 4, 2), (257, 511, 512)),
    (KP, 9, (True, 64, 5, 3), (11, 287, 288)),
    (KP, 10, (True, 64, 5, 2), (12, 319, 320)),
    (KP, 11, (True, 64, 6, 3), (13, 351, 352)),
    (KP, 12, (True, 64, 6, 2), (14, 383, 384)),
    (KP, 13, (True, 64, 7, 3), (15, 415, 416)),
    (KP, 14, (True, 64, 7, 2), (16, 447, 448)),
    (KP, 15, (True, 64, 8, 3), (17, 479, 480)),
    (KP, 16, (True, 64, 8, 2), (18, 511, 512)),
    # KPC (keep 4) and K
    (KPC, 4, (True, 64, 4, 1), (3, 255, 256)),
    (KPC, 4, (True, 128, 4, 1), (257, 511, 512)),
    (K, 1, (True, 64, 2, 1), (3, 127, 128)),
    (K, 1, (True, 64, 4, 1), (129, 255, 256)),
    (K, 1, (True, 128, 4, 1), (257, 511, 512)),
    # the single-level mapping
    (KP, 17, (False, 64, 2, 1), (19, 127, 128)),
    (KP, 17, (False, 64, 4, 1), (129, 254, 256)),
    (KP, 5, (False, 128, 4, 1), (321, 511, 512)),
    (KP, 3, (False, 256, 2, 1), (386, 511, 512)),
    (KP, 4, (False, 256, 4, 1), (513, 769, 874, 875)),
    (KPC, 4, (False, 256, 4, 1), (513, 769, 874, 875)),
    (K, 1, (False, 256, 4, 1), (513, 753, 754)),
]

# the largest length the library accepts, per (form, keep): the LDS of the shape (keep >= 3, KPC, K) or C <= NT (keep 1 / 2) sets it
N_MAX = {(KP, 1): 512, (KP, 2): 513, (KP, 3): 769, (KP, 4): 875, (KP, 5): 885, (KP, 6): 891, (KP, 7): 896, (KP, 8): 899, (KP, 12): 908, (KP, 16): 912,
         (KP, 17): 913, (KPC, 4): 875, (K, 1): 754}


def row_id(row):
    form, keep, (two, nt, spl, nwx), _ = row
    return f"{FORM_NAMES[form]}-keep{keep}-{'two' if two else 'single'}-{nt}x{spl}" + (f"-nwx{nwx}" if two else "")
