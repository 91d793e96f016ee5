"""Dev tool (CPU): the library's host-side shape queries as data.  `PO_LIB=<libpo_hip.so> python tools/shape_query_dump.py grid|golden <out.json>` writes, per
(formulation, keep, N): C, po_shape_threads, po_lds_bytes, po_polish_state_doubles, po_newton_park_doubles, po_has_polish_kernel, po_has_fixed_length.
    grid    every formulation, every keep of tests/shape_table.py's KEEPS, N = 2 .. 1100: two libraries answer alike iff the two files are equal (cmp)
    golden  every MATRIX row at its boundary lengths and (KP, keep 4, N = 200): tests/golden/shape_queries.json, which tests/test_shape_table.py pins
The state and park doubles size device buffers: a value that shrinks is an out-of-bounds write on the GPU."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
QUERIES = ("po_shape_threads", "po_lds_bytes", "po_polish_state_doubles", "po_newton_park_doubles", "po_has_polish_kernel", "po_has_fixed_length")


def golden_points():
    import shape_table as S

    pts = [(form, keep, N) for form, keep, _, lengths in S.MATRIX for N in lengths] + [(S.KP, 4, 200)]
    return sorted(set(pts))


def grid_points():
    import shape_table as S

    return [(form, keep, N) for form, keeps in S.KEEPS.items() for keep in keeps for N in S.N_GRID]


def query(lib, points):
    """[[form, keep, N, C, threads, lds bytes, state doubles, park doubles, has polish, has fixed length], ...]"""
    import shape_table as S

    for name in QUERIES:
        getattr(lib, name).restype = ctypes.c_size_t if name == "po_lds_bytes" else ctypes.c_int
        getattr(lib, name).argtypes = [ctypes.c_int] * 4
    return [[form, keep, N, S.problem_C(form, N, keep)] + [int(getattr(lib, q)(form, N, S.problem_C(form, N, keep), keep)) for q in QUERIES] for form, keep, N in points]


if __name__ == "__main__":
    from path_optimizer_amd import binding

    mode, out = sys.argv[1], sys.argv[2]
    rows = query(binding.lib(), {"grid": grid_points, "golden": golden_points}[mode]())
    with open(out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{binding.LIB_PATH}: {len(rows)} rows -> {out}")
