"""CPU reference of the obstacle-distance layer (tests only; pure numpy, exact): the definition of include/po_hip.h

    d2(i, j)   = min over occupied cells (p, q) of (i - p)^2 + (j - q)^2          exact integer (int64 here)
    dist(i, j) = float32(sqrt(double(d2(i, j)))) * float32(resolution)             one float32 multiply
    no occupied cell: d2 = size_x^2 + size_y^2 everywhere (the library's own rule)

occ is indexed [size_x, size_y] (0 = occupied, anything else free), like Engine.set_map's `dist`; the transform is symmetric in the two axes.

Three routes to d2, all exact, cross-checked against each other and against scipy in tests/test_distance_map.py:
  separable, broadcast   per line of axis 1 the distance g to the nearest occupied cell of the line, then per line of axis 0  min_q (i - q)^2 + g(q)^2  by broadcasting
                         in int64, in row blocks (memory); cost size_x^2 * size_y — the plain statement, used up to BROADCAST_LIMIT
  separable, shifted     the same minimum taken offset by offset, q = i -+ d for d = 1, 2, ...: an offset with d^2 >= the largest value still standing cannot improve any
                         cell, so the loop ends there; cost (largest distance) * cells — what large dense images need
  brute force            the definition itself, one pass per occupied cell; for images with a handful of occupied cells (4096 x 4096 in the GPU test)"""
import numpy as np

FAR = np.int64(1) << 40          # "no occupied cell on this line": far above any real 2 * 4095^2, far below int64 overflow when squares are added
BROADCAST_LIMIT = 3 * 10 ** 8    # size_x^2 * size_y up to which d2() takes the broadcast route


def line_distance(occ):
    """g[i, j] = min |j - z| over the occupied z of line i (FAR where the line has none)."""
    occ = np.asarray(occ)
    sx, sy = occ.shape
    j = np.arange(sy, dtype=np.int64)[None, :]
    hit = occ == 0
    last = np.maximum.accumulate(np.where(hit, j, -FAR), axis=1)                       # nearest occupied index <= j
    nxt = np.minimum.accumulate(np.where(hit, j, FAR)[:, ::-1], axis=1)[:, ::-1]       # nearest occupied index >= j
    return np.minimum(np.where(last < 0, FAR, j - last), np.where(nxt >= FAR, FAR, nxt - j))


def _second_pass_broadcast(g2):
    sx, sy = g2.shape
    q = np.arange(sx, dtype=np.int64)
    out = np.empty_like(g2)
    block = max(1, int(2 * 10 ** 7 // max(1, sx * sy)))
    for i0 in range(0, sx, block):
        i = np.arange(i0, min(sx, i0 + block), dtype=np.int64)
        off2 = (i[:, None] - q[None, :]) ** 2                                          # [block, q]
        out[i0:i0 + len(i)] = (off2[:, :, None] + g2[None, :, :]).min(axis=1)
    return out


def _second_pass_shifted(g2):
    sx = g2.shape[0]
    best = g2.copy()
    for d in range(1, sx):
        dd = np.int64(d) * d
        if dd >= best.max():
            break
        np.minimum(best[d:], g2[:-d] + dd, out=best[d:])
        np.minimum(best[:-d], g2[d:] + dd, out=best[:-d])
    return best


def d2(occ, route=None):
    """Exact squared distance in cells, int64 [size_x, size_y]; route: None (by size), "broadcast" or "shifted"."""
    occ = np.asarray(occ)
    sx, sy = occ.shape
    if not (occ == 0).any():
        return np.full((sx, sy), sx * sx + sy * sy, dtype=np.int64)
    g = line_distance(occ)
    g2 = np.where(g >= FAR, FAR, g * g)
    if route is None:
        route = "broadcast" if sx * sx * sy <= BROADCAST_LIMIT else "shifted"
    return _second_pass_broadcast(g2) if route == "broadcast" else _second_pass_shifted(g2)


def d2_brute(occ):
    """The definition, one pass per occupied cell (images with few of them)."""
    occ = np.asarray(occ)
    sx, sy = occ.shape
    ps, qs = np.nonzero(occ == 0)
    if len(ps) == 0:
        return np.full((sx, sy), sx * sx + sy * sy, dtype=np.int64)
    i = np.arange(sx, dtype=np.int64)[:, None]
    j = np.arange(sy, dtype=np.int64)[None, :]
    best = None
    for p, q in zip(ps.tolist(), qs.tolist()):
        c = (i - p) ** 2 + (j - q) ** 2
        best = c if best is None else np.minimum(best, c, out=best)
    return best


def to_metres(d2_cells, resolution):
    """The two float32 steps of the definition."""
    return np.sqrt(d2_cells.astype(np.float64)).astype(np.float32) * np.float32(resolution)


def distance_map(occ, resolution, route=None):
    return to_metres(d2(occ, route), resolution)


def random_occupancy(rng, sx, sy, kind):
    """uint8 [sx, sy], 0 = occupied.  kind: "single" (one occupied cell), "corner" (cell (0, 0) only), "all", "none", or a density in (0, 1]."""
    if kind == "all":
        return np.zeros((sx, sy), dtype=np.uint8)
    occ = np.full((sx, sy), 255, dtype=np.uint8)
    if kind == "none":
        return occ
    if kind == "corner":
        occ[0, 0] = 0
    elif kind == "single":
        occ[rng.integers(sx), rng.integers(sy)] = 0
    else:
        occ[rng.random((sx, sy)) < float(kind)] = 0
        occ[occ != 0] = rng.integers(1, 256, size=int((occ != 0).sum()), dtype=np.uint8)   # "anything else is free"
    return occ
