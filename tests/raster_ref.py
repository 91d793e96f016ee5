"""The definition of po_rasterize_batch (include/po_hip.h) in numpy: per-layer obstacle lists -> occupancy images.

Every arithmetic step is ONE numpy ufunc on float64 arrays (np.add / np.subtract / np.multiply, then a comparison), so each operation is rounded once and nothing can
be fused — the device kernel is compiled without contraction and must agree bit for bit.  There is no culling here: every obstacle of a layer is tested against every
cell of the layer.

Arrays are indexed [i, j] = [x index, y index] like every map of the binding; obstacles are records of binding.OBSTACLE_DTYPE."""
import numpy as np

PO_OBS_DISC, PO_OBS_POLY, PO_OBS_MAX_VERTS = 0, 1, 8


def cell_centres(size, res, pos):
    """Centres of cells 0 .. size-1 along one axis: getPositionFromIndex, p = (pos + (0.5 * (size * res) - 0.5 * res)) + res * (-idx)."""
    res, pos = np.float64(res), np.float64(pos)
    origin = np.add(pos, np.subtract(np.multiply(np.float64(0.5), np.multiply(np.float64(size), res)), np.multiply(np.float64(0.5), res)))
    return np.add(origin, np.multiply(res, (-np.arange(size)).astype(np.float64)))


def covers(o, X, Y):
    """bool [sx, sy]: the cells whose centre (X [sx, 1], Y [1, sy]) obstacle record `o` covers."""
    none = np.zeros((X.shape[0], Y.shape[1]), dtype=bool)
    v = np.asarray(o["v"], dtype=np.float64)
    kind = int(o["kind"])
    if kind == PO_OBS_DISC:
        if np.isnan(v[:3]).any():
            return none
        dx, dy = np.subtract(X, v[0]), np.subtract(Y, v[1])
        return np.less_equal(np.add(np.multiply(dx, dx), np.multiply(dy, dy)), np.multiply(v[2], v[2]))
    if kind == PO_OBS_POLY:
        n = min(max(int(o["n_verts"]), 0), PO_OBS_MAX_VERTS)  # the device entries read n_verts clamped
        if n < 3 or np.isnan(v[:2 * n]).any():
            return none
        vx, vy = v[0:2 * n:2], v[1:2 * n:2]
        inside = (X >= vx.min()) & (X <= vx.max()) & (Y >= vy.min()) & (Y <= vy.max())  # the closed bounding box: exact min / max
        pos, neg = inside.copy(), inside.copy()
        for e in range(n):
            ax, ay, bx, by = vx[e], vy[e], vx[(e + 1) % n], vy[(e + 1) % n]
            ex, ey = np.subtract(bx, ax), np.subtract(by, ay)
            cr = np.subtract(np.multiply(ex, np.subtract(Y, ay)), np.multiply(ey, np.subtract(X, ax)))
            pos &= np.greater_equal(cr, 0.0)
            neg &= np.less_equal(cr, 0.0)
        return pos | neg
    return none  # unknown kind


def covered(obs, first, size_x, size_y, res, pos_xy):
    """bool [M, size_x, size_y]: cells covered by an obstacle of their layer.  first[] is read clamped into [0, n_obs] like the device entries do (a valid list is
    not changed by that); pos_xy [M, 2]."""
    M = len(first) - 1
    out = np.zeros((M, size_x, size_y), dtype=bool)
    with np.errstate(all="ignore"):  # (infinite coordinates: the predicate is evaluated all the same)
        for k in range(M):
            X = cell_centres(size_x, res, pos_xy[k][0])[:, None]
            Y = cell_centres(size_y, res, pos_xy[k][1])[None, :]
            lo, hi = (min(max(int(first[k + d]), 0), len(obs)) for d in (0, 1))
            for o in obs[lo:hi]:
                out[k] |= covers(o, X, Y)
    return out


def to_cells(cov, base=None):
    """uint8 [M, size_x, size_y], 0 = occupied / 255 = free, from covered() and an optional base ([size_x, size_y] shared, or one per layer; 0 = occupied)."""
    occ = cov if base is None else cov | (np.asarray(base) == 0)
    return np.where(occ, 0, 255).astype(np.uint8)


def rasterize(obs, first, size_x, size_y, res, pos_xy=None, pos=(0.0, 0.0), base=None):
    M = len(first) - 1
    pos_xy = np.tile(np.asarray(pos, dtype=np.float64), (M, 1)) if pos_xy is None else np.asarray(pos_xy, dtype=np.float64)
    return to_cells(covered(obs, first, size_x, size_y, res, pos_xy), base)
