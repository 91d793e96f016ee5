"""The definition of po_rasterize_scene_batch (include/po_hip.h) in numpy: obstacle lists, a world grid and polygon rings -> occupancy images.

Every arithmetic step is ONE numpy ufunc on float64 arrays, so each operation is rounded once and nothing can be fused.  There is no culling here: every edge of every
ring a layer owns is tested against every cell of the layer.  The base / DISC / POLY clauses are raster_ref's.

Arrays are indexed [i, j] = [x index, y index] like every map of the binding.  Ring tables are read the way the device entries read them: start[] clamped into
[0, n_verts], n_shared and first[] into [0, n_rings], rings with fewer than 3 vertices or an unknown flag ignored, longer ones cut to PO_RING_MAX_VERTS — a valid table
is not changed by that."""
import numpy as np

import raster_ref

PO_RING_SOLID, PO_RING_FREE, PO_RING_MAX_VERTS = 0, 1, 4096


def contains(xy, X, Y):
    """bool [sx, sy]: the cells whose centre (X [sx, 1], Y [1, sy]) the ring xy [n, 2] contains — even-odd over the edges a -> b, the last one closing."""
    n = len(xy)
    par = np.zeros((X.shape[0], Y.shape[1]), dtype=bool)
    with np.errstate(all="ignore"):
        for e in range(n):
            ax, ay = xy[e]
            bx, by = xy[(e + 1) % n]
            straddles = np.not_equal(np.greater(ay, Y), np.greater(by, Y))
            t = np.subtract(np.multiply(np.subtract(bx, ax), np.subtract(Y, ay)), np.multiply(np.subtract(by, ay), np.subtract(X, ax)))
            right = np.greater(t, 0.0) if by > ay else np.less(t, 0.0)
            par ^= straddles & right
    return par


def _clamp(v, hi):
    return min(max(int(v), 0), hi)


def layer_rings(rings, k):
    """The (xy, flag) pairs layer k owns, read clamped.  rings = (verts, start, flags, n_shared, first or None) as binding.pack_rings returns them."""
    verts, start, flags, n_shared, first = rings
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 2)
    nr, nv = len(flags), len(verts)
    own = list(range(_clamp(n_shared, nr)))
    if first is not None:
        own += list(range(_clamp(first[k], nr), _clamp(first[k + 1], nr)))
    out = []
    for r in own:
        s0, s1 = _clamp(start[r], nv), _clamp(start[r + 1], nv)
        n = min(s1 - s0, PO_RING_MAX_VERTS)
        if n >= 3 and int(flags[r]) in (PO_RING_SOLID, PO_RING_FREE):
            out.append((verts[s0:s0 + n], int(flags[r])))
    return out


def ring_occupied(rings, M, size_x, size_y, res, pos_xy):
    """bool [M, size_x, size_y]: the SOLID and FREE clauses."""
    out = np.zeros((M, size_x, size_y), dtype=bool)
    for k in range(M):
        X = raster_ref.cell_centres(size_x, res, pos_xy[k][0])[:, None]
        Y = raster_ref.cell_centres(size_y, res, pos_xy[k][1])[None, :]
        in_free, has_free = np.zeros((size_x, size_y), dtype=bool), False
        for xy, flag in layer_rings(rings, k):
            c = contains(xy, X, Y)
            if flag == PO_RING_SOLID:
                out[k] |= c
            else:
                has_free = True
                in_free |= c
        if has_free:
            out[k] |= ~in_free
    return out


def world_index(p, wpos, wsize, wres):
    """isInside + getIndexFromPosition along one axis: the world index under each coordinate of p, -1 outside."""
    wres, wpos = np.float64(wres), np.float64(wpos)
    ln = np.multiply(np.float64(wsize), wres)
    half = np.multiply(np.float64(0.5), ln)
    with np.errstate(all="ignore"):
        t = np.negative(np.subtract(np.subtract(p, wpos), half))
        inside = np.greater_equal(t, 0.0) & np.less(t, ln)
        q = np.negative(np.divide(np.subtract(np.subtract(p, half), wpos), wres))
        idx = np.where(inside, np.trunc(np.where(inside, q, 0.0)), -1).astype(np.int64)
    return np.where(inside & (idx >= 0) & (idx < wsize), idx, -1)


def world_occupied(world, wres, wpos, outside_occupied, M, size_x, size_y, res, pos_xy):
    """bool [M, size_x, size_y]: the world clause.  world [wsx, wsy], 0 = occupied."""
    world = np.asarray(world)
    out = np.zeros((M, size_x, size_y), dtype=bool)
    for k in range(M):
        ix = world_index(raster_ref.cell_centres(size_x, res, pos_xy[k][0]), wpos[0], world.shape[0], wres)[:, None]
        iy = world_index(raster_ref.cell_centres(size_y, res, pos_xy[k][1]), wpos[1], world.shape[1], wres)[None, :]
        ok = (ix >= 0) & (iy >= 0)
        out[k] = np.where(ok, world[np.maximum(ix, 0), np.maximum(iy, 0)] == 0, bool(outside_occupied))
    return out


def rasterize(obs, first, rings, size_x, size_y, res, pos_xy=None, pos=(0.0, 0.0), base=None, world=None):
    """uint8 [M, size_x, size_y], 0 = occupied / 255 = free.  rings: None or binding.pack_rings' tuple; world: None or (image [wsx, wsy], wres, (wpx, wpy),
    outside_occupied)."""
    M = len(first) - 1
    pos_xy = np.tile(np.asarray(pos, dtype=np.float64), (M, 1)) if pos_xy is None else np.asarray(pos_xy, dtype=np.float64)
    occ = raster_ref.covered(obs, first, size_x, size_y, res, pos_xy)
    if rings is not None:
        occ |= ring_occupied(rings, M, size_x, size_y, res, pos_xy)
    if world is not None:
        occ |= world_occupied(world[0], world[1], world[2], world[3], M, size_x, size_y, res, pos_xy)
    return raster_ref.to_cells(occ, base)
