"""ctypes binding over the C ABI of libpo_hip.so (include/po_hip.h).

Plumbing only: the product is the shared library.  There is NO CPU fallback — importing works without a
GPU (so the symbol/ABI tests can run), but every compute call goes to the HIP kernels and raises
PoError if the library or a device is missing.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from .abi import (INFO_BYTES, INFO_DTYPE, PO_ABI_VERSION, PO_ERR_HIP, PO_ERR_UNSUPPORTED, PO_OK, PoBatchIn, PoBatchOut, PoParams)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PO_LIB") or os.path.join(_HERE, "libpo_hip.so")  # PO_LIB: dev builds (make dev), A/B experiments
_LIB = None

EXPORTS = ["po_default_params", "po_problem_dims", "po_keep_control_steps", "po_create", "po_destroy", "po_set_stream", "po_debug_set", "po_device_count",
           "po_solve_batch", "po_solve_batch_device", "po_assemble_batch", "po_scaling_batch", "po_last_kernel_ms", "po_last_phase_ms", "po_debug_get", "po_strerror",
           "po_last_hip_error", "po_version", "po_set_map", "po_postcheck_batch", "po_postcheck_batch_device", "po_bounds_batch",
           "po_bounds_batch_device", "po_map_sample", "po_smooth_dims", "po_smooth_batch", "po_smooth_batch_device",
           "po_resample_batch", "po_resample_batch_device", "po_limits_batch", "po_limits_batch_device", "po_dp_search_batch",
           "po_dp_search_batch_device", "po_bspline_batch_device", "po_segment_raw_batch_device", "po_post_project_batch_device",
           "po_segment_init_batch_device", "po_plan_batch", "po_plan_batch_device", "po_densify_batch", "po_densify_batch_device",
           "po_distance_map_batch", "po_distance_map_batch_device", "po_set_map_occupancy", "po_set_map_occupancy_device", "po_get_map",
           "po_set_map_stack", "po_set_map_stack_occupancy", "po_set_map_stack_occupancy_device", "po_set_map_assignment", "po_set_map_assignment_device",
           "po_get_map_layer", "po_map_sample_layer",
           "po_rasterize_batch", "po_rasterize_batch_device", "po_set_map_stack_obstacles", "po_set_map_stack_obstacles_device",
           "po_set_world_occupancy", "po_set_world_occupancy_device", "po_rasterize_scene_batch", "po_rasterize_scene_batch_device",
           "po_set_map_stack_scene", "po_set_map_stack_scene_device",
           "po_default_select_params", "po_select_batch", "po_select_batch_device",
           "po_default_speed_params", "po_speed_batch", "po_speed_batch_device",
           "po_default_dynamic_params", "po_dynamic_batch", "po_dynamic_batch_device",
           "po_default_stplan_params", "po_stplan_batch", "po_stplan_batch_device",
           "po_default_nudge_params", "po_nudge_batch", "po_nudge_batch_device",
           "po_default_trajectory_params", "po_trajectory_batch", "po_trajectory_batch_device",
           "po_default_agentsets_params", "po_agentsets_batch", "po_agentsets_batch_device",
           "po_default_stgo_params", "po_stgo_batch", "po_stgo_batch_device",
           "po_default_speedqp_params", "po_speedqp_batch", "po_speedqp_batch_device"]


class PoError(RuntimeError):
    pass


_ENV_DEBUG = {"PO_IDENTITY_ORDER": "identity_order", "PO_DEBUG_CYCLES": "debug_cycles", "PO_SMOOTH_SEQ": "smooth_seq",
              "PO_SMOOTH_WAVES": "smooth_waves", "PO_SMOOTH_NOPAD": "smooth_nopad", "PO_SMOOTH_DEBUG": "smooth_debug", "PO_DP_ONE_WAVE": "dp_one_wave", "PO_NEWTON_SLICE": "newton_slice",
              "PO_FIXED_LENGTH": "fixed_length", "PO_FIXED_CLASSES": "fixed_classes"}


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise PoError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        try:  # if torch lives in this process too, let it load ITS libamdhip64 first so that both share one HIP runtime
            import torch  # noqa: F401
        except Exception:  # torch is optional plumbing (allocator / streams), never required by the library
            pass
        L = C.CDLL(LIB_PATH)
        L.po_strerror.restype = C.c_char_p
        L.po_last_hip_error.restype = C.c_char_p
        L.po_version.restype = C.c_char_p
        # the structs of abi.py are laid out for ONE ABI: a stale libpo_hip.so (or an older dev build picked through PO_LIB) would be driven with shifted fields
        ver = L.po_version().decode()
        parts = ver.split()
        if len(parts) < 2 or not parts[1].isdigit() or int(parts[1]) != PO_ABI_VERSION:
            raise PoError(f"{LIB_PATH} reports '{ver}' but this binding is written against PO_ABI_VERSION {PO_ABI_VERSION} (include/po_hip.h): rebuild the library")
        L.po_create.argtypes = [C.c_int, C.POINTER(PoParams), C.POINTER(C.c_void_p)]
        L.po_destroy.argtypes = [C.c_void_p]
        L.po_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.po_solve_batch.argtypes = [C.c_void_p, C.POINTER(PoBatchIn), C.POINTER(PoBatchOut)]
        L.po_solve_batch_device.argtypes = [C.c_void_p, C.POINTER(PoBatchIn), C.POINTER(PoBatchOut)]
        L.po_assemble_batch.argtypes = [C.c_void_p, C.POINTER(PoBatchIn), C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_scaling_batch.argtypes = [C.c_void_p, C.POINTER(PoBatchIn), C.c_void_p]
        L.po_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.po_last_phase_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.po_debug_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_longlong)]
        L.po_distance_map_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.po_distance_map_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.po_set_map_occupancy.argtypes = [C.c_void_p, C.c_void_p]
        L.po_set_map_occupancy_device.argtypes = [C.c_void_p, C.c_void_p]
        L.po_get_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_set_map_stack.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.po_set_map_stack_occupancy.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.po_set_map_stack_occupancy_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.po_set_map_assignment.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.po_set_map_assignment_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.po_get_map_layer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.po_map_sample_layer.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_rasterize_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_rasterize_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_set_map_stack_obstacles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.po_set_map_stack_obstacles_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.po_set_world_occupancy.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.po_set_world_occupancy_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.po_rasterize_scene_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_rasterize_scene_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_set_map_stack_scene.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.po_set_map_stack_scene_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.po_default_select_params.argtypes = [C.c_void_p]
        L.po_default_select_params.restype = None
        L.po_select_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_select_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_default_speed_params.argtypes = [C.c_void_p]
        L.po_default_speed_params.restype = None
        L.po_speed_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_speed_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_default_dynamic_params.argtypes = [C.c_void_p]
        L.po_default_dynamic_params.restype = None
        L.po_dynamic_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_dynamic_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_default_stplan_params.argtypes = [C.c_void_p]
        L.po_default_stplan_params.restype = None
        L.po_stplan_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_stplan_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_default_nudge_params.argtypes = [C.c_void_p]
        L.po_default_nudge_params.restype = None
        L.po_nudge_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_nudge_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_default_trajectory_params.argtypes = [C.c_void_p]
        L.po_default_trajectory_params.restype = None
        L.po_trajectory_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_trajectory_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_default_agentsets_params.argtypes = [C.c_void_p]
        L.po_default_agentsets_params.restype = None
        L.po_agentsets_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_agentsets_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_default_stgo_params.argtypes = [C.c_void_p]
        L.po_default_stgo_params.restype = None
        L.po_stgo_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_stgo_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_default_speedqp_params.argtypes = [C.c_void_p]
        L.po_default_speedqp_params.restype = None
        L.po_speedqp_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_speedqp_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


def _check(rc: int):
    if rc != PO_OK:
        L = lib()
        msg = L.po_strerror(rc).decode()
        if rc == PO_ERR_HIP:
            msg += ": " + L.po_last_hip_error().decode()
        raise PoError(f"libpo_hip: {msg} (rc={rc})")


def default_params() -> PoParams:
    p = PoParams()
    lib().po_default_params(C.byref(p))
    return p


def default_select_params():
    """po_default_select_params: the cost weights and thresholds of po_select_batch* (a starting point nobody has tuned)."""
    from .abi import PoSelectParams

    p = PoSelectParams()
    lib().po_default_select_params(C.byref(p))
    return p


def default_speed_params():
    """po_default_speed_params: the caps of po_speed_batch* (a starting point nobody has tuned)."""
    from .abi import PoSpeedParams

    p = PoSpeedParams()
    lib().po_default_speed_params(C.byref(p))
    return p


def default_dynamic_params():
    """po_default_dynamic_params: margin and stop distance of po_dynamic_batch* (a starting point nobody has tuned)."""
    from .abi import PoDynamicParams

    p = PoDynamicParams()
    lib().po_default_dynamic_params(C.byref(p))
    return p


def default_stplan_params():
    """po_default_stplan_params: the knobs of po_stplan_batch* (a starting point nobody has tuned)."""
    from .abi import PoStplanParams

    p = PoStplanParams()
    lib().po_default_stplan_params(C.byref(p))
    return p


def default_stgo_params():
    """po_default_stgo_params: the knobs of po_stgo_batch*, po_stplan_batch*'s and the sample times (a starting point nobody has tuned)."""
    from .abi import PoStgoParams

    p = PoStgoParams()
    lib().po_default_stgo_params(C.byref(p))
    return p


def default_speedqp_params():
    """po_default_speedqp_params: the knobs of po_speedqp_batch*, po_stgo_batch*'s grids, the limits, the weights and the ADMM settings (a starting point nobody
    has tuned)."""
    from .abi import PoSpeedqpParams

    p = PoSpeedqpParams()
    lib().po_default_speedqp_params(C.byref(p))
    return p


def default_nudge_params():
    """po_default_nudge_params: the knobs of po_nudge_batch* (a starting point nobody has tuned)."""
    from .abi import PoNudgeParams

    p = PoNudgeParams()
    lib().po_default_nudge_params(C.byref(p))
    return p


def default_trajectory_params():
    """po_default_trajectory_params: horizon, agent discs and agent points of po_trajectory_batch* (a starting point nobody has tuned)."""
    from .abi import PoTrajectoryParams

    p = PoTrajectoryParams()
    lib().po_default_trajectory_params(C.byref(p))
    return p


def covering_discs(params):
    """(offsets [4], radius) of the four covering circles of a parameter struct (PoParams or the oracle's: the same fields): the offsets po_params.d[j] along the
    heading and the radius po_bounds_batch* and po_nudge_batch* derive, sqrt((car_length / 8)^2 + (car_width / 2)^2) + safety_margin, in that order of
    operations.  What po_trajectory_params.disc_offset / disc_radius take to emit a vehicle as the corridor stages see it."""
    rad = np.sqrt(np.float64(params.car_length / 8) * np.float64(params.car_length / 8) + np.float64(params.car_width / 2) * np.float64(params.car_width / 2))
    return [float(params.d[j]) for j in range(4)], float(rad + np.float64(params.safety_margin))


def default_agentsets_params():
    """po_default_agentsets_params: reach, time windows and owner rule of po_agentsets_batch* (a starting point nobody has tuned)."""
    from .abi import PoAgentsetsParams

    p = PoAgentsetsParams()
    lib().po_default_agentsets_params(C.byref(p))
    return p


def footprint_reach(params, margin):
    """The reach (po_agentsets_params.reach) with which po_dynamic_batch* at this margin cannot miss an agent: no footprint circle's edge is farther from the path
    point than max_q (hypot(cx_q, cy_q) + cr_q) over the six circles of a parameter struct (PoParams or the oracle's; car_geometry.cpp:38-56 as po_capi.cpp's
    make_car writes it), plus the margin, plus 1e-6 of slack for the roundings of the rotated centres."""
    width, back, front = params.car_width, params.car_length / 2.0 - params.rear_axle_to_center, params.car_length / 2.0 + params.rear_axle_to_center
    length, bx, shift = front + back, (front - back) / 2.0, width / 4.0
    small_r = float(np.sqrt(2 * (shift * shift)))
    large_r = float(np.sqrt(width * width + ((length - width) / 2.0) * ((length - width) / 2.0))) / 2
    cx = [-back + shift, -back + shift, front - shift, front - shift, bx + (length - width) / 4, bx - (length - width) / 4]
    cy = [-width / 2.0 + shift, width / 2.0 - shift, -width / 2.0 + shift, width / 2.0 - shift, 0.0, 0.0]
    cr = [small_r] * 4 + [large_r] * 2
    return max(float(np.hypot(cx[q], cy[q])) + cr[q] for q in range(6)) + float(margin) + 1e-6


def problem_dims(form: int, N: int, keep: int):
    n, m, c = C.c_int(), C.c_int(), C.c_int()
    _check(lib().po_problem_dims(form, N, keep, C.byref(n), C.byref(m), C.byref(c)))
    return n.value, m.value, c.value


def smooth_dims(kind: int, P: int):
    n, m = C.c_int(), C.c_int()
    _check(lib().po_smooth_dims(kind, P, C.byref(n), C.byref(m)))
    return n.value, m.value


def keep_control_steps(form: int, ref_s) -> int:
    ref_s = np.ascontiguousarray(ref_s, dtype=np.float64)
    k = lib().po_keep_control_steps(form, ref_s.ctypes.data_as(C.c_void_p), len(ref_s))
    if k < 0:
        _check(k)
    return k


def _np(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- obstacle lists (po_obstacle) ----
OBSTACLE_DTYPE = np.dtype([("kind", np.int32), ("n_verts", np.int32), ("v", np.float64, (16,))])  # po_obstacle, 136 bytes


def obstacle_disc(x, y, r):
    """A disc of radius r >= 0 centred at (x, y), world frame: one record of OBSTACLE_DTYPE."""
    from .abi import PO_OBS_DISC

    o = np.zeros((), dtype=OBSTACLE_DTYPE)
    o["kind"] = PO_OBS_DISC
    o["v"][:3] = (x, y, r)
    return o


def obstacle_polygon(xy):
    """A convex polygon with 3 .. 8 vertices xy [n, 2] (world frame, either orientation)."""
    from .abi import PO_OBS_MAX_VERTS, PO_OBS_POLY

    xy = np.asarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2 or not 3 <= len(xy) <= PO_OBS_MAX_VERTS:
        raise ValueError("a polygon has 3 .. 8 vertices (x, y)")
    o = np.zeros((), dtype=OBSTACLE_DTYPE)
    o["kind"] = PO_OBS_POLY
    o["n_verts"] = len(xy)
    o["v"][:2 * len(xy)] = xy.reshape(-1)
    return o


def obstacle_box(cx, cy, half_length, half_width, yaw):
    """An oriented box as a 4-vertex polygon.  The corners are computed HERE, on the host: the device sees polygons only, so no trigonometry enters the
    bit-exact path (two hosts whose cos / sin differ in the last bit hand over different polygons, each rasterised exactly)."""
    c, s = np.cos(yaw), np.sin(yaw)
    corners = [(cx + sl * half_length * c - sw * half_width * s, cy + sl * half_length * s + sw * half_width * c) for sl, sw in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
    return obstacle_polygon(corners)


def pack_obstacles(layers):
    """M lists of obstacle records -> (obs [n_obs] of OBSTACLE_DTYPE, first [M + 1] int32): layer k owns obs[first[k]:first[k + 1]].  A tuple (obs, first) that is
    packed already passes through (converted, not checked: the library checks)."""
    if isinstance(layers, tuple) and len(layers) == 2:
        return np.ascontiguousarray(layers[0], dtype=OBSTACLE_DTYPE).reshape(-1), np.ascontiguousarray(layers[1], dtype=np.int32).reshape(-1)
    first = np.zeros(len(layers) + 1, dtype=np.int32)
    first[1:] = np.cumsum([len(l) for l in layers])
    obs = np.zeros(int(first[-1]), dtype=OBSTACLE_DTYPE)
    n = 0
    for l in layers:
        for o in l:
            obs[n] = o
            n += 1
    return obs, first


# ---- moving agents (po_agent) ----
AGENT_DTYPE = np.dtype([("n_pts", np.int32), ("flags", np.int32), ("radius", np.float64), ("t", np.float64, (8,)), ("x", np.float64, (8,)),
                        ("y", np.float64, (8,))])  # po_agent, 208 bytes


def pack_agents(sets):
    """S sets of agents -> (agents [n_agents] of AGENT_DTYPE, first [S + 1] int32): set k owns agents[first[k]:first[k + 1]].  An agent is (radius, flags,
    [(t, x, y), ...]) with 1 .. 8 points; flags are abi.PO_AGENT_HOLD_BEFORE / PO_AGENT_HOLD_AFTER.  A tuple (agents, first) that is packed already passes through.
    Converted, not checked (a point list that is too long is refused here: it has no place in the record): the library checks."""
    if isinstance(sets, tuple) and len(sets) == 2:
        return np.ascontiguousarray(sets[0], dtype=AGENT_DTYPE).reshape(-1), np.ascontiguousarray(sets[1], dtype=np.int32).reshape(-1)
    first = np.zeros(len(sets) + 1, dtype=np.int32)
    first[1:] = np.cumsum([len(s) for s in sets])
    agents = np.zeros(int(first[-1]), dtype=AGENT_DTYPE)
    i = 0
    for s in sets:
        for radius, flags, pts in s:
            if len(pts) > 8:
                raise ValueError("an agent has at most 8 points (t, x, y)")
            agents[i]["n_pts"], agents[i]["flags"], agents[i]["radius"] = len(pts), int(flags), radius
            for j, (t, x, y) in enumerate(pts):
                agents[i]["t"][j], agents[i]["x"][j], agents[i]["y"][j] = t, x, y
            i += 1
    return agents, first


def _agent_lists(agents):
    """agents (what pack_agents takes) -> (the PoAgentLists of a host-pointer entry, agents, first).  The struct stores bare addresses: the CALLER holds the two
    packed arrays in locals until its C call has returned, as for _i32."""
    from .abi import PoAgentLists

    ag, first = pack_agents(agents)
    return PoAgentLists(_np(ag) if len(ag) else None, _np(first), len(ag), len(first) - 1), ag, first


def _agent_lists_device(t):
    """t["agents"] (a uint8 tensor over AGENT_DTYPE records, or None when there are none) and t["first"] [S + 1] i32 -> the PoAgentLists of a device-pointer entry
    (the caller's dict holds the tensors)."""
    from .abi import PoAgentLists

    ag = t.get("agents")
    n_agents = 0 if ag is None else ag.numel() * ag.element_size() // AGENT_DTYPE.itemsize
    return PoAgentLists(C.c_void_p(ag.data_ptr()) if n_agents else None, C.c_void_p(t["first"].data_ptr()), n_agents, t["first"].shape[0] - 1)


def pack_rings(shared, layers=None):
    """Rings -> the arrays of po_rings: (verts [n_verts, 2] float64, start [n_rings + 1] int32, flags [n_rings] int32, n_shared, first [M + 1] int32 or None).
    shared: a list of (xy array [n, 2], flag) every layer owns; layers: None, or M lists of (xy, flag), the rings of each layer alone.  flag is abi.PO_RING_SOLID or
    abi.PO_RING_FREE.  Converted, not checked: the library checks."""
    rings = list(shared) + ([] if layers is None else [r for l in layers for r in l])
    xy = [np.asarray(r[0], dtype=np.float64).reshape(-1, 2) for r in rings]
    start = np.zeros(len(rings) + 1, dtype=np.int32)
    start[1:] = np.cumsum([len(v) for v in xy])
    verts = np.concatenate(xy) if xy else np.zeros((0, 2))
    flags = np.array([int(r[1]) for r in rings], dtype=np.int32)
    first = None
    if layers is not None:
        first = np.full(len(layers) + 1, len(shared), dtype=np.int32)
        first[1:] += np.cumsum([len(l) for l in layers]).astype(np.int32)
    return np.ascontiguousarray(verts, dtype=np.float64), start, flags, len(shared), first


def _i32(a):
    """int32 view / copy of an optional index array.  The CALLER holds the result in a local until its C call has returned: the PoBatchIn / PoSplineIn ... structs
    store the bare address only (no module-level parking: another thread's calls would drop an array this thread's C call is still reading)."""
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


class Engine:
    """One handle = one HIP device + one stream (po_create / po_destroy)."""

    def __init__(self, device: int = 0, params: PoParams | None = None):
        self.params = params or default_params()
        self._h = C.c_void_p()
        _check(lib().po_create(device, C.byref(self.params), C.byref(self._h)))
        # developer conveniences of THIS Python plumbing (tools/*.py, A/B runs): PO_* environment variables are translated into po_debug_set calls
        # here; the C library itself reads no environment variable.  A switch this build does not have is
        # reported and ignored; any other failure destroys the handle before it propagates.
        try:
            for env, key in _ENV_DEBUG.items():
                v = os.environ.get(env)
                if v not in (None, "", "0"):
                    rc = lib().po_debug_set(self._h, key.encode(), int(v) if v.lstrip("-").isdigit() else 1)
                    if rc == PO_ERR_UNSUPPORTED:
                        sys.stderr.write(f"[path_optimizer_amd] {env} ignored: this build of libpo_hip.so has no '{key}' switch\n")
                    else:
                        _check(rc)
        except Exception:
            self.close()
            raise

    def debug_set(self, key: str, value: int):
        """po_debug_set: developer A/B switches (identity_order, debug_cycles, host_threads, smooth_seq, smooth_waves, smooth_nopad, smooth_debug, dp_one_wave, newton_slice, fixed_length, fixed_classes).
        Read-only keys go through debug_get: fixed_length_used, fixed_classes_used (paths of the last solve the constant-class Newton kernels took), "fixed_classes_flag:<b>" (did they take path b of it: 1 / 0, -1 when they did not run, PoError for a b outside the batch), newton_list_ok (the second sliced launch's lists: 1 in order, complete and — two lists — split as the flags say), dp_waves_used (8 or 1: the variant of the last DP lattice search; dp_one_wave = 1 forces 1), smooth_variant_used (100 * kind + 10 * waves + WPE of the last smoothing launch), fallback_paths,
        newton_parked, map_ptr, map_layers."""
        _check(lib().po_debug_set(self._h, key.encode(), int(value)))

    def debug_get(self, key: str) -> int:
        v = C.c_longlong()
        _check(lib().po_debug_get(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def close(self):
        if self._h:
            lib().po_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, raw_stream: int | None):
        _check(lib().po_set_stream(self._h, C.c_void_p(raw_stream or 0)))

    # ---- host-pointer path (H2D + solve + D2H) ----
    def solve_batch(self, batch, want_x: bool = False, order=None):
        """order: optional permutation of range(B) — scheduling hint (po_batch_in.order), results do not depend on it."""
        n, m, _ = problem_dims(batch.formulation, batch.N, batch.keep)
        npts, ordr = _i32(getattr(batch, 'n_points', None)), _i32(order)  # (locals: alive until po_solve_batch has returned)
        bi = PoBatchIn(batch.formulation, batch.B, batch.N, batch.keep, _np(batch.ref_x), _np(batch.ref_y), _np(batch.ref_z),
                       _np(batch.ref_k), _np(batch.ref_s), _np(batch.bounds), _np(batch.x0), _np(batch.goal_z), _np(batch.max_k), _np(batch.max_kp), _np(npts),
                       _np(ordr))
        states = np.zeros((batch.B, batch.N, 5))
        info = np.zeros(batch.B, dtype=INFO_DTYPE)
        xs = np.zeros((batch.B, n)) if want_x else None
        bo = PoBatchOut(_np(states), _np(info), _np(xs))
        _check(lib().po_solve_batch(self._h, C.byref(bi), C.byref(bo)))
        return states, info, xs

    def assemble_batch(self, batch):
        n, m, _ = problem_dims(batch.formulation, batch.N, batch.keep)
        npts = _i32(getattr(batch, 'n_points', None))
        bi = PoBatchIn(batch.formulation, batch.B, batch.N, batch.keep, _np(batch.ref_x), _np(batch.ref_y), _np(batch.ref_z),
                       _np(batch.ref_k), _np(batch.ref_s), _np(batch.bounds), _np(batch.x0), _np(batch.goal_z), _np(batch.max_k), _np(batch.max_kp), _np(npts))
        l = np.zeros((batch.B, m)); u = np.zeros((batch.B, m)); dyn = np.zeros((batch.B, batch.N - 1, 3))
        _check(lib().po_assemble_batch(self._h, C.byref(bi), _np(l), _np(u), _np(dyn)))
        return l, u, dyn

    def scaling_batch(self, batch):
        npts = _i32(getattr(batch, 'n_points', None))
        bi = PoBatchIn(batch.formulation, batch.B, batch.N, batch.keep, _np(batch.ref_x), _np(batch.ref_y), _np(batch.ref_z),
                       _np(batch.ref_k), _np(batch.ref_s), _np(batch.bounds), _np(batch.x0), _np(batch.goal_z), _np(batch.max_k), _np(batch.max_kp), _np(npts))
        out = np.zeros((batch.B, 64))
        _check(lib().po_scaling_batch(self._h, C.byref(bi), _np(out)))
        return out

    # ---- device-pointer path: tensors are torch CUDA(=HIP) tensors already resident in HBM ----
    def solve_batch_device(self, dev: "DeviceBatch"):
        bi = PoBatchIn(dev.formulation, dev.B, dev.N, dev.keep, *(None if t is None else t.data_ptr() for t in
                       (dev.ref_x, dev.ref_y, dev.ref_z, dev.ref_k, dev.ref_s, dev.bounds, dev.x0, dev.goal_z, dev.max_k, dev.max_kp, dev.n_points,
                        getattr(dev, "order", None))))
        bo = PoBatchOut(dev.out_states.data_ptr(), dev.out_info.data_ptr(), None if dev.out_x is None else dev.out_x.data_ptr())
        _check(lib().po_solve_batch_device(self._h, C.byref(bi), C.byref(bo)))

    # ---- post-solve step ----
    def set_map(self, dist, resolution, pos_x, pos_y):
        """Upload the obstacle-distance layer dist[size_x, size_y] (float32; kept column-major like grid_map's MatrixXf)."""
        from .abi import PoMap

        d = np.asfortranarray(dist, dtype=np.float32)
        m = PoMap(d.ctypes.data_as(C.c_void_p), d.shape[0], d.shape[1], float(resolution), float(pos_x), float(pos_y))
        _check(lib().po_set_map(self._h, C.byref(m)))

    # ---- the obstacle-distance layer from an occupancy image (po_edt.hip) ----
    @staticmethod
    def _occ_u8(occ):
        """uint8 occupancy (0 = occupied, non-zero = free) of any array: other dtypes go through `!= 0`, never through a wrapping cast."""
        a = np.asarray(occ)
        return a if a.dtype == np.uint8 else (a != 0).astype(np.uint8)

    def set_map_occupancy(self, occ, resolution, pos_x, pos_y):
        """Build the handle's map from the occupancy image occ[size_x, size_y] (uint8, 0 = occupied, non-zero = free; same index convention as set_map's
        `dist`): the exact Euclidean distance transform times `resolution` runs on the device, one byte per cell is uploaded."""
        from .abi import PoOccupancy

        o = np.asfortranarray(self._occ_u8(occ))
        if o.ndim != 2:
            raise ValueError("occ must be [size_x, size_y]")
        oc = PoOccupancy(o.ctypes.data_as(C.c_void_p), o.shape[0], o.shape[1], float(resolution), float(pos_x), float(pos_y))
        _check(lib().po_set_map_occupancy(self._h, C.byref(oc)))

    def set_map_occupancy_device(self, occ, resolution, pos_x, pos_y):
        """Device-pointer entry, enqueued on the handle's stream (no synchronisation; nothing is allocated when the size is the one the handle holds).
        occ: torch uint8 tensor on the handle's device, indexed [size_x, size_y] like set_map's `dist` and laid out so that x is contiguous, i.e. with strides
        (1, size_x): the transposed VIEW of a contiguous [size_y, size_x] image — `img_yx.t()`, or `torch.from_numpy(np.asfortranarray(occ_xy).T).to(dev).t()`.
        The tensor must stay alive until the stream has passed the call."""
        from .abi import PoOccupancy

        if occ.dim() != 2 or str(occ.dtype) != "torch.uint8":
            raise ValueError("occ must be a 2-d torch.uint8 tensor")
        sx, sy = int(occ.shape[0]), int(occ.shape[1])
        if (sx > 1 and occ.stride(0) != 1) or (sy > 1 and occ.stride(1) != sx):
            raise ValueError("occ must be indexed [size_x, size_y] with strides (1, size_x): pass img_yx.t() of a contiguous [size_y, size_x] image")
        oc = PoOccupancy(C.c_void_p(occ.data_ptr()), sx, sy, float(resolution), float(pos_x), float(pos_y))
        _check(lib().po_set_map_occupancy_device(self._h, C.byref(oc)))

    def distance_map_batch(self, occ, resolution):
        """The raw transform (host-pointer entry; the handle's map is not touched): occ [M, size_x, size_y] (0 = occupied) -> float32 [M, size_x, size_y],
        metres to the nearest occupied cell, bit-identical to float32(sqrt(d2)) * float32(resolution)."""
        from .abi import PoOccupancy

        o = self._occ_u8(occ)
        if o.ndim != 3:
            raise ValueError("occ must be [M, size_x, size_y]")
        M, sx, sy = o.shape
        img = np.ascontiguousarray(o.transpose(0, 2, 1))  # [M][size_y][size_x], x contiguous
        out = np.empty((M, sy, sx), dtype=np.float32)
        oc = PoOccupancy(img.ctypes.data_as(C.c_void_p), sx, sy, float(resolution), 0.0, 0.0)
        _check(lib().po_distance_map_batch(self._h, M, C.byref(oc), _np(out)))
        return out.transpose(0, 2, 1)

    def get_map(self):
        """The handle's current map, in set_map's argument order: (dist [size_x, size_y] float32, resolution, pos_x, pos_y) — eng2.set_map(*eng.get_map())."""
        from .abi import PoMap

        m = PoMap()
        _check(lib().po_get_map(self._h, C.byref(m), None))
        d = np.empty((m.size_x, m.size_y), dtype=np.float32, order="F")
        _check(lib().po_get_map(self._h, C.byref(m), d.ctypes.data_as(C.c_void_p)))
        return d, m.resolution, m.pos_x, m.pos_y

    # ---- per-instance maps: a stack of layers and an assignment of instances to layers ----
    @staticmethod
    def _pos_xy(pos_xy, M):
        if pos_xy is None:
            return None
        p = np.ascontiguousarray(pos_xy, dtype=np.float64)
        if p.shape != (M, 2):
            raise ValueError("pos_xy must be [M, 2]")
        return p

    def set_map_stack(self, dists, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0):
        """Install M distance layers dists[M, size_x, size_y] (float32, each indexed like set_map's `dist`).  pos_xy [M, 2]: the centre of each layer; None: every
        layer at (pos_x, pos_y)."""
        from .abi import PoMap

        d = np.asarray(dists, dtype=np.float32)
        if d.ndim != 3:
            raise ValueError("dists must be [M, size_x, size_y]")
        M, sx, sy = d.shape
        mem = np.ascontiguousarray(d.transpose(0, 2, 1))  # [M][size_y][size_x], x contiguous
        pos = self._pos_xy(pos_xy, M)
        m = PoMap(mem.ctypes.data_as(C.c_void_p), sx, sy, float(resolution), float(pos_x), float(pos_y))
        _check(lib().po_set_map_stack(self._h, M, C.byref(m), _np(pos)))

    def set_map_stack_occupancy(self, occ, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0):
        """Build the stack from M occupancy images occ[M, size_x, size_y] (0 = occupied) on the device; layers bit-identical to distance_map_batch(occ)."""
        from .abi import PoOccupancy

        o = self._occ_u8(occ)
        if o.ndim != 3:
            raise ValueError("occ must be [M, size_x, size_y]")
        M, sx, sy = o.shape
        img = np.ascontiguousarray(o.transpose(0, 2, 1))
        pos = self._pos_xy(pos_xy, M)
        oc = PoOccupancy(img.ctypes.data_as(C.c_void_p), sx, sy, float(resolution), float(pos_x), float(pos_y))
        _check(lib().po_set_map_stack_occupancy(self._h, M, C.byref(oc), _np(pos)))

    def set_map_stack_occupancy_device(self, occ, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0):
        """Device-pointer entry, enqueued on the handle's stream (no synchronisation and no allocation when M and the size are those the handle holds).
        occ: CONTIGUOUS torch uint8 tensor [M, size_y, size_x] on the handle's device (x contiguous, image after image); pos_xy: contiguous torch float64 tensor
        [M, 2] on the device, or None.  Both must stay alive until the stream has passed the call."""
        from .abi import PoOccupancy

        if occ.dim() != 3 or str(occ.dtype) != "torch.uint8" or not occ.is_contiguous():
            raise ValueError("occ must be a contiguous 3-d torch.uint8 tensor [M, size_y, size_x]")
        M, sy, sx = (int(v) for v in occ.shape)
        if pos_xy is not None and (tuple(pos_xy.shape) != (M, 2) or str(pos_xy.dtype) != "torch.float64" or not pos_xy.is_contiguous()):
            raise ValueError("pos_xy must be a contiguous torch.float64 tensor [M, 2]")
        oc = PoOccupancy(C.c_void_p(occ.data_ptr()), sx, sy, float(resolution), float(pos_x), float(pos_y))
        _check(lib().po_set_map_stack_occupancy_device(self._h, M, C.byref(oc), None if pos_xy is None else C.c_void_p(pos_xy.data_ptr())))

    # ---- the stack from per-layer obstacle lists, rasterised on the device (po_raster.hip) ----
    def _host_lists(self, layers, size_x, size_y, resolution, pos_xy, pos_x, pos_y, base):
        """(M, PoObstacleLists, pos array, the arrays the struct points into): host pointers."""
        from .abi import PoObstacleLists

        obs, first = pack_obstacles(layers)
        M = len(first) - 1
        b, nb = None, 0
        if base is not None:
            b = self._occ_u8(base)
            if b.shape == (size_x, size_y):
                b = b[None]
            if b.ndim != 3 or b.shape[1:] != (size_x, size_y):
                raise ValueError("base must be [size_x, size_y] or [M, size_x, size_y]")
            nb = b.shape[0]
            b = np.ascontiguousarray(b.transpose(0, 2, 1))  # [n][size_y][size_x], x contiguous
        pos = self._pos_xy(pos_xy, M)
        ls = PoObstacleLists(_np(obs) if len(obs) else None, _np(first), len(obs), _np(b), nb, int(size_x), int(size_y), float(resolution), float(pos_x), float(pos_y))
        return M, ls, pos, (obs, first, b)

    def rasterize_batch(self, layers, size_x, size_y, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0, base=None):
        """M obstacle lists -> M occupancy images, uint8 [M, size_x, size_y] (0 = occupied, 255 = free), on the device; the handle's map is not touched.
        layers: M lists of obstacle_disc / obstacle_box / obstacle_polygon records (or a packed (obs, first) tuple, see pack_obstacles); base: None, one image
        [size_x, size_y] shared by every layer, or [M, size_x, size_y] (0 = occupied); pos_xy [M, 2]: the centre of each layer, None: every layer at (pos_x, pos_y)."""
        M, ls, pos, keep = self._host_lists(layers, size_x, size_y, resolution, pos_xy, pos_x, pos_y, base)
        out = np.empty((M, size_y, size_x), dtype=np.uint8)
        _check(lib().po_rasterize_batch(self._h, M, C.byref(ls), _np(pos), _np(out)))
        return out.transpose(0, 2, 1)

    def set_map_stack_obstacles(self, layers, size_x, size_y, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0, base=None):
        """Build the stack from M obstacle lists: rasterised and transformed on the device; only the lists (136 bytes per obstacle), the centres and the base are
        uploaded.  Layers bit-identical to set_map_stack_occupancy(rasterize_batch(...)).  Arguments as rasterize_batch."""
        M, ls, pos, keep = self._host_lists(layers, size_x, size_y, resolution, pos_xy, pos_x, pos_y, base)
        _check(lib().po_set_map_stack_obstacles(self._h, M, C.byref(ls), _np(pos)))

    @staticmethod
    def _device_lists(obs, first, size_x, size_y, resolution, pos_xy, pos_x, pos_y, base):
        from .abi import PoObstacleLists

        if str(obs.dtype) != "torch.uint8" or obs.dim() != 2 or obs.shape[1] != OBSTACLE_DTYPE.itemsize or not obs.is_contiguous():
            raise ValueError("obs must be a contiguous torch.uint8 tensor [n_obs, 136]: the bytes of an OBSTACLE_DTYPE array")
        if first.dim() != 1 or str(first.dtype) != "torch.int32" or not first.is_contiguous() or first.shape[0] < 2:
            raise ValueError("first must be a contiguous torch.int32 tensor [M + 1]")
        M = int(first.shape[0]) - 1
        nb = 0
        if base is not None:
            if str(base.dtype) != "torch.uint8" or base.dim() != 3 or tuple(base.shape[1:]) != (size_y, size_x) or not base.is_contiguous():
                raise ValueError("base must be a contiguous torch.uint8 tensor [1 or M, size_y, size_x]")
            nb = int(base.shape[0])
        if pos_xy is not None and (tuple(pos_xy.shape) != (M, 2) or str(pos_xy.dtype) != "torch.float64" or not pos_xy.is_contiguous()):
            raise ValueError("pos_xy must be a contiguous torch.float64 tensor [M, 2]")
        n_obs = int(obs.shape[0])
        ls = PoObstacleLists(C.c_void_p(obs.data_ptr()) if n_obs else None, C.c_void_p(first.data_ptr()), n_obs, None if base is None else C.c_void_p(base.data_ptr()), nb,
                             int(size_x), int(size_y), float(resolution), float(pos_x), float(pos_y))
        return M, ls, None if pos_xy is None else C.c_void_p(pos_xy.data_ptr())

    def rasterize_batch_device(self, obs, first, out, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0, base=None):
        """Device-pointer entry, enqueued on the handle's stream.  obs: torch uint8 [n_obs, 136] (torch.from_numpy(obs_array.view(np.uint8).reshape(-1, 136)));
        first: torch int32 [M + 1]; out: contiguous torch uint8 [M, size_y, size_x]; base: torch uint8 [1 or M, size_y, size_x] or None; pos_xy: torch float64
        [M, 2] or None.  The lists are NOT validated (n_verts and first[] are read clamped).  Every tensor must stay alive until the stream has passed the call."""
        if str(out.dtype) != "torch.uint8" or out.dim() != 3 or not out.is_contiguous():
            raise ValueError("out must be a contiguous torch.uint8 tensor [M, size_y, size_x]")
        sy, sx = int(out.shape[1]), int(out.shape[2])
        M, ls, pos = self._device_lists(obs, first, sx, sy, resolution, pos_xy, pos_x, pos_y, base)
        if int(out.shape[0]) != M:
            raise ValueError("out must hold M = len(first) - 1 images")
        _check(lib().po_rasterize_batch_device(self._h, M, C.byref(ls), pos, C.c_void_p(out.data_ptr())))

    def set_map_stack_obstacles_device(self, obs, first, size_x, size_y, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0, base=None):
        """Device-pointer entry, enqueued on the handle's stream (no synchronisation and no allocation when M and the size are those the handle holds).
        Tensors as rasterize_batch_device."""
        M, ls, pos = self._device_lists(obs, first, int(size_x), int(size_y), resolution, pos_xy, pos_x, pos_y, base)
        _check(lib().po_set_map_stack_obstacles_device(self._h, M, C.byref(ls), pos))

    # ---- the static world: a world grid on the handle and polygon rings (po_scene.hip) ----
    def set_world_occupancy(self, world, resolution, pos_x=0.0, pos_y=0.0, outside_occupied=False):
        """Install the site's static occupancy grid world[size_x, size_y] (0 = occupied; its own resolution and centre) on the handle; None clears it.  Scene
        calls with use_world=True read it: a layer cell is occupied when the world cell under its centre is, or, outside the world, when outside_occupied."""
        from .abi import PoOccupancy

        if world is None:
            _check(lib().po_set_world_occupancy(self._h, None, 0))
            return
        w = np.asfortranarray(self._occ_u8(world))
        if w.ndim != 2:
            raise ValueError("world must be [size_x, size_y]")
        oc = PoOccupancy(w.ctypes.data_as(C.c_void_p), w.shape[0], w.shape[1], float(resolution), float(pos_x), float(pos_y))
        _check(lib().po_set_world_occupancy(self._h, C.byref(oc), int(bool(outside_occupied))))

    def set_world_occupancy_device(self, world, resolution, pos_x=0.0, pos_y=0.0, outside_occupied=False):
        """Device-pointer entry: world is a CONTIGUOUS torch uint8 tensor [size_y, size_x] on the handle's device (x contiguous), copied into the handle's block
        on the stream; it must stay alive until the stream has passed the call."""
        from .abi import PoOccupancy

        if world.dim() != 2 or str(world.dtype) != "torch.uint8" or not world.is_contiguous():
            raise ValueError("world must be a contiguous 2-d torch.uint8 tensor [size_y, size_x]")
        oc = PoOccupancy(C.c_void_p(world.data_ptr()), int(world.shape[1]), int(world.shape[0]), float(resolution), float(pos_x), float(pos_y))
        _check(lib().po_set_world_occupancy_device(self._h, C.byref(oc), int(bool(outside_occupied))))

    def _host_scene(self, layers, rings, use_world, size_x, size_y, resolution, pos_xy, pos_x, pos_y, base):
        """(M, PoScene, pos array, the arrays the struct points into): host pointers.  rings: None, or what pack_rings returns."""
        from .abi import PoRings, PoScene

        M, ls, pos, keep = self._host_lists(layers, size_x, size_y, resolution, pos_xy, pos_x, pos_y, base)
        rg = PoRings()
        if rings is not None:
            verts = np.ascontiguousarray(rings[0], dtype=np.float64).reshape(-1, 2)
            start, flags = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in rings[1:3])
            first = _i32(rings[4])
            if len(start) != len(flags) + 1 or (first is not None and first.shape != (M + 1,)):
                raise ValueError("rings: start must be [n_rings + 1], flags [n_rings] and first None or [M + 1]")
            rg = PoRings(_np(verts), _np(start), _np(flags), len(flags), len(verts), int(rings[3]), _np(first))
            keep = keep + (verts, start, flags, first)
        return M, PoScene(ls, rg, int(bool(use_world))), pos, keep

    def rasterize_scene_batch(self, layers, rings, size_x, size_y, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0, base=None, use_world=False):
        """rasterize_batch plus the static world: rings (pack_rings(shared, per_layer) or None) and, with use_world, the handle's world grid.  uint8
        [M, size_x, size_y], 0 = occupied, 255 = free; the handle's map is not touched."""
        M, sc, pos, keep = self._host_scene(layers, rings, use_world, size_x, size_y, resolution, pos_xy, pos_x, pos_y, base)
        out = np.empty((M, size_y, size_x), dtype=np.uint8)
        _check(lib().po_rasterize_scene_batch(self._h, M, C.byref(sc), _np(pos), _np(out)))
        return out.transpose(0, 2, 1)

    def set_map_stack_scene(self, layers, rings, size_x, size_y, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0, base=None, use_world=False):
        """Build the stack from M scenes: rasterised and transformed on the device.  Layers bit-identical to set_map_stack_occupancy(rasterize_scene_batch(...))."""
        M, sc, pos, keep = self._host_scene(layers, rings, use_world, size_x, size_y, resolution, pos_xy, pos_x, pos_y, base)
        _check(lib().po_set_map_stack_scene(self._h, M, C.byref(sc), _np(pos)))

    def _device_scene(self, obs, first, rings, use_world, size_x, size_y, resolution, pos_xy, pos_x, pos_y, base):
        """rings: None or (verts float64 [n_verts, 2], start int32 [n_rings + 1], flags int32 [n_rings], n_shared, first int32 [M + 1] or None), contiguous torch
        tensors on the handle's device.  The tables are NOT validated (the kernel reads them clamped)."""
        from .abi import PoRings, PoScene

        M, ls, pos = self._device_lists(obs, first, size_x, size_y, resolution, pos_xy, pos_x, pos_y, base)
        rg = PoRings()
        if rings is not None:
            verts, start, flags, n_shared, rfirst = rings
            if not hasattr(verts, "data_ptr") or str(verts.dtype) != "torch.float64" or verts.dim() != 2 or verts.shape[1] != 2 or not verts.is_contiguous():
                raise ValueError("rings: verts must be a contiguous torch.float64 tensor [n_verts, 2]")
            def i32_ok(a, n=None):
                return hasattr(a, "data_ptr") and a.dim() == 1 and str(a.dtype) == "torch.int32" and a.is_contiguous() and (n is None or int(a.shape[0]) == n)

            if not i32_ok(start) or int(start.shape[0]) < 1:
                raise ValueError("rings: start must be a contiguous torch.int32 tensor [n_rings + 1]")
            if not i32_ok(flags, int(start.shape[0]) - 1) or (rfirst is not None and not i32_ok(rfirst, M + 1)):
                raise ValueError("rings: flags must be a contiguous torch.int32 tensor [n_rings] and first None or one of [M + 1]")
            rg = PoRings(C.c_void_p(verts.data_ptr()) if verts.shape[0] else None, C.c_void_p(start.data_ptr()), C.c_void_p(flags.data_ptr()) if flags.shape[0] else None,
                         int(flags.shape[0]), int(verts.shape[0]), int(n_shared), None if rfirst is None else C.c_void_p(rfirst.data_ptr()))
        return M, PoScene(ls, rg, int(bool(use_world))), pos

    def rasterize_scene_batch_device(self, obs, first, rings, out, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0, base=None, use_world=False):
        """Device-pointer entry, enqueued on the handle's stream: rasterize_batch_device plus rings (see _device_scene) and the handle's world grid."""
        if str(out.dtype) != "torch.uint8" or out.dim() != 3 or not out.is_contiguous():
            raise ValueError("out must be a contiguous torch.uint8 tensor [M, size_y, size_x]")
        sy, sx = int(out.shape[1]), int(out.shape[2])
        M, sc, pos = self._device_scene(obs, first, rings, use_world, sx, sy, resolution, pos_xy, pos_x, pos_y, base)
        if int(out.shape[0]) != M:
            raise ValueError("out must hold M = len(first) - 1 images")
        _check(lib().po_rasterize_scene_batch_device(self._h, M, C.byref(sc), pos, C.c_void_p(out.data_ptr())))

    def set_map_stack_scene_device(self, obs, first, rings, size_x, size_y, resolution, pos_xy=None, pos_x=0.0, pos_y=0.0, base=None, use_world=False):
        """Device-pointer entry, enqueued on the handle's stream (no synchronisation and no allocation when M and the size are those the handle holds)."""
        M, sc, pos = self._device_scene(obs, first, rings, use_world, int(size_x), int(size_y), resolution, pos_xy, pos_x, pos_y, base)
        _check(lib().po_set_map_stack_scene_device(self._h, M, C.byref(sc), pos))

    def set_map_assignment(self, layer_of):
        """layer_of[b] = the layer instance b of every map-reading batch call reads (validated: outside [0, M) raises and the previous table stays); None or
        empty clears the table — every instance reads layer 0."""
        a = None if layer_of is None else np.ascontiguousarray(layer_of, dtype=np.int32).reshape(-1)
        _check(lib().po_set_map_assignment(self._h, 0 if a is None else len(a), _np(a)))

    def set_map_assignment_device(self, layer_of):
        """Device-pointer entry: contiguous torch int32 tensor [n], copied on the handle's stream (not validated: the kernels clamp each index into [0, M - 1])."""
        if layer_of is None:
            _check(lib().po_set_map_assignment_device(self._h, 0, None))
            return
        if layer_of.dim() != 1 or str(layer_of.dtype) != "torch.int32" or not layer_of.is_contiguous():
            raise ValueError("layer_of must be a contiguous 1-d torch.int32 tensor")
        _check(lib().po_set_map_assignment_device(self._h, int(layer_of.shape[0]), C.c_void_p(layer_of.data_ptr())))

    def get_map_layer(self, k: int):
        """Layer k of the handle's stack, like get_map: (dist [size_x, size_y] float32, resolution, pos_x, pos_y)."""
        from .abi import PoMap

        m = PoMap()
        _check(lib().po_get_map_layer(self._h, int(k), C.byref(m), None))
        d = np.empty((m.size_x, m.size_y), dtype=np.float32, order="F")
        _check(lib().po_get_map_layer(self._h, int(k), C.byref(m), d.ctypes.data_as(C.c_void_p)))
        return d, m.resolution, m.pos_x, m.pos_y

    def map_sample_layer(self, k: int, xy):
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        d = np.zeros(len(xy)); ins = np.zeros(len(xy), dtype=np.int32)
        _check(lib().po_map_sample_layer(self._h, int(k), len(xy), _np(xy), _np(d), _np(ins)))
        return d, ins

    def postcheck_batch(self, states, info, n_points=None):
        """Host-pointer entry: states [B,N,5], info structured array -> n_valid [B], ok [B]."""
        states = np.ascontiguousarray(states, dtype=np.float64)
        info = np.ascontiguousarray(info)
        B, N = states.shape[0], states.shape[1]
        nv = np.zeros(B, dtype=np.int32); ok = np.zeros(B, dtype=np.int32)
        npts = _i32(n_points)
        _check(lib().po_postcheck_batch(self._h, B, N, _np(npts), _np(states), _np(info), _np(nv), _np(ok)))
        return nv, ok

    def densify_batch(self, states, info, M: int, n_points=None):
        """optimizePath's densifying output branch (host-pointer entry): states [B,N,5], info -> out [B,M,5], n_out [B], ok [B]."""
        states = np.ascontiguousarray(states, dtype=np.float64)
        info = np.ascontiguousarray(info)
        B, N = states.shape[0], states.shape[1]
        out = np.zeros((B, M, 5)); n = np.zeros(B, dtype=np.int32); ok = np.zeros(B, dtype=np.int32)
        npts = _i32(n_points)
        _check(lib().po_densify_batch(self._h, B, N, _np(npts), _np(states), _np(info), M, _np(out), _np(n), _np(ok)))
        return out, n, ok

    def postcheck_batch_device(self, dev: "DeviceBatch", n_valid, ok):
        """Device-pointer entry on the outputs of solve_batch_device; n_valid / ok are int32 torch tensors [B]."""
        _check(lib().po_postcheck_batch_device(self._h, dev.B, dev.N, None if dev.n_points is None else C.c_void_p(dev.n_points.data_ptr()),
                                               C.c_void_p(dev.out_states.data_ptr()), C.c_void_p(dev.out_info.data_ptr()),
                                               C.c_void_p(n_valid.data_ptr()), C.c_void_p(ok.data_ptr())))

    # ---- corridor-bounds producer ----
    def bounds_batch(self, paths: dict, n_points=None, n_knots=None):
        """Host-pointer entry. paths: dict of [B,N] ref_x/ref_y/ref_z/ref_s and [B,K] knot_s/knot_x/knot_y (synth.make_spline_paths).
        Returns bounds [B,N,4,2] (lb, ub), n_valid [B]."""
        from .abi import PoBoundsIn

        f = lambda k: np.ascontiguousarray(paths[k], dtype=np.float64)
        arr = {k: f(k) for k in ("ref_x", "ref_y", "ref_z", "ref_s", "knot_s", "knot_x", "knot_y")}
        B, N = arr["ref_x"].shape
        K = arr["knot_s"].shape[1]
        npts, nk = _i32(n_points), _i32(n_knots)
        bi = PoBoundsIn(B, N, K, _np(arr["ref_x"]), _np(arr["ref_y"]), _np(arr["ref_z"]), _np(arr["ref_s"]), _np(npts),
                        _np(arr["knot_s"]), _np(arr["knot_x"]), _np(arr["knot_y"]), _np(nk))
        bounds = np.zeros((B, N, 4, 2)); nv = np.zeros(B, dtype=np.int32)
        _check(lib().po_bounds_batch(self._h, C.byref(bi), _np(bounds), _np(nv)))
        return bounds, nv

    def bounds_batch_device(self, t: dict, bounds, n_valid):
        """Device-pointer entry: t holds torch tensors (same keys as bounds_batch), bounds [B,N,4,2] f64 and n_valid [B] i32 are outputs."""
        from .abi import PoBoundsIn

        B, N = t["ref_x"].shape
        K = t["knot_s"].shape[1]
        p = lambda k: None if t.get(k) is None else C.c_void_p(t[k].data_ptr())
        bi = PoBoundsIn(B, N, K, p("ref_x"), p("ref_y"), p("ref_z"), p("ref_s"), p("n_points"), p("knot_s"), p("knot_x"), p("knot_y"), p("n_knots"))
        _check(lib().po_bounds_batch_device(self._h, C.byref(bi), C.c_void_p(bounds.data_ptr()), C.c_void_p(n_valid.data_ptr())))

    # ---- reference-smoothing QPs ----
    def smooth_batch(self, kind: int, inp: dict, want_raw: bool = False):
        """Host-pointer entry. inp: dict of [B,P] arrays x, y, angle, k, s (TENSION2 / TENSION) or s, lb, ub + l0 [B] (POST), optional
        n_points [B] (synth.make_smooth_inputs).  Returns out_x, out_y, out_s [B,P], info [B] (+ raw [B,n_max] in the reference order)."""
        from .abi import PoSmoothIn, PoSmoothOut

        f = lambda k: None if inp.get(k) is None else np.ascontiguousarray(inp[k], dtype=np.float64)
        arr = {k: f(k) for k in ("x", "y", "angle", "k", "s", "lb", "ub", "l0")}
        B, P = arr["s"].shape
        npts = _i32(inp.get("n_points"))
        si = PoSmoothIn(kind, B, P, _np(npts), *[_np(arr[k]) for k in ("x", "y", "angle", "k", "s", "lb", "ub", "l0")])
        ox = np.zeros((B, P)); oy = np.zeros((B, P)); os_ = np.zeros((B, P))
        info = np.zeros(B, dtype=INFO_DTYPE)
        raw = np.zeros((B, smooth_dims(kind, P)[0])) if want_raw else None
        so = PoSmoothOut(_np(ox), _np(oy), _np(os_), _np(info), _np(raw))
        _check(lib().po_smooth_batch(self._h, C.byref(si), C.byref(so)))
        return ox, oy, os_, info, raw

    def smooth_batch_device(self, kind: int, t: dict, out: dict):
        """Device-pointer entry: t / out hold torch tensors (keys as above; out: x, y, s [B,P] f64, info [B,sizeof(po_info)] u8, optional raw)."""
        from .abi import PoSmoothIn, PoSmoothOut

        B, P = t["s"].shape
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        si = PoSmoothIn(kind, B, P, p(t, "n_points"), *[p(t, k) for k in ("x", "y", "angle", "k", "s", "lb", "ub", "l0")])
        so = PoSmoothOut(p(out, "x"), p(out, "y"), p(out, "s"), p(out, "info"), p(out, "raw"))
        _check(lib().po_smooth_batch_device(self._h, C.byref(si), C.byref(so)))

    # ---- reference re-sampling, limits, DP lattice search ----
    @staticmethod
    def _spline_in(sp: dict, length, n_knots=None):
        from .abi import PoSplineIn

        arr = {k: np.ascontiguousarray(sp[k], dtype=np.float64) for k in ("knot_s", "knot_x", "knot_y")}
        arr["length"] = np.ascontiguousarray(length, dtype=np.float64)
        B, K = arr["knot_s"].shape
        nk = arr["n_knots"] = _i32(n_knots)  # (travels with `arr`, which the caller holds until its C call has returned)
        return PoSplineIn(B, K, _np(arr["knot_s"]), _np(arr["knot_x"]), _np(arr["knot_y"]), _np(nk), _np(arr["length"])), arr, B

    def resample_batch(self, sp: dict, length, ds_smaller: float, ds_larger: float, N: int, n_knots=None):
        """buildReferenceFromSpline over a batch of splines (knots knot_s/knot_x/knot_y [B,K], length [B]).  Returns dict ref_x, ref_y,
        ref_z, ref_k, ref_s [B,N] and n_points [B]."""
        si, keep, B = self._spline_in(sp, length, n_knots)
        out = {k: np.zeros((B, N)) for k in ("ref_x", "ref_y", "ref_z", "ref_k", "ref_s")}
        npts = np.zeros(B, dtype=np.int32)
        _check(lib().po_resample_batch(self._h, C.byref(si), C.c_double(ds_smaller), C.c_double(ds_larger), N, _np(out["ref_x"]), _np(out["ref_y"]),
                                       _np(out["ref_z"]), _np(out["ref_k"]), _np(out["ref_s"]), _np(npts)))
        out["n_points"] = npts
        return out

    def limits_batch(self, v, a, n_points=None):
        v = np.ascontiguousarray(v, dtype=np.float64); a = np.ascontiguousarray(a, dtype=np.float64)
        B, N = v.shape
        mk = np.zeros((B, N)); mkp = np.zeros((B, N))
        npts = _i32(n_points)
        _check(lib().po_limits_batch(self._h, B, N, _np(npts), _np(v), _np(a), _np(mk), _np(mkp)))
        return mk, mkp

    def dp_search_batch(self, sp: dict, length, start, L: int, n_knots=None):
        """graphSearchDp over a batch.  start [B,3] = (x, y, heading).  Returns layer_s, lb, ub [B,L], l0 [B], n_layers [B]."""
        si, keep, B = self._spline_in(sp, length, n_knots)
        start = np.ascontiguousarray(start, dtype=np.float64)
        ls = np.zeros((B, L)); lb = np.zeros((B, L)); ub = np.zeros((B, L)); l0 = np.zeros(B); nl = np.zeros(B, dtype=np.int32)
        _check(lib().po_dp_search_batch(self._h, C.byref(si), _np(start), L, _np(ls), _np(lb), _np(ub), _np(l0), _np(nl)))
        return ls, lb, ub, l0, nl

    def dp_search_batch_device(self, t: dict, start, L: int, out: dict):
        """Device-pointer entry: t holds torch tensors knot_s/knot_x/knot_y [B,K], length [B]; start [B,3]; out: layer_s, lb, ub [B,L], l0 [B], n_layers [B] i32."""
        from .abi import PoSplineIn

        B, K = t["knot_s"].shape
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        si = PoSplineIn(B, K, p(t, "knot_s"), p(t, "knot_x"), p(t, "knot_y"), p(t, "n_knots"), p(t, "length"))
        _check(lib().po_dp_search_batch_device(self._h, C.byref(si), C.c_void_p(start.data_ptr()), L, p(out, "layer_s"), p(out, "lb"), p(out, "ub"),
                                               p(out, "l0"), p(out, "n_layers")))

    def resample_batch_device(self, t: dict, ds_smaller: float, ds_larger: float, N: int, out: dict):
        from .abi import PoSplineIn

        B, K = t["knot_s"].shape
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        si = PoSplineIn(B, K, p(t, "knot_s"), p(t, "knot_x"), p(t, "knot_y"), p(t, "n_knots"), p(t, "length"))
        _check(lib().po_resample_batch_device(self._h, C.byref(si), C.c_double(ds_smaller), C.c_double(ds_larger), N, p(out, "ref_x"), p(out, "ref_y"),
                                              p(out, "ref_z"), p(out, "ref_k"), p(out, "ref_s"), p(out, "n_points")))

    # ---- PathOptimizer::solve for a batch of planning instances ----
    def plan_batch(self, way_x, way_y, start, goal, N: int = 512, n_way=None, max_length: float = 0.0):
        """Host-pointer entry of po_plan_batch.  way_x / way_y [B,W], start [B,4] (x, y, heading, k), goal [B,3].
        Returns states [B,N,5], n_states [B], ok [B], stage [B], info [B]."""
        from .abi import PoPlanIn, PoPlanOut

        wx = np.ascontiguousarray(way_x, dtype=np.float64); wy = np.ascontiguousarray(way_y, dtype=np.float64)
        st = np.ascontiguousarray(start, dtype=np.float64); gl = np.ascontiguousarray(goal, dtype=np.float64)
        B, W = wx.shape
        nw = _i32(n_way)
        pi = PoPlanIn(B, W, _np(nw), _np(wx), _np(wy), _np(st), _np(gl), float(max_length), N)
        states = np.zeros((B, N, 5)); n = np.zeros(B, dtype=np.int32); ok = np.zeros(B, dtype=np.int32); stage = np.zeros(B, dtype=np.int32)
        info = np.zeros(B, dtype=INFO_DTYPE)
        po = PoPlanOut(_np(states), _np(n), _np(ok), _np(stage), _np(info))
        _check(lib().po_plan_batch(self._h, C.byref(pi), C.byref(po)))
        return states, n, ok, stage, info

    def plan_batch_device(self, t: dict, out: dict, N: int, max_length: float):
        """Device-pointer entry: t: way_x, way_y [B,W], start [B,4], goal [B,3] (+ n_way); out: states [B,N,5], n_states, ok (+ stage, info [B,sizeof(po_info)] u8)."""
        from .abi import PoPlanIn, PoPlanOut

        B, W = t["way_x"].shape
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        pi = PoPlanIn(B, W, p(t, "n_way"), p(t, "way_x"), p(t, "way_y"), p(t, "start"), p(t, "goal"), float(max_length), N)
        po = PoPlanOut(p(out, "states"), p(out, "n_states"), p(out, "ok"), p(out, "stage"), p(out, "info"))
        _check(lib().po_plan_batch_device(self._h, C.byref(pi), C.byref(po)))

    # ---- score and select: one winner per group of candidates ----
    def select_batch(self, states, group_start, n_states=None, ok=None, goal=None, prev_states=None, prev_n=None, params=None, want_states=True):
        """Host-pointer entry of po_select_batch.  states [B,N,5], group_start [G+1]; optional n_states [B], ok [B], goal [B,>=2], prev_states [G,Np,5], prev_n [G].
        Returns a dict: feat [B,8], cost [B], best [G], best_cost [G], n_feasible [G], sel_states [G,N,5] and sel_n [G] (None without want_states)."""
        from .abi import PO_N_FEAT, PoSelectIn, PoSelectOut

        states = np.ascontiguousarray(states, dtype=np.float64)
        B, N = states.shape[0], states.shape[1]
        gs = _i32(group_start).reshape(-1)
        G = len(gs) - 1
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        gl, pv = f(goal), f(prev_states)
        ns, okk, pn = _i32(n_states), _i32(ok), _i32(prev_n)
        si = PoSelectIn(B, N, _np(states), _np(ns), _np(okk), _np(gl), 0 if gl is None else gl.shape[1], G, _np(gs), 0 if pv is None else pv.shape[1], _np(pv), _np(pn))
        r = {"feat": np.zeros((B, PO_N_FEAT)), "cost": np.zeros(B), "best": np.zeros(G, dtype=np.int32), "best_cost": np.zeros(G),
             "n_feasible": np.zeros(G, dtype=np.int32), "sel_states": np.zeros((G, N, 5)) if want_states else None,
             "sel_n": np.zeros(G, dtype=np.int32) if want_states else None}
        so = PoSelectOut(*[_np(r[k]) for k in ("feat", "cost", "best", "best_cost", "n_feasible", "sel_states", "sel_n")])
        sp = params if params is not None else default_select_params()
        _check(lib().po_select_batch(self._h, C.byref(sp), C.byref(si), C.byref(so)))
        return r

    def select_batch_device(self, t: dict, out: dict, params=None):
        """Device-pointer entry: t: states [B,N,5] f64, group_start [G+1] i32 (+ n_states, ok, goal [B,stride], prev_states [G,Np,5], prev_n); out: best [G] i32
        (+ feat [B,8], cost [B], best_cost [G], n_feasible [G], sel_states [G,N,5] with sel_n [G]).  Enqueued on the handle's stream, no synchronisation."""
        from .abi import PoSelectIn, PoSelectOut

        B, N = t["states"].shape[0], t["states"].shape[1]
        G = t["group_start"].shape[0] - 1
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        gl, pv = t.get("goal"), t.get("prev_states")
        si = PoSelectIn(B, N, p(t, "states"), p(t, "n_states"), p(t, "ok"), p(t, "goal"), 0 if gl is None else int(gl.stride(0)), G, p(t, "group_start"),
                        0 if pv is None else int(pv.shape[1]), p(t, "prev_states"), p(t, "prev_n"))
        so = PoSelectOut(*[p(out, k) for k in ("feat", "cost", "best", "best_cost", "n_feasible", "sel_states", "sel_n")])
        sp = params if params is not None else default_select_params()
        _check(lib().po_select_batch_device(self._h, C.byref(sp), C.byref(si), C.byref(so)))

    # ---- speed profile: v, a, t for every state of every path ----
    def speed_batch(self, states, v0, n_states=None, ok=None, v_end=None, v_limit=None, params=None, want_t=True):
        """Host-pointer entry of po_speed_batch.  states [B,N,5], v0 [B]; optional n_states [B], ok [B], v_end [B], v_limit [B,N] (negative or NaN: no limit).
        Returns a dict: v, a [B,N] (what limits_batch reads), t [B,N] and total_time [B] (None without want_t), status [B]."""
        from .abi import PoSpeedIn, PoSpeedOut

        states = np.ascontiguousarray(states, dtype=np.float64)
        B, N = states.shape[0], states.shape[1]
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        v0, ve, vl = f(v0), f(v_end), f(v_limit)
        ns, okk = _i32(n_states), _i32(ok)
        si = PoSpeedIn(B, N, _np(states), _np(ns), _np(okk), _np(v0), _np(ve), _np(vl))
        r = {"v": np.zeros((B, N)), "a": np.zeros((B, N)), "t": np.zeros((B, N)) if want_t else None, "total_time": np.zeros(B) if want_t else None,
             "status": np.zeros(B, dtype=np.int32)}
        so = PoSpeedOut(*[_np(r[k]) for k in ("v", "a", "t", "total_time", "status")])
        sp = params if params is not None else default_speed_params()
        _check(lib().po_speed_batch(self._h, C.byref(sp), C.byref(si), C.byref(so)))
        return r

    def speed_batch_device(self, t: dict, out: dict, params=None):
        """Device-pointer entry: t: states [B,N,5] f64, v0 [B] f64 (+ n_states, ok i32, v_end [B], v_limit [B,N]); out: v, a [B,N] f64, status [B] i32 (+ t [B,N],
        total_time [B]).  Enqueued on the handle's stream, no synchronisation."""
        from .abi import PoSpeedIn, PoSpeedOut

        B, N = t["states"].shape[0], t["states"].shape[1]
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        si = PoSpeedIn(B, N, p(t, "states"), p(t, "n_states"), p(t, "ok"), p(t, "v0"), p(t, "v_end"), p(t, "v_limit"))
        so = PoSpeedOut(*[p(out, k) for k in ("v", "a", "t", "total_time", "status")])
        sp = params if params is not None else default_speed_params()
        _check(lib().po_speed_batch_device(self._h, C.byref(sp), C.byref(si), C.byref(so)))

    # ---- moving obstacles: timed paths against predicted agents ----
    DYNAMIC_KEYS = ("status", "ok_out", "gap_min", "first_state", "first_agent", "stop_state", "first_time", "gap", "v_limit")

    def dynamic_batch(self, states, t, agents, n_states=None, ok=None, set_of=None, v_limit_in=None, params=None, want_rows=True):
        """Host-pointer entry of po_dynamic_batch.  states [B,N,5], t [B,N] (speed_batch's t), agents: what pack_agents takes; optional n_states [B], ok [B],
        set_of [B] (None: set 0), v_limit_in [B,N].  Returns a dict: status, ok_out, first_state, first_agent, stop_state [B] i32, gap_min, first_time [B], gap and
        v_limit [B,N] (None without want_rows)."""
        from .abi import PoDynamicIn, PoDynamicOut

        states = np.ascontiguousarray(states, dtype=np.float64)
        B, N = states.shape[0], states.shape[1]
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        tt, vin = f(t), f(v_limit_in)
        ns, okk, so = _i32(n_states), _i32(ok), _i32(set_of)
        lists, ag, first = _agent_lists(agents)
        di = PoDynamicIn(B, N, _np(states), _np(ns), _np(okk), _np(tt), _np(so), C.pointer(lists), _np(vin))
        i32 = lambda: np.zeros(B, dtype=np.int32)
        r = {"status": i32(), "ok_out": i32(), "gap_min": np.zeros(B), "first_state": i32(), "first_agent": i32(), "stop_state": i32(), "first_time": np.zeros(B),
             "gap": np.zeros((B, N)) if want_rows else None, "v_limit": np.zeros((B, N)) if want_rows else None}
        do = PoDynamicOut(*[_np(r[k]) for k in self.DYNAMIC_KEYS])
        dp = params if params is not None else default_dynamic_params()
        _check(lib().po_dynamic_batch(self._h, C.byref(dp), C.byref(di), C.byref(do)))
        return r

    def dynamic_batch_device(self, t: dict, out: dict, params=None):
        """Device-pointer entry: t: states [B,N,5] f64, t [B,N] f64, agents (a uint8 tensor over AGENT_DTYPE records, or None when there are none), first [S+1] i32
        (+ n_states, ok, set_of i32 [B], v_limit_in [B,N]); out: status [B] i32 (+ any of DYNAMIC_KEYS).  Enqueued on the handle's stream, no synchronisation."""
        from .abi import PoDynamicIn, PoDynamicOut

        B, N = t["states"].shape[0], t["states"].shape[1]
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        lists = _agent_lists_device(t)
        di = PoDynamicIn(B, N, p(t, "states"), p(t, "n_states"), p(t, "ok"), p(t, "t"), p(t, "set_of"), C.pointer(lists), p(t, "v_limit_in"))
        do = PoDynamicOut(*[p(out, k) for k in self.DYNAMIC_KEYS])
        dp = params if params is not None else default_dynamic_params()
        _check(lib().po_dynamic_batch_device(self._h, C.byref(dp), C.byref(di), C.byref(do)))

    # ---- station-time speed planning: pass or yield around predicted agents ----
    STPLAN_KEYS = ("status", "ok_out", "n_layers", "cost", "station", "cells", "v_limit")

    def stplan_batch(self, states, v0, agents, n_states=None, ok=None, v_cap=None, set_of=None, v_limit_in=None, params=None, want_rows=True):
        """Host-pointer entry of po_stplan_batch.  states [B,N,5], v0 [B], agents: what pack_agents takes; optional n_states [B], ok [B], v_cap [B,N], set_of [B]
        (None: set 0), v_limit_in [B,N].  Returns a dict: status, ok_out, n_layers [B] i32, cost [B], station [B,17] i32, cells [B,K,128] i32 and v_limit [B,N]
        (the last two None without want_rows)."""
        from .abi import PO_ST_MAX_LAYERS, PO_ST_MAX_STATIONS, PoStplanIn, PoStplanOut

        states = np.ascontiguousarray(states, dtype=np.float64)
        B, N = states.shape[0], states.shape[1]
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        vv, cap, vin = f(v0), f(v_cap), f(v_limit_in)
        ns, okk, so = _i32(n_states), _i32(ok), _i32(set_of)
        lists, ag, first = _agent_lists(agents)
        si = PoStplanIn(B, N, _np(states), _np(ns), _np(okk), _np(vv), _np(cap), _np(so), C.pointer(lists), _np(vin))
        sp = params if params is not None else default_stplan_params()
        i32 = lambda *shape: np.zeros(shape, dtype=np.int32)
        r = {"status": i32(B), "ok_out": i32(B), "n_layers": i32(B), "cost": np.zeros(B), "station": i32(B, PO_ST_MAX_LAYERS + 1),
             "cells": i32(B, max(int(sp.K), 0), PO_ST_MAX_STATIONS) if want_rows else None, "v_limit": np.zeros((B, N)) if want_rows else None}
        so_ = PoStplanOut(*[_np(r[k]) for k in self.STPLAN_KEYS])
        _check(lib().po_stplan_batch(self._h, C.byref(sp), C.byref(si), C.byref(so_)))
        return r

    def stplan_batch_device(self, t: dict, out: dict, params=None):
        """Device-pointer entry: t: states [B,N,5] f64, v0 [B] f64, agents (a uint8 tensor over AGENT_DTYPE records, or None when there are none), first [S+1] i32
        (+ n_states, ok, set_of i32 [B], v_cap, v_limit_in [B,N]); out: status [B] i32 (+ any of STPLAN_KEYS: station [B,17] i32, cells [B,K,128] i32).  Enqueued on
        the handle's stream, no synchronisation."""
        from .abi import PoStplanIn, PoStplanOut

        B, N = t["states"].shape[0], t["states"].shape[1]
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        lists = _agent_lists_device(t)
        si = PoStplanIn(B, N, p(t, "states"), p(t, "n_states"), p(t, "ok"), p(t, "v0"), p(t, "v_cap"), p(t, "set_of"), C.pointer(lists), p(t, "v_limit_in"))
        so = PoStplanOut(*[p(out, k) for k in self.STPLAN_KEYS])
        sp = params if params is not None else default_stplan_params()
        _check(lib().po_stplan_batch_device(self._h, C.byref(sp), C.byref(si), C.byref(so)))

    # ---- stop, wait, go: station-time plans that resume, sampled in time ----
    STGO_KEYS = ("status", "ok_out", "n_layers", "cost", "station", "cells", "n_resumes", "states", "v", "a", "t", "index", "first_held", "end")

    def stgo_batch(self, states, v0, agents, n_states=None, ok=None, v_cap=None, set_of=None, params=None, want_rows=True):
        """Host-pointer entry of po_stgo_batch.  states [B,N,5], v0 [B], agents: what pack_agents takes; optional n_states [B], ok [B], v_cap [B,N], set_of [B]
        (None: set 0).  Returns a dict: status, ok_out, n_layers, n_resumes, first_held, end [B] i32, cost [B], station [B,17] i32, cells [B,K,128] i32 (None
        without want_rows), and the samples: states [B,Q,5], v, a, t [B,Q], index [B,Q] i32 (what dynamic_batch and trajectory_batch read)."""
        from .abi import PO_ST_MAX_LAYERS, PO_ST_MAX_STATIONS, PoStgoIn, PoStgoOut

        states = np.ascontiguousarray(states, dtype=np.float64)
        B, N = states.shape[0], states.shape[1]
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        vv, cap = f(v0), f(v_cap)
        ns, okk, so = _i32(n_states), _i32(ok), _i32(set_of)
        lists, ag, first = _agent_lists(agents)
        gi = PoStgoIn(B, N, _np(states), _np(ns), _np(okk), _np(vv), _np(cap), _np(so), C.pointer(lists))
        gp = params if params is not None else default_stgo_params()
        K, Q = max(int(gp.K), 0), max(int(gp.Q), 0)
        i32 = lambda *shape: np.zeros(shape, dtype=np.int32)
        r = {"status": i32(B), "ok_out": i32(B), "n_layers": i32(B), "cost": np.zeros(B), "station": i32(B, PO_ST_MAX_LAYERS + 1),
             "cells": i32(B, K, PO_ST_MAX_STATIONS) if want_rows else None, "n_resumes": i32(B), "states": np.zeros((B, Q, 5)), "v": np.zeros((B, Q)),
             "a": np.zeros((B, Q)), "t": np.zeros((B, Q)), "index": i32(B, Q), "first_held": i32(B), "end": i32(B)}
        go = PoStgoOut(*[_np(r[k]) for k in self.STGO_KEYS])
        _check(lib().po_stgo_batch(self._h, C.byref(gp), C.byref(gi), C.byref(go)))
        return r

    def stgo_batch_device(self, t: dict, out: dict, params=None):
        """Device-pointer entry: t: states [B,N,5] f64, v0 [B] f64, agents (a uint8 tensor over AGENT_DTYPE records, or None when there are none), first [S+1] i32
        (+ n_states, ok, set_of i32 [B], v_cap [B,N]); out: status [B] i32, states [B,Q,5] f64 (+ any of STGO_KEYS: station [B,17] i32, cells [B,K,128] i32,
        v, a, t [B,Q] f64, index [B,Q] i32).  Q is params.Q.  Enqueued on the handle's stream, no synchronisation."""
        from .abi import PoStgoIn, PoStgoOut

        B, N = t["states"].shape[0], t["states"].shape[1]
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        lists = _agent_lists_device(t)
        gi = PoStgoIn(B, N, p(t, "states"), p(t, "n_states"), p(t, "ok"), p(t, "v0"), p(t, "v_cap"), p(t, "set_of"), C.pointer(lists))
        go = PoStgoOut(*[p(out, k) for k in self.STGO_KEYS])
        gp = params if params is not None else default_stgo_params()
        _check(lib().po_stgo_batch_device(self._h, C.byref(gp), C.byref(gi), C.byref(go)))

    # ---- speed QP: a jerk-limited s(t) inside a station-time plan's free tunnel ----
    SPEEDQP_KEYS = ("status", "iters", "n_fact", "r_prim", "r_dual", "n_q", "states", "v", "a", "jerk", "t", "lo", "hi", "index")
    SPEEDQP_IN_KEYS = ("states", "n_states", "ok", "v0", "v_cap", "station", "n_layers", "cells", "ref_states")

    def speedqp_batch(self, states, v0, station, n_layers, ref_states, n_states=None, ok=None, v_cap=None, cells=None, params=None):
        """Host-pointer entry of po_speedqp_batch.  states [B,N,5], v0 [B], and the plan as stgo_batch / stplan_batch return it: station [B,17] i32, n_layers [B] i32,
        ref_states [B,Q,5] (the planner's samples at the same dts and Q, t0 = 0); optional n_states [B], ok [B] (the planner's ok_out), v_cap [B,N], cells
        [B,K,128] i32 (None: nothing is blocked).  Returns a dict: status, iters, n_fact, n_q [B] i32, r_prim, r_dual [B], states [B,Q,5], v, a, jerk, t, lo, hi
        [B,Q], index [B,Q] i32."""
        from .abi import PoSpeedqpIn, PoSpeedqpOut

        states = np.ascontiguousarray(states, dtype=np.float64)
        B, N = states.shape[0], states.shape[1]
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        vv, cap, ref = f(v0), f(v_cap), f(ref_states)
        ns, okk, stn, nl, cl = _i32(n_states), _i32(ok), _i32(station), _i32(n_layers), _i32(cells)
        qi = PoSpeedqpIn(B, N, _np(states), _np(ns), _np(okk), _np(vv), _np(cap), _np(stn), _np(nl), _np(cl), _np(ref))
        qp = params if params is not None else default_speedqp_params()
        Q = max(int(qp.Q), 0)
        i32 = lambda *shape: np.zeros(shape, dtype=np.int32)
        r = {"status": i32(B), "iters": i32(B), "n_fact": i32(B), "r_prim": np.zeros(B), "r_dual": np.zeros(B), "n_q": i32(B), "states": np.zeros((B, Q, 5)),
             "v": np.zeros((B, Q)), "a": np.zeros((B, Q)), "jerk": np.zeros((B, Q)), "t": np.zeros((B, Q)), "lo": np.zeros((B, Q)), "hi": np.zeros((B, Q)),
             "index": i32(B, Q)}
        qo = PoSpeedqpOut(*[_np(r[k]) for k in self.SPEEDQP_KEYS])
        _check(lib().po_speedqp_batch(self._h, C.byref(qp), C.byref(qi), C.byref(qo)))
        return r

    def speedqp_batch_device(self, t: dict, out: dict, params=None):
        """Device-pointer entry: t: states [B,N,5] f64, v0 [B] f64, station [B,17] i32, n_layers [B] i32, ref_states [B,Q,5] f64 (+ n_states, ok i32 [B], v_cap
        [B,N] f64, cells [B,K,128] i32); out: status [B] i32, states [B,Q,5] f64 (+ any of SPEEDQP_KEYS).  Q is params.Q.  Enqueued on the handle's stream, no
        synchronisation."""
        from .abi import PoSpeedqpIn, PoSpeedqpOut

        B, N = t["states"].shape[0], t["states"].shape[1]
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        qi = PoSpeedqpIn(B, N, *[p(t, k) for k in self.SPEEDQP_IN_KEYS])
        qo = PoSpeedqpOut(*[p(out, k) for k in self.SPEEDQP_KEYS])
        qp = params if params is not None else default_speedqp_params()
        _check(lib().po_speedqp_batch_device(self._h, C.byref(qp), C.byref(qi), C.byref(qo)))

    # ---- corridor nudge: carve predicted agents out of the corridor bounds, pass left or right ----
    NUDGE_KEYS = ("status", "ok_out", "bounds", "side", "first_blocked_state", "first_blocked_agent", "width_min")

    def nudge_batch(self, ref_x, ref_y, ref_z, t, bounds, agents, n_points=None, ok=None, set_of=None, side_prev=None, W=None, params=None):
        """Host-pointer entry of po_nudge_batch.  ref_x, ref_y, ref_z, t [B,N], bounds [B,N,4,2] (bounds_batch's), agents: what pack_agents takes; optional
        n_points [B], ok [B], set_of [B] (None: set 0), side_prev [B,W] (the side of the last call).  W: columns of side (None: side_prev's, else the largest
        set, at least 1).  Returns a dict: status, ok_out, first_blocked_state, first_blocked_agent [B] i32, bounds [B,N,4,2] (solve_batch's), side [B,W] i32,
        width_min [B]."""
        from .abi import PoNudgeIn, PoNudgeOut

        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        rx, ry, rz, tt, bnd = f(ref_x), f(ref_y), f(ref_z), f(t), f(bounds)
        B, N = rx.shape[0], rx.shape[1]
        ns, okk, so, sp_ = _i32(n_points), _i32(ok), _i32(set_of), _i32(side_prev)
        lists, ag, first = _agent_lists(agents)
        if W is None:
            W = sp_.shape[1] if sp_ is not None else max(1, int(np.diff(first).max()) if len(first) > 1 else 1)
        ni = PoNudgeIn(B, N, W, _np(rx), _np(ry), _np(rz), _np(ns), _np(okk), _np(tt), _np(bnd), _np(so), C.pointer(lists), _np(sp_))
        i32 = lambda *shape: np.zeros(shape, dtype=np.int32)
        r = {"status": i32(B), "ok_out": i32(B), "bounds": np.zeros((B, N, 4, 2)), "side": i32(B, W) if W > 0 else None, "first_blocked_state": i32(B),
             "first_blocked_agent": i32(B), "width_min": np.zeros(B)}
        no = PoNudgeOut(*[_np(r[k]) for k in self.NUDGE_KEYS])
        npar = params if params is not None else default_nudge_params()
        _check(lib().po_nudge_batch(self._h, C.byref(npar), C.byref(ni), C.byref(no)))
        return r

    def nudge_batch_device(self, t: dict, out: dict, params=None):
        """Device-pointer entry: t: ref_x, ref_y, ref_z, t [B,N] f64, bounds [B,N,4,2] f64, agents (a uint8 tensor over AGENT_DTYPE records, or None when there
        are none), first [S+1] i32 (+ n_points, ok, set_of i32 [B], side_prev [B,W] i32); out: status [B] i32, bounds [B,N,4,2] f64 (+ any of NUDGE_KEYS: side
        [B,W] i32).  W is the second dimension of side or side_prev (0 without both).  Enqueued on the handle's stream, no synchronisation."""
        from .abi import PoNudgeIn, PoNudgeOut

        B, N = t["ref_x"].shape[0], t["ref_x"].shape[1]
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        wide = out.get("side") if out.get("side") is not None else t.get("side_prev")
        W = 0 if wide is None else wide.shape[1]
        lists = _agent_lists_device(t)
        ni = PoNudgeIn(B, N, W, p(t, "ref_x"), p(t, "ref_y"), p(t, "ref_z"), p(t, "n_points"), p(t, "ok"), p(t, "t"), p(t, "bounds"), p(t, "set_of"),
                       C.pointer(lists), p(t, "side_prev"))
        no = PoNudgeOut(*[p(out, k) for k in self.NUDGE_KEYS])
        npar = params if params is not None else default_nudge_params()
        _check(lib().po_nudge_batch_device(self._h, C.byref(npar), C.byref(ni), C.byref(no)))

    # ---- timed trajectory: speed-profiled paths sampled at uniform time steps, and as agents ----
    TRAJECTORY_KEYS = ("status", "states", "v", "a", "t", "index", "first_held", "agents")

    def trajectory_batch(self, states, v, t, n_states=None, ok=None, params=None):
        """Host-pointer entry of po_trajectory_batch.  states [B,N,5], v, t [B,N] (speed_batch's); optional n_states [B], ok [B].  Returns a dict: status,
        first_held [B] i32, states [B,K,5], v, a, t [B,K], index [B,K] i32 and agents [B * n_discs] of AGENT_DTYPE (None with n_discs = 0): path b, disc d at
        b * n_discs + d, what pack_agents passes through as (agents, first)."""
        from .abi import PoTrajectoryIn, PoTrajectoryOut

        states = np.ascontiguousarray(states, dtype=np.float64)
        B, N = states.shape[0], states.shape[1]
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        vv, tt = f(v), f(t)
        ns, okk = _i32(n_states), _i32(ok)
        tp = params if params is not None else default_trajectory_params()
        K, D = max(int(tp.K), 0), max(int(tp.n_discs), 0)
        ti = PoTrajectoryIn(B, N, _np(states), _np(ns), _np(okk), _np(vv), _np(tt))
        i32 = lambda *shape: np.zeros(shape, dtype=np.int32)
        r = {"status": i32(B), "states": np.zeros((B, K, 5)), "v": np.zeros((B, K)), "a": np.zeros((B, K)), "t": np.zeros((B, K)), "index": i32(B, K),
             "first_held": i32(B), "agents": np.zeros(B * D, dtype=AGENT_DTYPE) if D > 0 else None}
        to = PoTrajectoryOut(*[_np(r[k]) for k in self.TRAJECTORY_KEYS])
        _check(lib().po_trajectory_batch(self._h, C.byref(tp), C.byref(ti), C.byref(to)))
        return r

    def trajectory_batch_device(self, t: dict, out: dict, params=None):
        """Device-pointer entry: t: states [B,N,5], v, t [B,N] f64 (+ n_states, ok i32 [B]); out: status [B] i32, states [B,K,5] f64 (+ any of TRAJECTORY_KEYS:
        v, a, t [B,K] f64, index [B,K] i32, first_held [B] i32, agents: a uint8 tensor over B * n_discs AGENT_DTYPE records, which dynamic_batch_device,
        stplan_batch_device and nudge_batch_device take as their agents).  Enqueued on the handle's stream, no synchronisation."""
        from .abi import PoTrajectoryIn, PoTrajectoryOut

        B, N = t["states"].shape[0], t["states"].shape[1]
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        ti = PoTrajectoryIn(B, N, p(t, "states"), p(t, "n_states"), p(t, "ok"), p(t, "v"), p(t, "t"))
        to = PoTrajectoryOut(*[p(out, k) for k in self.TRAJECTORY_KEYS])
        tp = params if params is not None else default_trajectory_params()
        _check(lib().po_trajectory_batch_device(self._h, C.byref(tp), C.byref(ti), C.byref(to)))

    # ---- agent sets: per ego path, the agents that can matter to it ----
    AGENTSETS_KEYS = ("agents", "first", "count", "status", "set_of", "src_index", "total")

    def agentsets_batch(self, states, t, sources, pool_of=None, owner=None, capacity=None, params=None, n_states=None, ok=None):
        """Host-pointer entry of po_agentsets_batch.  states [B,N,5], t [B,N] or None (the window of params), sources: one or two of what pack_agents takes (the
        fleet in pools, then perception in pools); optional pool_of [B], owner [n_agents of source 0], n_states, ok [B].  capacity None: one counting call with
        capacity 0, then a call with room for `total` records.  Returns a dict: agents [capacity] of AGENT_DTYPE, first [B + 1], count, status, set_of [B] i32,
        src_index [capacity] i32, total (int), capacity; (agents, first) is what pack_agents passes through and set_of what the consumers take."""
        from .abi import PoAgentsetsIn, PoAgentsetsOut

        states = np.ascontiguousarray(states, dtype=np.float64)
        B, N = states.shape[0], states.shape[1]
        tt = None if t is None else np.ascontiguousarray(t, dtype=np.float64)
        ns, okk, pool, own = _i32(n_states), _i32(ok), _i32(pool_of), _i32(owner)
        if not 1 <= len(sources) <= 2:
            raise ValueError("sources: the fleet's lists, then optionally perception's")
        held = [_agent_lists(s) for s in sources]  # (struct, agents, first): the arrays live until the C calls have returned
        src = (C.POINTER(type(held[0][0])) * 2)(C.pointer(held[0][0]), C.pointer(held[1][0]) if len(held) > 1 else None)
        ai = PoAgentsetsIn(B, N, _np(states), _np(ns), _np(okk), _np(tt), src, _np(pool), _np(own))
        ap = params if params is not None else default_agentsets_params()
        i32 = lambda n: np.zeros(n, dtype=np.int32)

        def call(cap):
            r = {"agents": np.zeros(cap, dtype=AGENT_DTYPE), "first": i32(B + 1), "count": i32(B), "status": i32(B), "set_of": i32(B), "src_index": i32(cap),
                 "total": np.zeros(1, dtype=np.int64)}
            ao = PoAgentsetsOut(cap, *[_np(r[k]) if len(r[k]) else None for k in self.AGENTSETS_KEYS])
            _check(lib().po_agentsets_batch(self._h, C.byref(ap), C.byref(ai), C.byref(ao)))
            return r

        if capacity is None:
            capacity = int(call(0)["total"][0])
            if capacity >= 2 ** 31:
                raise PoError(f"agentsets_batch: {capacity} records do not fit one call")
        r = call(int(capacity))
        r["total"], r["capacity"] = int(r["total"][0]), int(capacity)
        return r

    def agentsets_batch_device(self, t: dict, out: dict, params=None):
        """Device-pointer entry: t: states [B,N,5] f64, agents (a uint8 tensor over AGENT_DTYPE records, or None) and first [S+1] i32 of the fleet (+ t [B,N] f64,
        n_states, ok, pool_of i32 [B], owner i32 [n_agents], and agents1 / first1: the perception list); out: agents (a uint8 tensor over `capacity` records;
        None: capacity 0, the counting call), first [B+1], count, status [B] i32 (+ set_of [B] i32, src_index [capacity] i32, total [1] i64).  out's agents,
        first and set_of are what dynamic_batch_device, stplan_batch_device and nudge_batch_device take.  Enqueued on the handle's stream, no synchronisation."""
        from .abi import PoAgentLists, PoAgentsetsIn, PoAgentsetsOut

        B, N = t["states"].shape[0], t["states"].shape[1]
        p = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
        l0 = _agent_lists_device(t)
        l1 = _agent_lists_device({"agents": t.get("agents1"), "first": t["first1"]}) if t.get("first1") is not None else None
        src = (C.POINTER(PoAgentLists) * 2)(C.pointer(l0), C.pointer(l1) if l1 is not None else None)
        ai = PoAgentsetsIn(B, N, p(t, "states"), p(t, "n_states"), p(t, "ok"), p(t, "t"), src, p(t, "pool_of"), p(t, "owner"))
        ag = out.get("agents")
        cap = 0 if ag is None else ag.numel() * ag.element_size() // AGENT_DTYPE.itemsize
        ao = PoAgentsetsOut(cap, *[p(out, k) for k in self.AGENTSETS_KEYS])
        ap = params if params is not None else default_agentsets_params()
        _check(lib().po_agentsets_batch_device(self._h, C.byref(ap), C.byref(ai), C.byref(ao)))

    def map_sample(self, xy):
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        d = np.zeros(len(xy)); ins = np.zeros(len(xy), dtype=np.int32)
        _check(lib().po_map_sample(self._h, len(xy), _np(xy), _np(d), _np(ins)))
        return d, ins

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _check(lib().po_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_phase_ms(self) -> dict:
        """po_last_phase_ms: where the last solve spent its time (host-pointer entry: pack + H2D / solve / D2H / host pack / host unpack; split scheduling: the solve's own phases)."""
        ms = (C.c_float * 8)()
        _check(lib().po_last_phase_ms(self._h, ms))
        keys = ("pack_h2d", "solve", "d2h", "host_pack", "host_unpack", "warm_start", "newton", "fallback")
        return {k: float(ms[i]) for i, k in enumerate(keys)}


class DeviceBatch:
    """A synth.Batch uploaded once into HBM as torch tensors (torch is only the allocator here)."""

    def __init__(self, batch, device="cuda:0", want_x=False):
        import torch

        self.formulation, self.B, self.N, self.keep = batch.formulation, batch.B, batch.N, batch.keep
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.ref_x, self.ref_y, self.ref_z, self.ref_k, self.ref_s = map(up, (batch.ref_x, batch.ref_y, batch.ref_z, batch.ref_k, batch.ref_s))
        self.bounds, self.x0, self.goal_z, self.max_k, self.max_kp = map(up, (batch.bounds, batch.x0, batch.goal_z, batch.max_k, batch.max_kp))
        npts = getattr(batch, 'n_points', None)
        self.n_points = None if npts is None else torch.from_numpy(np.ascontiguousarray(npts, dtype=np.int32)).to(device)
        n, _, _ = problem_dims(batch.formulation, batch.N, batch.keep)
        self.out_states = torch.zeros((batch.B, batch.N, 5), dtype=torch.float64, device=device)
        self.out_info = torch.zeros((batch.B, INFO_BYTES), dtype=torch.uint8, device=device)  # sizeof(po_info)
        self.out_x = torch.zeros((batch.B, n), dtype=torch.float64, device=device) if want_x else None
        self.order = None  # optional int32 [B] device tensor: scheduling hint (po_batch_in.order), see set_order()

    def set_order(self, order):
        """Scheduling hint for the next solves of this batch: a permutation of range(B), e.g. np.argsort(-previous_info["iters"], kind="stable")
        (longest path first).  None: the engine's own mixing."""
        import torch

        self.order = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(self.out_states.device)

    def clone_outputs(self):
        """Same (shared, read-only) inputs, fresh output buffers: lets several handles solve the batch concurrently."""
        import copy

        import torch

        d = copy.copy(self)
        d.out_states = torch.zeros_like(self.out_states)
        d.out_info = torch.zeros_like(self.out_info)
        d.out_x = None if self.out_x is None else torch.zeros_like(self.out_x)
        return d

    def info_numpy(self):
        return self.out_info.cpu().numpy().view(INFO_DTYPE).reshape(-1)
