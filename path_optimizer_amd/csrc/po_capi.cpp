// po_capi.cpp — the C ABI of libpo_hip.so (include/po_hip.h): handle management, host<->device staging,
// kernel launches (the solve entries: po_solve.cpp; the plan chain: po_plan.cpp).  No torch types, no oracle, no CPU fallback: every entry point that computes runs the HIP
// kernels or returns an error code.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/po_hip.h"
#include "po_handle.hpp"
#include "po_launch.hpp"
#include "po_list_check.hpp"
#include "po_map.hpp"
#include "po_smooth.hpp"

static thread_local std::string g_hip_err;

bool hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    g_hip_err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

extern "C" {

void po_default_params(po_params *p) {
    if (!p) return;
    // car geometry and weights: /root/reference/src/config/planning_flags.cpp:8-14,18-43,102-119
    const double car_length = 4.9, rear_axle_to_center = 1.45;
    std::memset(p, 0, sizeof(*p));
    p->d[0] = -3.0 / 8.0 * car_length + rear_axle_to_center;
    p->d[1] = -1.0 / 8.0 * car_length + rear_axle_to_center;
    p->d[2] = 1.0 / 8.0 * car_length + rear_axle_to_center;
    p->d[3] = 3.0 / 8.0 * car_length + rear_axle_to_center;
    p->w_curv = 10; p->w_curv_rate = 200; p->w_dev = 0; p->w_slack = 3;
    p->k_w_curv = 50; p->k_w_curv_rate = 200; p->k_w_dev = 0;
    p->w_k_slack = 500; p->w_kp_slack = 25000;
    p->margin = 1.3;
    p->max_steer = 30.0 * M_PI / 180.0;
    p->wheel_base = 2.85;
    p->enable_collision_check = 1;
    p->car_width = 2.0; p->car_length = 4.9; p->rear_axle_to_center = 1.45; p->safety_margin = 0.0;  /* planning_flags.cpp:18-29 */
    p->constraint_end_heading = 1;
    p->scaling = 10;  // OSQP default (the reference leaves it untouched)
    p->eps_abs = 1e-4; p->eps_rel = 1e-4; p->eps_prim_inf = 1e-4; p->eps_dual_inf = 1e-4;
    p->rho0 = 0.1; p->sigma = 1e-6; p->alpha = 1.6; p->adapt_tol = 5.0;
    p->max_iter = 4000; p->check_every = 25; p->adapt_every = 100;
    // reference-smoothing QPs, planning_flags.cpp:76-86
    p->t2_w_dev = 0.005; p->t2_w_curv = 1; p->t2_w_curv_rate = 10;
    p->cart_w_curv = 1; p->cart_w_curv_rate = 50; p->cart_w_dev = 0.0;
    /* planning_flags.cpp:41-43,57-63,137 */
    p->mu = 0.4; p->max_curvature_rate = 0.1; p->search_lateral_range = 10.0; p->search_long_spacing = 1.5; p->search_lat_spacing = 0.6;
    p->enable_dynamic_segmentation = 1;
    p->enable_raw_output = 1; p->output_spacing = 0.3; /* planning_flags.cpp:127-129 */
    p->polish = 0; p->polish_delta = 1e-6; p->polish_refine_iter = 3;  /* OSQP defaults (polish off) */
    p->refine = 0; p->refine_eps = 1e-7; p->refine_rounds = 1; p->refine_chain = 2; p->refine_extra_rounds = 0;
    p->refine_newton_rho = 100.0; p->refine_newton_rho_eq = 1e4; p->refine_newton_rho_max = 1e5; p->refine_ls_tol = 0.6; p->refine_ls_max = 30; p->refine_newton_max = 300; p->refine_newton_final = 3; p->refine_newton_escalate = 12; p->refine_newton_rho_eq_max = 1e6; /* refine = 2 */
}

int po_problem_dims(int form, int N, int keep, int *n, int *m, int *C) {
    if (N < 2) return PO_ERR_INVALID;
    int c, nn, mm;
    if (form == PO_KP) {  // solver_kp_as_input.cpp:13-24
        if (keep < 1) return PO_ERR_INVALID;
        c = (N + keep - 2) / keep; nn = 5 * N + c; mm = 11 * N + c + 2;
    } else if (form == PO_KPC) {  // solver_kp_as_input_constrained.cpp:13-24
        if (keep != 4) return PO_ERR_INVALID;
        c = (N + keep - 2) / keep; nn = 6 * N + c; mm = 12 * N + 3 * c + 2;
    } else if (form == PO_K) {  // solver_k_as_input.cpp:14-20
        c = N - 1; nn = 4 * N - 1; mm = 11 * N - 1;
    } else {
        return PO_ERR_INVALID;
    }
    if (n) *n = nn;
    if (m) *m = mm;
    if (C) *C = c;
    return PO_OK;
}

int po_keep_control_steps(int form, const double *ref_s, int N) {
    if (!ref_s || N < 2) return PO_ERR_INVALID;
    if (form == PO_KPC) return 4;
    if (form == PO_K) return 1;
    if (form != PO_KP) return PO_ERR_INVALID;
    double interval = 0;  // solver.cpp:19,22-27
    for (int i = 1; i < N && i < 10; ++i) interval = std::fmax(interval, ref_s[i] - ref_s[i - 1]);
    const double q = 1.2 / interval;  // solver_kp_as_input.cpp:17 (truncating cast)
    const int k = (q >= 2147483647.0 || q != q) ? 1 : static_cast<int>(q);
    return k > 1 ? k : 1;
}

// Several engines in ONE process (OsqpSolver::solveBatch(..., engines), one host thread + handle + stream each): the HIP runtime maps a process's streams onto a pool of
// GPU_MAX_HW_QUEUES hardware queues (default 4), and streams that share a hardware queue run their kernels one after the other — measured on one MI355X with E engines
// solving 64-path batches side by side (tools/engines_procs.py, round 6): per call 1.21 / 1.22 / 1.82 / 4.24 ms for E = 1 / 2 / 4 / 8 with the default pool, 1.23 / 2.39 /
// 4.77 / 7.16 with a pool of 2, 1.22 / 1.23 / 1.36 / 1.53 with a pool of 16; E PROCESSES (a pool each): 1.22 / 1.46 / 1.66 / 1.88.  The pool size is read once, when the
// runtime starts; so, BEFORE this library's first HIP call, the variable is set to 16 unless the caller has set it (overwrite = 0; a process whose runtime is already up —
// e.g. one that imported torch first — keeps what it started with: export GPU_MAX_HW_QUEUES there).
static void runtime_prepare() {
    static std::once_flag once;
    std::call_once(once, [] { setenv("GPU_MAX_HW_QUEUES", "16", 0); });
}

int po_device_count(void) {
    runtime_prepare();
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int po_create(int device, const po_params *params, po_handle *out) {
    if (!params || !out) return PO_ERR_INVALID;
    if (params->scaling < 0 || params->scaling > 100) return PO_ERR_INVALID;
    if (params->refine != 0 && params->refine != 2) return PO_ERR_INVALID;  // (refine = 1 was removed with ABI 5, include/po_hip.h)
    // the rounds of the refinement (refine_rounds regular ones + refine_extra_rounds below eps) are counted in 5 bits of the hand-back status: 32 or more used to switch the
    // refinement off silently — refused here instead
    if (params->refine == 2 && (params->refine_rounds > 1 ? params->refine_rounds : 1) + (params->refine_extra_rounds > 0 ? params->refine_extra_rounds : 0) >= 32) return PO_ERR_INVALID;
    runtime_prepare();
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return PO_ERR_INVALID;
    HIP_TRY(hipSetDevice(device));
    po_handle_s *h = new (std::nothrow) po_handle_s;
    if (!h) return PO_ERR_NOMEM;
    h->device = device;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->wave_slots = 4 * cus; }
    h->params = *params;
    if (!hip_ok(hipStreamCreateWithFlags(&h->own_stream.s, hipStreamNonBlocking), "hipStreamCreate") ||
        !hip_ok(hipEventCreate(&h->ev0.e), "hipEventCreate") || !hip_ok(hipEventCreate(&h->ev1.e), "hipEventCreate")) {
        delete h;  // (the handle destroys what had been created)
        return PO_ERR_HIP;
    }
    for (Event &e : h->evh) if (!hip_ok(hipEventCreate(&e.e), "hipEventCreate")) { delete h; return PO_ERR_HIP; }
    for (Event &e : h->evp) if (!hip_ok(hipEventCreate(&e.e), "hipEventCreate")) { delete h; return PO_ERR_HIP; }
    {
        Lock g(h->mu);
        h->stream = h->own_stream.s;
    }
    *out = h;
    return PO_OK;
}

int po_destroy(po_handle h) {
    if (!h) return PO_ERR_INVALID;
    (void)hipSetDevice(h->device);
    {
        Lock g(h->mu);
        (void)hipStreamSynchronize(h->stream);
    }
    delete h;  // buffers, then events, then the stream (po_handle_s, po_handle.hpp)
    return PO_OK;
}

int po_debug_set(po_handle h, const char *key, int value) {
    if (!h || !key) return PO_ERR_INVALID;
    Lock g(h->mu);
    const std::string k(key);
    if (k == "identity_order") h->env_identity = value != 0;
    else if (k == "host_threads") h->host_threads = value < 0 ? 0 : value;
    else if (k == "debug_cycles") h->env_cycles = value != 0;
    else if (k == "newton_slice") { h->nw_slice = value > 0 ? (int)value : 0; h->nw_slice_forced = value > 0; }  // (set explicitly: also on batches the engine would not slice)
    else if (k == "fixed_length") h->fixed_length = value != 0;  // (0: the generic kernels also for the lengths of PO_FIXED_N; an A/B switch, the results do not depend on it)
    else if (k == "fixed_classes") h->fixed_classes = value != 0;  // (0: no constant-class Newton kernels; an A/B switch, the results do not depend on it)
    else if (k == "smooth_seq") h->env_smooth_seq = value != 0;
    else if (k == "smooth_waves") h->env_smooth_waves = value;
    else if (k == "smooth_nopad") h->env_smooth_nopad = value != 0;
    else if (k == "smooth_debug") h->env_smooth_debug = value != 0;
    else if (k == "dp_one_wave") h->env_dp_one_wave = value != 0;
    else return PO_ERR_INVALID;
    return PO_OK;
}

int po_debug_get(po_handle h, const char *key, long long *value) {
    if (!h || !key || !value) return PO_ERR_INVALID;
    const std::string k(key);
    Lock g(h->mu);
    if (k == "map_ptr") {  // where the handle's map layer lives (0: none); no device call
        *value = (long long)reinterpret_cast<uintptr_t>(h->maps.d);
        return PO_OK;
    }
    if (k == "map_layers") {  // how many layers the handle's map stack holds (0: no map); no device call
        *value = h->maps.d ? h->maps.M : 0;
        return PO_OK;
    }
    if (k == "world_cells") {  // the size of the handle's world grid (0: none); no device call
        *value = h->world.cells ? (long long)h->world.size_x * (long long)h->world.size_y : 0;
        return PO_OK;
    }
    if (k == "fixed_length_used") {  // did the last solve run the length-specialised kernels (1) or the generic ones (0)?  no device call
        *value = h->fixed_used;
        return PO_OK;
    }
    if (k == "dp_waves_used") {  // which variant the launcher picked for the handle's last DP lattice search: 8 or 1 waves per instance (0: no search yet); no device call
        *value = h->dp_waves_used;
        return PO_OK;
    }
    if (k == "smooth_variant_used") {  // which instantiation the launcher picked for the handle's last smoothing call: 100 * kind + 10 * waves per QP + WPE (0: no call yet); no device call
        *value = h->smooth_variant_used;
        return PO_OK;
    }
    if (k == "fallback_paths") {  // split scheduling of refine = 2: how many paths the last solve's Newton launch handed to the fallback launch
        *value = 0;
        if (!h->fb_buf.p) return PO_OK;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        int c = 0;
        HIP_TRY(hipMemcpy(&c, h->fb_buf.p, sizeof(int), hipMemcpyDeviceToHost));
        *value = c;
        return PO_OK;
    }
    if (k == "fixed_classes_used") {  // how many paths of the last solve the constant-class Newton kernels were given (0: it did not run them): the flags on the device, summed
        *value = 0;
        if (!h->nw_idx_buf.p || h->std_flag_at < 0 || h->std_B <= 0) return PO_OK;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        std::vector<int> flag((size_t)h->std_B);
        HIP_TRY(hipMemcpy(flag.data(), static_cast<int *>(h->nw_idx_buf.p) + h->std_flag_at, sizeof(int) * flag.size(), hipMemcpyDeviceToHost));
        for (int f : flag) *value += f != 0;
        return PO_OK;
    }
    if (k.rfind("fixed_classes_flag:", 0) == 0) {  // "fixed_classes_flag:<b>": was path b of the last solve flagged standard (1) or not (0)?  -1: it did not run the
        // constant-class kernels; a path that is none of the last solve's: PO_ERR_INVALID.  (A count hides two wrong flags that cancel: tests/test_fixed_classes_edges.py)
        const char *const num = key + sizeof("fixed_classes_flag:") - 1;
        char *end = nullptr;
        const long long b = std::strtoll(num, &end, 10);
        if (end == num || *end != '\0' || *num < '0' || *num > '9' || b < 0) return PO_ERR_INVALID;
        *value = -1;
        if (!h->nw_idx_buf.p || h->std_flag_at < 0 || h->std_B <= 0) return PO_OK;
        if (b >= h->std_B) return PO_ERR_INVALID;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        int f = 0;
        HIP_TRY(hipMemcpy(&f, static_cast<int *>(h->nw_idx_buf.p) + h->std_flag_at + b, sizeof(int), hipMemcpyDeviceToHost));
        *value = f != 0;
        return PO_OK;
    }
    if (k == "newton_parked") {  // sliced Newton launches: how many paths of the last solve went on into the second launch (-1: the last solve was not sliced)
        *value = -1;
        if (!h->nw_idx_buf.p || h->nw_last_B <= 0) return PO_OK;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        int c = 0;
        HIP_TRY(hipMemcpy(&c, static_cast<int *>(h->nw_idx_buf.p) + h->nw_last_B, sizeof(int), hipMemcpyDeviceToHost));
        *value = c;
        if (h->std_left2_at >= 0) {  // (the constant-class kernels ran: the parked paths are on two lists)
            HIP_TRY(hipMemcpy(&c, static_cast<int *>(h->nw_idx_buf.p) + h->std_left2_at, sizeof(int), hipMemcpyDeviceToHost));
            *value += c;
        }
        return PO_OK;
    }
    if (k == "newton_list_ok") {  // sliced Newton launches: is the second launch's list what nw_sort_kernel promises — every parked path exactly once, keys non-increasing, ties in path
        // order?  1 yes, 0 no, -1 the last solve was not sliced.  (The results of a solve do not depend on the list's ORDER, so only this check sees an ordering bug.)
        *value = -1;
        if (!h->nw_idx_buf.p || h->nw_last_B <= 0) return PO_OK;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        const int B = h->nw_last_B;
        // (the constant-class kernels ran: two lists, each ordered like that, which hold every parked path exactly once between them — the first only paths flagged
        // standard, the second only the others: po_list_check.hpp)
        const bool two_lists = h->std_left2_at >= 0 && h->std_flag_at >= 0;
        std::vector<int> kl(two_lists ? (size_t)h->std_flag_at + (size_t)B : 2 * (size_t)B + 1);
        HIP_TRY(hipMemcpy(kl.data(), h->nw_idx_buf.p, sizeof(int) * kl.size(), hipMemcpyDeviceToHost));
        const bool ok = po::newton_list_ok(kl.data(), kl.data() + B, two_lists ? kl.data() + h->std_left2_at : nullptr, two_lists ? kl.data() + h->std_flag_at : nullptr, B);
        *value = ok ? 1 : 0;
        return PO_OK;
    }
    return PO_ERR_INVALID;
}

int po_set_stream(po_handle h, void *hip_stream) {
    if (!h) return PO_ERR_INVALID;
    Lock g(h->mu);
    h->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream.s;
    return PO_OK;
}

// ---- post-solve step -------------------------------------------------------------------------------------------
static po::DevCar make_car(const po_params &p) {
    // CollisionChecker ctor (collision_checker.cpp:9-15) + CarGeometry::setCircles (car_geometry.cpp:38-56)
    po::DevCar c{};
    const double width = p.car_width, back = p.car_length / 2.0 - p.rear_axle_to_center, front = p.car_length / 2.0 + p.rear_axle_to_center;
    const double length = front + back;
    c.bx = (front - back) / 2.0;
    c.br = std::sqrt((length / 2) * (length / 2) + (width / 2) * (width / 2));
    const double shift = width / 4.0, small_r = std::sqrt(2 * (shift * shift));
    const double large_r = std::sqrt(width * width + ((length - width) / 2.0) * ((length - width) / 2.0)) / 2;
    const double px[4] = {-back + shift, -back + shift, front - shift, front - shift};          // rr, rl, fr, fl
    const double py[4] = {-width / 2.0 + shift, width / 2.0 - shift, -width / 2.0 + shift, width / 2.0 - shift};
    for (int i = 0; i < 4; ++i) { c.cx[i] = px[i]; c.cy[i] = py[i]; c.cr[i] = small_r; }
    c.cx[4] = c.bx + (length - width) / 4; c.cy[4] = 0; c.cr[4] = large_r;  // fm
    c.cx[5] = c.bx - (length - width) / 4; c.cy[5] = 0; c.cr[5] = large_r;  // rm
    c.enable = p.enable_collision_check;
    return c;
}

// ---- the map stack.  Every install goes through publish_stack; the single-map entries are the stack entries with M = 1. ----
// The view the kernels get, after the layers are in place.  An install that changes M drops the assignment, one with the same M keeps it.
static void publish_stack(po_handle h, int M, int sx, int sy, double res, double px, double py, bool layer_pos) PO_REQUIRES(h->mu) {
    const bool keep = h->maps.M == M && h->maps.layer_of;
    po::DevMaps s{};
    s.d = static_cast<const float *>(h->map_buf.p); s.sx = sx; s.sy = sy; s.res = res; s.px = px; s.py = py;
    s.M = M; s.stride = (size_t)sx * (size_t)sy;
    s.pos = layer_pos ? static_cast<const double *>(h->map_pos_buf.p) : nullptr;
    s.layer_of = keep ? static_cast<const int *>(h->map_assign_buf.p) : nullptr;
    s.n_assign = keep ? h->maps.n_assign : 0;
    h->maps = s;
}
// M float layers from host memory: upload, synchronise, publish
static int install_layers(po_handle h, int M, const po_map *map, const double *pos_xy) PO_REQUIRES(h->mu) {
    HIP_TRY(hipSetDevice(h->device));
    const size_t bytes = sizeof(float) * (size_t)M * (size_t)map->size_x * (size_t)map->size_y;
    if (bytes > h->map_buf.cap) h->maps.d = nullptr;  // the old layers are about to be released: no map until the new ones are in place
    if (int rc = grow_after_sync(h, h->map_buf, bytes)) return rc;
    if (pos_xy) {
        if (int rc = grow_after_sync(h, h->map_pos_buf, sizeof(double) * 2 * (size_t)M)) return rc;
        HIP_TRY(hipMemcpyAsync(h->map_pos_buf.p, pos_xy, sizeof(double) * 2 * (size_t)M, hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(hipMemcpyAsync(h->map_buf.p, map->distance, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    publish_stack(h, M, map->size_x, map->size_y, map->resolution, map->pos_x, map->pos_y, pos_xy != nullptr);
    return PO_OK;
}

int po_set_map(po_handle h, const po_map *map) {
    if (!h || !map || !map->distance || map->size_x < 1 || map->size_y < 1 || !(map->resolution > 0)) return PO_ERR_INVALID;
    Lock g(h->mu);
    return install_layers(h, 1, map, nullptr);
}

int po_set_map_stack(po_handle h, int M, const po_map *layers, const double *pos_xy) {
    if (!h || M < 1 || !layers || !layers->distance || layers->size_x < 1 || layers->size_y < 1 || !(layers->resolution > 0)) return PO_ERR_INVALID;
    if (layers->size_x > po_edt_max_side() || layers->size_y > po_edt_max_side() || M > po_edt_max_images()) return PO_ERR_UNSUPPORTED;
    Lock call(h->call_mu);
    Lock g(h->mu);
    return install_layers(h, M, layers, pos_xy);
}

int po_set_map_assignment_device(po_handle h, int n, const int *layer_of) {
    if (!h || n < 0) return PO_ERR_INVALID;
    Lock g(h->mu);
    if (n == 0 || !layer_of) {  // clear: every instance reads layer 0 again (launches already enqueued got the table by value of its address: the block stays)
        h->maps.layer_of = nullptr; h->maps.n_assign = 0;
        return PO_OK;
    }
    if (!h->maps.d) return PO_ERR_INVALID;  // no stack to assign into
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = grow_after_sync(h, h->map_assign_buf, sizeof(int) * (size_t)n)) return rc;
    HIP_TRY(hipMemcpyAsync(h->map_assign_buf.p, layer_of, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    h->maps.layer_of = static_cast<const int *>(h->map_assign_buf.p); h->maps.n_assign = n;
    return PO_OK;
}

int po_set_map_assignment(po_handle h, int n, const int *layer_of) {
    if (!h || n < 0) return PO_ERR_INVALID;
    Lock call(h->call_mu);
    Lock g(h->mu);
    if (n == 0 || !layer_of) {
        h->maps.layer_of = nullptr; h->maps.n_assign = 0;
        return PO_OK;
    }
    if (!h->maps.d) return PO_ERR_INVALID;
    for (int b = 0; b < n; ++b)
        if (layer_of[b] < 0 || layer_of[b] >= h->maps.M) return PO_ERR_INVALID;  // (nothing has been touched: the previous table stays in force)
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = grow_after_sync(h, h->map_assign_buf, sizeof(int) * (size_t)n)) {
        h->maps.layer_of = nullptr; h->maps.n_assign = 0;  // (the old block is gone)
        return rc;
    }
    // the table replaces one that enqueued launches may still read: the copy is ordered behind them on the stream, and the caller's array is free when we return
    HIP_TRY(hipMemcpyAsync(h->map_assign_buf.p, layer_of, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->maps.layer_of = static_cast<const int *>(h->map_assign_buf.p); h->maps.n_assign = n;
    return PO_OK;
}

// ---- the obstacle-distance layer from an occupancy image (po_edt.hip) ----------------------------------------------
// Argument checks of every occupancy entry, before any device call (testable without a GPU)
static int check_occupancy(po_handle h, int M, const po_occupancy *occ) {
    if (!h || M < 1 || !occ || !occ->cells || occ->size_x < 1 || occ->size_y < 1 || !(occ->resolution > 0)) return PO_ERR_INVALID;
    if (occ->size_x > po_edt_max_side() || occ->size_y > po_edt_max_side() || M > po_edt_max_images()) return PO_ERR_UNSUPPORTED;
    return PO_OK;
}

int po_distance_map_batch_device(po_handle h, int M, const po_occupancy *occ, float *distance) {
    if (int rc = check_occupancy(h, M, occ)) return rc;
    if (!distance) return PO_ERR_INVALID;
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = grow_after_sync(h, h->edt_buf, po_edt_scratch_bytes(M, occ->size_x, occ->size_y))) return rc;
    HIP_TRY(po_launch_edt(occ->cells, M, occ->size_x, occ->size_y, (float)occ->resolution, h->edt_buf.p, distance, h->stream));
    return PO_OK;
}

int po_distance_map_batch(po_handle h, int M, const po_occupancy *occ, float *distance) {
    if (int rc = check_occupancy(h, M, occ)) return rc;
    if (!distance) return PO_ERR_INVALID;
    const size_t cells = (size_t)M * (size_t)occ->size_x * (size_t)occ->size_y;
    Stage S;
    const Slot<float> d_dist = S.out(distance, cells);
    const Slot<unsigned char> d_cells = S.in(occ->cells, cells);
    return staged_call(h, S, &po_handle_s::edt_io, true, [&] {
        po_occupancy dev = *occ;
        dev.cells = d_cells;
        return po_distance_map_batch_device(h, M, &dev, d_dist);
    });
}

// M images on the device -> the handle's stack (device set): grow what has to grow, transform, publish
static int stack_from_images(po_handle h, int M, const unsigned char *cells, int sx, int sy, double res, double px, double py, const double *pos_xy)
    PO_REQUIRES(h->mu) {
    // same M and size as before: every block is large enough already — nothing is allocated, nothing waits; the transform overwrites the layers in stream order
    const size_t stack_bytes = sizeof(float) * (size_t)M * (size_t)sx * (size_t)sy;
    if (stack_bytes > h->map_buf.cap) h->maps.d = nullptr;  // the old layers are about to be released: no map until the new ones are in place
    if (int rc = grow_after_sync(h, h->map_buf, stack_bytes)) return rc;
    if (int rc = grow_after_sync(h, h->edt_buf, po_edt_scratch_bytes(M, sx, sy))) return rc;
    if (pos_xy) {
        if (int rc = grow_after_sync(h, h->map_pos_buf, sizeof(double) * 2 * (size_t)M)) return rc;
        HIP_TRY(hipMemcpyAsync(h->map_pos_buf.p, pos_xy, sizeof(double) * 2 * (size_t)M, hipMemcpyDeviceToDevice, h->stream));
    }
    HIP_TRY(po_launch_edt(cells, M, sx, sy, (float)res, h->edt_buf.p, static_cast<float *>(h->map_buf.p), h->stream));
    publish_stack(h, M, sx, sy, res, px, py, pos_xy != nullptr);
    return PO_OK;
}

int po_set_map_stack_occupancy_device(po_handle h, int M, const po_occupancy *occ, const double *pos_xy) {
    if (int rc = check_occupancy(h, M, occ)) return rc;
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    return stack_from_images(h, M, occ->cells, occ->size_x, occ->size_y, occ->resolution, occ->pos_x, occ->pos_y, pos_xy);
}

int po_set_map_occupancy_device(po_handle h, const po_occupancy *occ) { return po_set_map_stack_occupancy_device(h, 1, occ, nullptr); }

int po_set_map_stack_occupancy(po_handle h, int M, const po_occupancy *occ, const double *pos_xy) {
    if (int rc = check_occupancy(h, M, occ)) return rc;
    Stage S;
    const Slot<unsigned char> d_cells = S.in(occ->cells, (size_t)M * (size_t)occ->size_x * (size_t)occ->size_y);
    const Slot<double> d_pos = S.in(pos_xy, 2 * (size_t)M);
    // (no output: the synchronise alone) like po_set_map: the caller's images may be reused, the stack is in place
    return staged_call(h, S, &po_handle_s::edt_io, true, [&] {
        po_occupancy dev = *occ;
        dev.cells = d_cells;
        return po_set_map_stack_occupancy_device(h, M, &dev, d_pos);
    });
}

int po_set_map_occupancy(po_handle h, const po_occupancy *occ) { return po_set_map_stack_occupancy(h, 1, occ, nullptr); }

// ---- obstacle lists -> occupancy images -> the stack (po_raster.hip) --------------------------------
// What every entry can check without reading through a pointer of the struct (testable without a GPU)
static int check_lists(po_handle h, int M, const po_obstacle_lists *L) {
    if (!h || M < 1 || !L || !L->first || L->n_obs < 0 || (L->n_obs > 0 && !L->obs) || L->size_x < 1 || L->size_y < 1 || !(L->resolution > 0) ||
        !std::isfinite(L->resolution))
        return PO_ERR_INVALID;
    if (L->base_count != 0 && L->base_count != 1 && L->base_count != M) return PO_ERR_INVALID;
    if (L->base_count != 0 && !L->base) return PO_ERR_INVALID;
    if (L->size_x > po_edt_max_side() || L->size_y > po_edt_max_side() || M > po_edt_max_images()) return PO_ERR_UNSUPPORTED;
    return PO_OK;
}
// The host entries read the lists themselves: everything the device entries can only clamp is refused here, before the handle is touched
static int check_list_contents(int M, const po_obstacle_lists *L) {
    if (L->first[0] != 0) return PO_ERR_INVALID;
    for (int k = 0; k < M; ++k)
        if (L->first[k + 1] < L->first[k]) return PO_ERR_INVALID;
    if (L->first[M] > L->n_obs) return PO_ERR_INVALID;
    for (int i = 0; i < L->n_obs; ++i) {
        const po_obstacle &o = L->obs[i];
        if (o.kind == PO_OBS_DISC) {
            if (!std::isfinite(o.v[0]) || !std::isfinite(o.v[1]) || !std::isfinite(o.v[2]) || o.v[2] < 0) return PO_ERR_INVALID;
        } else if (o.kind == PO_OBS_POLY) {
            if (o.n_verts < 3 || o.n_verts > PO_OBS_MAX_VERTS) return PO_ERR_INVALID;
            for (int e = 0; e < 2 * o.n_verts; ++e)
                if (!std::isfinite(o.v[e])) return PO_ERR_INVALID;
        } else {
            return PO_ERR_INVALID;
        }
    }
    return PO_OK;
}
// The device copy of a host struct: the staged arrays in place of the caller's
struct StagedLists {
    Slot<po_obstacle> obs;
    Slot<int> first;
    Slot<unsigned char> base;
    Slot<double> pos;
    void declare(Stage &S, int M, const po_obstacle_lists *L, const double *pos_xy) {
        obs = S.in(L->n_obs > 0 ? L->obs : nullptr, (size_t)L->n_obs);
        first = S.in(L->first, (size_t)M + 1);
        base = S.in(L->base_count > 0 ? L->base : nullptr, (size_t)L->base_count * (size_t)L->size_x * (size_t)L->size_y);
        pos = S.in(pos_xy, 2 * (size_t)M);
    }
    po_obstacle_lists device(const po_obstacle_lists *L) const {
        po_obstacle_lists d = *L;
        d.obs = obs; d.first = first; d.base = base;
        return d;
    }
};

int po_rasterize_batch_device(po_handle h, int M, const po_obstacle_lists *lists, const double *pos_xy, unsigned char *cells_out) {
    if (int rc = check_lists(h, M, lists)) return rc;
    if (!cells_out) return PO_ERR_INVALID;
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(po_launch_raster(lists, M, pos_xy, cells_out, h->stream));
    return PO_OK;
}

int po_rasterize_batch(po_handle h, int M, const po_obstacle_lists *lists, const double *pos_xy, unsigned char *cells_out) {
    if (int rc = check_lists(h, M, lists)) return rc;
    if (!cells_out) return PO_ERR_INVALID;
    if (int rc = check_list_contents(M, lists)) return rc;
    Stage S;
    StagedLists d;
    d.declare(S, M, lists, pos_xy);
    const Slot<unsigned char> d_cells = S.out(cells_out, (size_t)M * (size_t)lists->size_x * (size_t)lists->size_y);
    return staged_call(h, S, &po_handle_s::edt_io, true, [&] {
        const po_obstacle_lists dev = d.device(lists);
        return po_rasterize_batch_device(h, M, &dev, d.pos, d_cells);
    });
}

int po_set_map_stack_obstacles_device(po_handle h, int M, const po_obstacle_lists *lists, const double *pos_xy) {
    if (int rc = check_lists(h, M, lists)) return rc;
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    // the images live in a grow-only block of the handle: with the M and size it already holds nothing is allocated and nothing waits
    if (int rc = grow_after_sync(h, h->raster_buf, (size_t)M * (size_t)lists->size_x * (size_t)lists->size_y)) return rc;
    unsigned char *cells = static_cast<unsigned char *>(h->raster_buf.p);
    HIP_TRY(po_launch_raster(lists, M, pos_xy, cells, h->stream));
    return stack_from_images(h, M, cells, lists->size_x, lists->size_y, lists->resolution, lists->pos_x, lists->pos_y, pos_xy);
}

int po_set_map_stack_obstacles(po_handle h, int M, const po_obstacle_lists *lists, const double *pos_xy) {
    if (int rc = check_lists(h, M, lists)) return rc;
    if (int rc = check_list_contents(M, lists)) return rc;
    Stage S;  // obs, first, pos_xy and the base: the images never exist on the host
    StagedLists d;
    d.declare(S, M, lists, pos_xy);
    // (no output: the synchronise alone) the caller's lists may be reused, the stack is in place
    return staged_call(h, S, &po_handle_s::edt_io, true, [&] {
        const po_obstacle_lists dev = d.device(lists);
        return po_set_map_stack_obstacles_device(h, M, &dev, d.pos);
    });
}

// ---- the static world: a world grid on the handle, polygon rings (po_scene.hip) --------------------------------
static int check_world(po_handle h, const po_occupancy *w, int outside_occupied) {
    if (!h || (outside_occupied != 0 && outside_occupied != 1)) return PO_ERR_INVALID;
    if (!w) return PO_OK;  // clears
    if (!w->cells || w->size_x < 1 || w->size_y < 1 || !(w->resolution > 0) || !std::isfinite(w->resolution) || !std::isfinite(w->pos_x) || !std::isfinite(w->pos_y))
        return PO_ERR_INVALID;
    if (w->size_x > PO_WORLD_MAX_SIDE || w->size_y > PO_WORLD_MAX_SIDE) return PO_ERR_UNSUPPORTED;
    return PO_OK;
}
// The image into the handle's block, on the stream: launches already enqueued that read the old world run before the copy
static int install_world(po_handle h, const po_occupancy *w, int outside_occupied, hipMemcpyKind kind) PO_REQUIRES(h->mu) {
    if (!w) {  // (the block stays: launches already enqueued got its address by value)
        h->world = po_occupancy{};
        return PO_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    const size_t bytes = (size_t)w->size_x * (size_t)w->size_y;
    if (bytes > h->world_buf.cap) h->world.cells = nullptr;  // the old image is about to be released: no world until the new one is in place
    if (int rc = grow_after_sync(h, h->world_buf, bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(h->world_buf.p, w->cells, bytes, kind, h->stream));
    h->world = *w;
    h->world.cells = static_cast<const unsigned char *>(h->world_buf.p);
    h->world_outside = outside_occupied;
    return PO_OK;
}

int po_set_world_occupancy_device(po_handle h, const po_occupancy *world, int outside_occupied) {
    if (int rc = check_world(h, world, outside_occupied)) return rc;
    Lock g(h->mu);
    return install_world(h, world, outside_occupied, hipMemcpyDeviceToDevice);
}

int po_set_world_occupancy(po_handle h, const po_occupancy *world, int outside_occupied) {
    if (int rc = check_world(h, world, outside_occupied)) return rc;
    Lock call(h->call_mu);
    Lock g(h->mu);
    PO_TRY(install_world(h, world, outside_occupied, hipMemcpyHostToDevice));
    if (world) HIP_TRY(hipStreamSynchronize(h->stream));  // the caller's image may be reused
    return PO_OK;
}

// What every scene entry can check without reading through a pointer of the struct (testable without a GPU); the handle is not looked at before the struct
static int check_scene(po_handle h, int M, const po_scene *S) {
    if (!h || !S) return PO_ERR_INVALID;
    if (int rc = check_lists(h, M, &S->lists)) return rc;
    const po_rings &R = S->rings;
    if (R.n_rings < 0 || (R.n_rings > 0 && (R.n_verts < 0 || !R.start || !R.flags || (R.n_verts > 0 && !R.verts)))) return PO_ERR_INVALID;
    if (S->use_world != 0 && S->use_world != 1) return PO_ERR_INVALID;
    return PO_OK;
}
// The host entries read the tables themselves: everything the device entries can only clamp is refused here, before the handle is touched
static int check_scene_contents(int M, const po_scene *S) {
    if (int rc = check_list_contents(M, &S->lists)) return rc;
    const po_rings &R = S->rings;
    if (R.n_rings == 0) return PO_OK;
    if (R.start[0] != 0) return PO_ERR_INVALID;
    for (int r = 0; r < R.n_rings; ++r) {
        const long long n = (long long)R.start[r + 1] - (long long)R.start[r];
        if (n < 3 || n > PO_RING_MAX_VERTS) return PO_ERR_INVALID;  // (also: start[] non-decreasing)
        if (R.flags[r] != PO_RING_SOLID && R.flags[r] != PO_RING_FREE) return PO_ERR_INVALID;
    }
    if (R.start[R.n_rings] > R.n_verts) return PO_ERR_INVALID;
    for (size_t i = 0; i < 2 * (size_t)R.n_verts; ++i)
        if (!std::isfinite(R.verts[i])) return PO_ERR_INVALID;
    if (R.n_shared < 0 || R.n_shared > R.n_rings) return PO_ERR_INVALID;
    if (!R.first) return R.n_shared == R.n_rings ? PO_OK : PO_ERR_INVALID;
    if (R.first[0] != R.n_shared) return PO_ERR_INVALID;
    for (int k = 0; k < M; ++k)
        if (R.first[k + 1] < R.first[k]) return PO_ERR_INVALID;
    if (R.first[M] > R.n_rings) return PO_ERR_INVALID;
    return PO_OK;
}
// The device copy of a host scene: the staged arrays in place of the caller's
struct StagedScene {
    StagedLists lists;
    Slot<double> verts;
    Slot<int> start, flags, first;
    void declare(Stage &S, int M, const po_scene *sc, const double *pos_xy) {
        lists.declare(S, M, &sc->lists, pos_xy);
        const po_rings &R = sc->rings;
        if (R.n_rings == 0) return;
        verts = S.in(R.n_verts > 0 ? R.verts : nullptr, 2 * (size_t)R.n_verts);
        start = S.in(R.start, (size_t)R.n_rings + 1);
        flags = S.in(R.flags, (size_t)R.n_rings);
        first = S.in(R.first, (size_t)M + 1);
    }
    po_scene device(const po_scene *sc) const {
        po_scene d = *sc;
        d.lists = lists.device(&sc->lists);
        d.rings.verts = verts; d.rings.start = start; d.rings.flags = flags; d.rings.first = first;
        return d;
    }
};
// scene -> M images at `cells` on the device (device set): po_raster.hip's image of the lists, then the world and the rings ORed into it
static int scene_images(po_handle h, int M, const po_scene *S, const double *pos_xy, unsigned char *cells) PO_REQUIRES(h->mu) {
    HIP_TRY(po_launch_raster(&S->lists, M, pos_xy, cells, h->stream));
    if (S->rings.n_rings == 0 && !S->use_world) return PO_OK;  // nothing to add: the bytes of po_rasterize_batch
    po_scene sc = *S;
    if (sc.rings.n_rings == 0) sc.rings = po_rings{};
    HIP_TRY(po_launch_scene(&sc, M, pos_xy, S->use_world ? &h->world : nullptr, h->world_outside, cells, h->stream));
    return PO_OK;
}
static bool world_missing(po_handle h, const po_scene *S) PO_REQUIRES(h->mu) { return S->use_world && !h->world.cells; }
// ... as the pre-check of staged_call: a scene entry that lacks its world refuses before anything is staged
static auto needs_world(const po_scene *S) {
    return [S](po_handle h) PO_REQUIRES(h->mu) { return world_missing(h, S) ? PO_ERR_INVALID : PO_OK; };
}

int po_rasterize_scene_batch_device(po_handle h, int M, const po_scene *scene, const double *pos_xy, unsigned char *cells_out) {
    if (int rc = check_scene(h, M, scene)) return rc;
    if (!cells_out) return PO_ERR_INVALID;
    Lock g(h->mu);
    if (world_missing(h, scene)) return PO_ERR_INVALID;
    HIP_TRY(hipSetDevice(h->device));
    return scene_images(h, M, scene, pos_xy, cells_out);
}

int po_rasterize_scene_batch(po_handle h, int M, const po_scene *scene, const double *pos_xy, unsigned char *cells_out) {
    if (int rc = check_scene(h, M, scene)) return rc;
    if (!cells_out) return PO_ERR_INVALID;
    if (int rc = check_scene_contents(M, scene)) return rc;
    Stage S;
    StagedScene d;
    d.declare(S, M, scene, pos_xy);
    const Slot<unsigned char> d_cells = S.out(cells_out, (size_t)M * (size_t)scene->lists.size_x * (size_t)scene->lists.size_y);
    return staged_call(h, S, &po_handle_s::edt_io, true, [&] {
        const po_scene dev = d.device(scene);
        return po_rasterize_scene_batch_device(h, M, &dev, d.lists.pos, d_cells);
    }, needs_world(scene));
}

int po_set_map_stack_scene_device(po_handle h, int M, const po_scene *scene, const double *pos_xy) {
    if (int rc = check_scene(h, M, scene)) return rc;
    Lock g(h->mu);
    if (world_missing(h, scene)) return PO_ERR_INVALID;
    HIP_TRY(hipSetDevice(h->device));
    const po_obstacle_lists &L = scene->lists;
    // the images live in a grow-only block of the handle: with the M and size it already holds nothing is allocated and nothing waits
    if (int rc = grow_after_sync(h, h->raster_buf, (size_t)M * (size_t)L.size_x * (size_t)L.size_y)) return rc;
    unsigned char *cells = static_cast<unsigned char *>(h->raster_buf.p);
    PO_TRY(scene_images(h, M, scene, pos_xy, cells));
    return stack_from_images(h, M, cells, L.size_x, L.size_y, L.resolution, L.pos_x, L.pos_y, pos_xy);
}

int po_set_map_stack_scene(po_handle h, int M, const po_scene *scene, const double *pos_xy) {
    if (int rc = check_scene(h, M, scene)) return rc;
    if (int rc = check_scene_contents(M, scene)) return rc;
    Stage S;  // the lists, the ring tables, pos_xy and the base: the images never exist on the host
    StagedScene d;
    d.declare(S, M, scene, pos_xy);
    // (no output: the synchronise alone) the caller's tables may be reused, the stack is in place
    return staged_call(h, S, &po_handle_s::edt_io, true, [&] {
        const po_scene dev = d.device(scene);
        return po_set_map_stack_scene_device(h, M, &dev, d.lists.pos);
    }, needs_world(scene));
}

int po_get_map_layer(po_handle h, int k, po_map *geometry_out, float *distance_or_null) {
    if (!h || !geometry_out) return PO_ERR_INVALID;
    Lock call(h->call_mu);
    Lock g(h->mu);
    const po::DevMaps &s = h->maps;
    if (!s.d || k < 0 || k >= s.M) return PO_ERR_INVALID;
    double pos[2] = {s.px, s.py};
    if (s.pos) {  // per-layer centres live on the device (they may have arrived through a device pointer)
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpyAsync(pos, s.pos + 2 * (size_t)k, sizeof(pos), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    *geometry_out = po_map{nullptr, s.sx, s.sy, s.res, pos[0], pos[1]};
    if (!distance_or_null) return PO_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(distance_or_null, s.d + (size_t)k * s.stride, sizeof(float) * s.stride, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PO_OK;
}

int po_get_map(po_handle h, po_map *geometry_out, float *distance_or_null) { return po_get_map_layer(h, 0, geometry_out, distance_or_null); }

// One argument check per stage, shared by its device-pointer entry and its host-pointer twin
static bool postcheck_args_ok(po_handle h, int B, int N, const double *states, const po_info *info, const int *n_valid, const int *ok) {
    return h && B >= 0 && N >= 1 && (B == 0 || (states && info && n_valid && ok));
}
static bool densify_args_ok(po_handle h, int B, int N, const double *states, const po_info *info, int M, const double *out_states, const int *n_out, const int *ok) {
    return h && B >= 0 && N >= 3 && M >= 1 && (B == 0 || (states && info && out_states && n_out && ok));
}

int po_postcheck_batch_device(po_handle h, int B, int N, const int *n_points, const double *states, const po_info *info, int *n_valid, int *ok) {
    if (!postcheck_args_ok(h, B, N, states, info, n_valid, ok)) return PO_ERR_INVALID;
    Lock g(h->mu);
    if (!h->maps.d && h->params.enable_collision_check) return PO_ERR_INVALID;  // no map set
    if (!assignment_covers(h, B)) return PO_ERR_INVALID;
    if (B == 0) return PO_OK;
    HIP_TRY(hipSetDevice(h->device));
    const po::DevCar car = make_car(h->params);
    HIP_TRY(po_launch_postcheck(&h->maps, &car, B, N, n_points, states, info, n_valid, ok, h->stream));
    return PO_OK;
}

int po_densify_batch_device(po_handle h, int B, int N, const int *n_points, const double *states, const po_info *info, int M, double *out_states, int *n_out, int *ok) {
    if (!densify_args_ok(h, B, N, states, info, M, out_states, n_out, ok)) return PO_ERR_INVALID;
    Lock g(h->mu);
    if (!h->maps.d && h->params.enable_collision_check) return PO_ERR_INVALID;  // no map set
    if (!assignment_covers(h, B)) return PO_ERR_INVALID;
    if (!(h->params.output_spacing > 0)) return PO_ERR_INVALID;
    if (B == 0) return PO_OK;
    if (sizeof(double) * 15 * (size_t)N > 160 * 1024) return PO_ERR_UNSUPPORTED;
    HIP_TRY(hipSetDevice(h->device));
    const po::DevCar car = make_car(h->params);
    HIP_TRY(po_launch_densify(&h->maps, &car, B, N, n_points, states, info, h->params.output_spacing, M, out_states, n_out, ok, h->stream));
    return PO_OK;
}

int po_densify_batch(po_handle h, int B, int N, const int *n_points, const double *states, const po_info *info, int M, double *out_states, int *n_out, int *ok) {
    if (!densify_args_ok(h, B, N, states, info, M, out_states, n_out, ok)) return PO_ERR_INVALID;
    if (B == 0) return PO_OK;
    Stage S;
    const Slot<double> d_states = S.in(states, 5 * (size_t)B * N), d_out = S.out(out_states, 5 * (size_t)B * M);
    const Slot<po_info> d_info = S.in(info, B);
    const Slot<int> d_np = S.in(n_points, B), d_nout = S.out(n_out, B), d_ok = S.out(ok, B);
    return staged_call(h, S, &po_handle_s::post_buf, false, [&] { return po_densify_batch_device(h, B, N, d_np, d_states, d_info, M, d_out, d_nout, d_ok); });
}

int po_postcheck_batch(po_handle h, int B, int N, const int *n_points, const double *states, const po_info *info, int *n_valid, int *ok) {
    if (!postcheck_args_ok(h, B, N, states, info, n_valid, ok)) return PO_ERR_INVALID;
    if (B == 0) return PO_OK;
    Stage S;
    const Slot<double> d_states = S.in(states, 5 * (size_t)B * N);
    const Slot<po_info> d_info = S.in(info, B);
    const Slot<int> d_np = S.in(n_points, B), d_nvalid = S.out(n_valid, B), d_ok = S.out(ok, B);
    return staged_call(h, S, &po_handle_s::post_buf, false, [&] { return po_postcheck_batch_device(h, B, N, d_np, d_states, d_info, d_nvalid, d_ok); });
}

// ---- score and select --------------------------------------------------------------------------
void po_default_select_params(po_select_params *p) {
    if (!p) return;
    const double w[PO_N_FEAT] = {1, 10, 10, 0, 0, 10, 5, 1};  // a starting point nobody has tuned
    for (int j = 0; j < PO_N_FEAT; ++j) p->w[j] = w[j];
    p->d_safe = 0.5;
    p->min_clearance = 0.0;
    p->max_kmax = std::numeric_limits<double>::max();
    p->max_goal_dist = std::numeric_limits<double>::max();
}

static bool select_args_ok(po_handle h, const po_select_params *p, const po_select_in *in, const po_select_out *out) {
    if (!h || !p || !in || !out || in->B < 0 || in->N < 0 || in->G < 0) return false;
    for (int j = 0; j < PO_N_FEAT; ++j)
        if (!std::isfinite(p->w[j])) return false;
    if (std::isnan(p->d_safe) || std::isnan(p->min_clearance) || std::isnan(p->max_kmax) || std::isnan(p->max_goal_dist)) return false;
    if (in->prev_states && in->Np < 0) return false;
    if (in->B == 0 || in->G == 0) return true;
    if (!in->states || !in->group_start || !out->best) return false;
    if (in->goal && in->goal_stride < 2) return false;
    return !out->sel_states || out->sel_n;
}

int po_select_batch_device(po_handle h, const po_select_params *p, const po_select_in *in, const po_select_out *out) {
    if (!select_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0 || in->G == 0) return PO_OK;  // nothing to score or nothing to select: no launch, whatever the handle holds
    Lock g(h->mu);
    if (!h->maps.d || !assignment_covers(h, in->B)) return PO_ERR_INVALID;  // po_set_map first; an assignment covers every candidate
    HIP_TRY(hipSetDevice(h->device));
    const size_t gs_bytes = (sizeof(int) * ((size_t)in->G + 1) + 15) & ~(size_t)15;
    PO_TRY(grow_after_sync(h, h->select_buf, gs_bytes + (out->cost ? 0 : sizeof(double) * (size_t)in->B)));
    po::DevSelect D{};
    D.B = in->B; D.N = in->N; D.G = in->G; D.goal_stride = in->goal_stride;
    D.Np = in->prev_states && in->Np > 0 ? in->Np : 0;
    D.states = in->states; D.n_states = in->n_states; D.ok = in->ok; D.goal = in->goal;
    D.group_start = in->group_start;
    D.prev_states = D.Np ? in->prev_states : nullptr; D.prev_n = in->prev_n;
    for (int j = 0; j < PO_N_FEAT; ++j) D.w[j] = p->w[j];
    D.d_safe = p->d_safe; D.min_clearance = p->min_clearance; D.max_kmax = p->max_kmax; D.max_goal_dist = p->max_goal_dist;
    D.gs = static_cast<int *>(h->select_buf.p);
    D.feat = out->feat;
    D.cost = out->cost ? out->cost : reinterpret_cast<double *>(static_cast<char *>(h->select_buf.p) + gs_bytes);
    D.best = out->best; D.best_cost = out->best_cost; D.n_feasible = out->n_feasible; D.sel_states = out->sel_states; D.sel_n = out->sel_n;
    const po::DevCar car = make_car(h->params);
    HIP_TRY(po_launch_select(&h->maps, &car, &D, h->stream));
    return PO_OK;
}

int po_select_batch(po_handle h, const po_select_params *p, const po_select_in *in, const po_select_out *out) {
    if (!select_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    const bool empty = in->B == 0 || in->G == 0;
    if (!empty) {  // the table is in host memory here: validated (the device entry reads it clamped instead)
        const int *gs = in->group_start;
        if (gs[0] < 0 || gs[in->G] > in->B) return PO_ERR_INVALID;
        for (int g = 0; g < in->G; ++g)
            if (gs[g + 1] < gs[g]) return PO_ERR_INVALID;
    }
    const size_t B = in->B, G = in->G, N = in->N, Np = in->prev_states && in->Np > 0 ? in->Np : 0;
    Stage S;
    po_select_in d = *in;
    po_select_out o{};
    if (!empty) {
        const Slot<double> states = S.in(in->states, 5 * B * N), goal = S.in(in->goal, B * (size_t)in->goal_stride), prev = S.in(Np ? in->prev_states : nullptr, 5 * G * Np);
        const Slot<int> ns = S.in(in->n_states, B), ok = S.in(in->ok, B), gs = S.in(in->group_start, G + 1), pn = S.in(Np ? in->prev_n : nullptr, G);
        const Slot<double> feat = S.out_opt(out->feat, PO_N_FEAT * B), cost = S.out_opt(out->cost, B);
        const Slot<double> bc = S.out_opt(out->best_cost, G), ss = S.out_opt(out->sel_states, 5 * G * N);
        const Slot<int> best = S.out(out->best, G), nf = S.out_opt(out->n_feasible, G), sn = S.out_opt(out->sel_n, G);
        return staged_call(h, S, &po_handle_s::post_buf, false, [&] {
            d.states = states; d.goal = goal; d.prev_states = prev; d.n_states = ns; d.ok = ok; d.group_start = gs; d.prev_n = pn;
            d.Np = (int)Np;
            o = po_select_out{feat, cost, best, bc, nf, ss, sn};
            return po_select_batch_device(h, p, &d, &o);
        });
    }
    return PO_OK;  // B = 0 or G = 0: nothing is staged, launched or written
}

// ---- speed profile -----------------------------------------------------------------------------
void po_default_speed_params(po_speed_params *p) {
    if (!p) return;
    *p = po_speed_params{15.0, 3.0, 2.0, 3.0, 1.0, 2.0, 0};  // a starting point nobody has tuned
}

static bool speed_args_ok(po_handle h, const po_speed_params *p, const po_speed_in *in, const po_speed_out *out) {
    if (!h || !p || !in || !out || in->B < 0 || in->N < 0) return false;
    // (every comparison is false for a NaN, so each range is written as the condition that must HOLD)
    if (!(p->v_max > 0) || !std::isfinite(p->v_max) || !(p->a_lat_max > 0) || !(p->a_lat_max <= h->params.mu * 9.8)) return false;
    if (!(p->a_max > 0) || !(p->b_max > 0) || !(p->clear_v0 >= 0) || !(p->clear_gain >= 0)) return false;
    if (in->B == 0) return true;
    return in->states && in->v0 && out->v && out->a && out->status;
}

int po_speed_batch_device(po_handle h, const po_speed_params *p, const po_speed_in *in, const po_speed_out *out) {
    if (!speed_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing to profile: no launch, whatever the handle holds
    Lock g(h->mu);
    if (p->use_map && (!h->maps.d || !assignment_covers(h, in->B))) return PO_ERR_INVALID;  // po_set_map first; an assignment covers every path
    HIP_TRY(hipSetDevice(h->device));
    po::DevSpeed D{};
    D.B = in->B; D.N = in->N; D.use_map = p->use_map ? 1 : 0;
    D.states = in->states; D.n_states = in->n_states; D.ok = in->ok; D.v0 = in->v0; D.v_end = in->v_end; D.v_limit = in->v_limit;
    D.v_max = p->v_max; D.a_lat_max = p->a_lat_max; D.a_max = p->a_max; D.b_max = p->b_max; D.clear_v0 = p->clear_v0; D.clear_gain = p->clear_gain;
    D.A = h->params.mu * 9.8;  // one multiply, as updateLimits forms it
    D.R = h->params.max_curvature_rate;
    D.v = out->v; D.a = out->a; D.t = out->t; D.total_time = out->total_time; D.status = out->status;
    const po::DevMaps maps = p->use_map ? h->maps : po::DevMaps{};  // use_map = 0: the kernels get no map to read
    const po::DevCar car = make_car(h->params);
    HIP_TRY(po_launch_speed(&maps, &car, &D, h->stream));
    return PO_OK;
}

int po_speed_batch(po_handle h, const po_speed_params *p, const po_speed_in *in, const po_speed_out *out) {
    if (!speed_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing is staged, launched or written
    const size_t B = in->B, bn = B * (size_t)in->N;
    Stage S;
    const Slot<double> states = S.in(in->states, 5 * bn), v0 = S.in(in->v0, B), ve = S.in(in->v_end, B), vl = S.in(in->v_limit, bn);
    const Slot<int> ns = S.in(in->n_states, B), ok = S.in(in->ok, B);
    const Slot<double> v = S.out(out->v, bn), a = S.out(out->a, bn), t = S.out_opt(out->t, bn), tt = S.out_opt(out->total_time, B);
    const Slot<int> status = S.out(out->status, B);
    return staged_call(h, S, &po_handle_s::post_buf, false, [&] {
        const po_speed_in d{in->B, in->N, states, ns, ok, v0, ve, vl};
        const po_speed_out o{v, a, t, tt, status};
        return po_speed_batch_device(h, p, &d, &o);
    });
}

// ---- moving obstacles (po_dynamic.hip) ----------------------------------------------------------
void po_default_dynamic_params(po_dynamic_params *p) {
    if (!p) return;
    *p = po_dynamic_params{0.3, 5.0};  // a starting point nobody has tuned
}

// ---- agent lists (po_agent_lists): what the entries of the stages that read agents share ----------------------------------------------
// What both entries can check without reading through a pointer of the lists; a batch of B > 0 needs lists
static bool agent_lists_shape_ok(const po_agent_lists *L, int B) {
    if (L && (L->S < 0 || L->n_agents < 0)) return false;
    if (B == 0) return true;
    return L && L->S >= 1 && L->first && (L->n_agents == 0 || L->agents);
}
// The host entries read the lists themselves: everything the device entries can only clamp is refused here, before the handle is touched
static bool agent_lists_host_ok(const po_agent_lists *L, const int *set_of, int B) {
    if (L->first[0] != 0) return false;
    for (int k = 0; k < L->S; ++k)
        if (L->first[k + 1] < L->first[k]) return false;
    if (L->first[L->S] > L->n_agents) return false;
    if (set_of)
        for (int b = 0; b < B; ++b)
            if (set_of[b] < 0 || set_of[b] >= L->S) return false;
    for (int i = 0; i < L->n_agents; ++i) {
        const po_agent &g = L->agents[i];
        if (g.n_pts < 1 || g.n_pts > PO_AGENT_MAX_PTS || (g.flags & ~(PO_AGENT_HOLD_BEFORE | PO_AGENT_HOLD_AFTER))) return false;
        if (!std::isfinite(g.radius) || g.radius < 0) return false;
        for (int j = 0; j < g.n_pts; ++j) {
            if (!std::isfinite(g.t[j]) || !std::isfinite(g.x[j]) || !std::isfinite(g.y[j])) return false;
            if (j > 0 && !(g.t[j] > g.t[j - 1])) return false;
        }
    }
    return true;
}
struct StagedAgents {
    Slot<po_agent> agents;
    Slot<int> first;
    po_agent_lists dev(const po_agent_lists *L) const { return po_agent_lists{agents, first, L->n_agents, L->S}; }  // (after the block is reserved)
};
static void stage_agent_lists(Stage &S, const po_agent_lists *L, StagedAgents *q) {  // declares the arrays of a po_agent_lists on S
    q->first = S.in(L->first, (size_t)L->S + 1);
    q->agents = S.in(L->n_agents > 0 ? L->agents : nullptr, (size_t)L->n_agents);
}

// What both entries can check without reading through a pointer of the structs (testable without a GPU)
static bool dynamic_args_ok(po_handle h, const po_dynamic_params *p, const po_dynamic_in *in, const po_dynamic_out *out) {
    if (!h || !p || !in || !out || in->B < 0 || in->N < 0) return false;
    if (!std::isfinite(p->margin) || !std::isfinite(p->stop_distance) || p->stop_distance < 0) return false;
    if (!agent_lists_shape_ok(in->agents, in->B)) return false;
    return in->B == 0 || (in->states && in->t && out->status);
}

int po_dynamic_batch_device(po_handle h, const po_dynamic_params *p, const po_dynamic_in *in, const po_dynamic_out *out) {
    if (!dynamic_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing to check: no launch, whatever the handle holds
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    po::DevDynamic D{};
    D.B = in->B; D.N = in->N; D.S = in->agents->S; D.n_agents = in->agents->n_agents;
    D.states = in->states; D.n_states = in->n_states; D.ok = in->ok; D.t = in->t; D.set_of = in->set_of;
    D.agents = in->agents->agents; D.first = in->agents->first; D.v_limit_in = in->v_limit_in;
    D.margin = p->margin; D.stop_distance = p->stop_distance;
    D.status = out->status; D.ok_out = out->ok_out; D.gap_min = out->gap_min; D.first_state = out->first_state; D.first_agent = out->first_agent;
    D.stop_state = out->stop_state; D.first_time = out->first_time; D.gap = out->gap; D.v_limit = out->v_limit;
    const po::DevCar car = make_car(h->params);
    HIP_TRY(po_launch_dynamic(&car, &D, h->stream));
    return PO_OK;
}

int po_dynamic_batch(po_handle h, const po_dynamic_params *p, const po_dynamic_in *in, const po_dynamic_out *out) {
    if (!dynamic_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing is staged, launched or written
    if (!agent_lists_host_ok(in->agents, in->set_of, in->B)) return PO_ERR_INVALID;
    const size_t B = in->B, bn = B * (size_t)in->N;
    Stage S;
    const Slot<double> states = S.in(in->states, 5 * bn), t = S.in(in->t, bn), vin = S.in(in->v_limit_in, bn);
    const Slot<int> ns = S.in(in->n_states, B), ok = S.in(in->ok, B), set_of = S.in(in->set_of, B);
    StagedAgents ag;
    stage_agent_lists(S, in->agents, &ag);
    const Slot<int> status = S.out(out->status, B), ok_out = S.out_opt(out->ok_out, B), fs = S.out_opt(out->first_state, B), fa = S.out_opt(out->first_agent, B);
    const Slot<int> ss = S.out_opt(out->stop_state, B);
    const Slot<double> gmin = S.out_opt(out->gap_min, B), ft = S.out_opt(out->first_time, B), gap = S.out_opt(out->gap, bn), vl = S.out_opt(out->v_limit, bn);
    return staged_call(h, S, &po_handle_s::post_buf, false, [&] {
        const po_agent_lists dl = ag.dev(in->agents);
        const po_dynamic_in d{in->B, in->N, states, ns, ok, t, set_of, &dl, vin};
        const po_dynamic_out o{status, ok_out, gmin, fs, fa, ss, ft, gap, vl};
        return po_dynamic_batch_device(h, p, &d, &o);
    });
}

// ---- station-time speed planning (po_stplan.hip) ------------------------------------------------
void po_default_stplan_params(po_stplan_params *p) {
    if (!p) return;
    *p = po_stplan_params{1.0, 8, 3, 20, 0.5, 2.0, 3.0, 15.0, 1.0, 1.0};  // a starting point nobody has tuned
}

// What both entries can check without reading through a pointer of the structs (testable without a GPU)
static bool stplan_args_ok(po_handle h, const po_stplan_params *p, const po_stplan_in *in, const po_stplan_out *out) {
    if (!h || !p || !in || !out || in->B < 0 || in->N < 0) return false;
    auto pos = [](double v) { return std::isfinite(v) && v > 0; };
    auto wgt = [](double v) { return std::isfinite(v) && v >= 0; };
    if (!pos(p->dt) || !pos(p->a_max) || !pos(p->b_max) || !pos(p->v_max) || !wgt(p->w_acc) || !wgt(p->w_slow) || !std::isfinite(p->margin)) return false;
    if (p->K < 1 || p->K > PO_ST_MAX_LAYERS || p->stride < 1 || p->U < 1 || p->U > PO_ST_MAX_STEP) return false;
    if (!agent_lists_shape_ok(in->agents, in->B)) return false;
    return in->B == 0 || (in->states && in->v0 && out->status);
}

int po_stplan_batch_device(po_handle h, const po_stplan_params *p, const po_stplan_in *in, const po_stplan_out *out) {
    if (!stplan_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing to plan: no launch, whatever the handle holds
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    po::DevStplan D{};
    D.B = in->B; D.N = in->N; D.S = in->agents->S; D.n_agents = in->agents->n_agents;
    D.states = in->states; D.n_states = in->n_states; D.ok = in->ok; D.v0 = in->v0; D.v_cap = in->v_cap; D.set_of = in->set_of;
    D.agents = in->agents->agents; D.first = in->agents->first; D.v_limit_in = in->v_limit_in;
    D.dt = p->dt; D.K = p->K; D.stride = p->stride; D.U = p->U; D.margin = p->margin; D.a_max = p->a_max; D.b_max = p->b_max; D.v_max = p->v_max;
    D.w_acc = p->w_acc; D.w_slow = p->w_slow;
    const int mb = in->N > 0 ? (in->N - 1) / p->stride + 1 : 1;  // no path of the call has more stations: the LDS is sized from it
    D.Mb = mb > PO_ST_MAX_STATIONS ? PO_ST_MAX_STATIONS : mb;
    D.status = out->status; D.ok_out = out->ok_out; D.n_layers = out->n_layers; D.cost = out->cost; D.station = out->station; D.cells = out->cells;
    D.v_limit = out->v_limit;
    const po::DevCar car = make_car(h->params);
    HIP_TRY(po_launch_stplan(&car, &D, h->stream));
    return PO_OK;
}

int po_stplan_batch(po_handle h, const po_stplan_params *p, const po_stplan_in *in, const po_stplan_out *out) {
    if (!stplan_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing is staged, launched or written
    if (!agent_lists_host_ok(in->agents, in->set_of, in->B)) return PO_ERR_INVALID;
    const size_t B = in->B, bn = B * (size_t)in->N;
    Stage S;
    const Slot<double> states = S.in(in->states, 5 * bn), v0 = S.in(in->v0, B), cap = S.in(in->v_cap, bn), vin = S.in(in->v_limit_in, bn);
    const Slot<int> ns = S.in(in->n_states, B), ok = S.in(in->ok, B), set_of = S.in(in->set_of, B);
    StagedAgents ag;
    stage_agent_lists(S, in->agents, &ag);
    const Slot<int> status = S.out(out->status, B), ok_out = S.out_opt(out->ok_out, B), nl = S.out_opt(out->n_layers, B);
    const Slot<int> station = S.out_opt(out->station, B * (PO_ST_MAX_LAYERS + 1)), cells = S.out_opt(out->cells, B * (size_t)p->K * PO_ST_MAX_STATIONS);
    const Slot<double> cost = S.out_opt(out->cost, B), vl = S.out_opt(out->v_limit, bn);
    return staged_call(h, S, &po_handle_s::post_buf, false, [&] {
        const po_agent_lists dl = ag.dev(in->agents);
        const po_stplan_in d{in->B, in->N, states, ns, ok, v0, cap, set_of, &dl, vin};
        const po_stplan_out o{status, ok_out, nl, cost, station, cells, vl};
        return po_stplan_batch_device(h, p, &d, &o);
    });
}

// ---- corridor nudge (po_nudge.hip) ---------------------------------------------------------------
void po_default_nudge_params(po_nudge_params *p) {
    if (!p) return;
    *p = po_nudge_params{0.3, 1.0, 1.0, 0.2, 0};  // a starting point nobody has tuned
}

// What both entries can check without reading through a pointer of the structs (testable without a GPU)
static bool nudge_args_ok(po_handle h, const po_nudge_params *p, const po_nudge_in *in, const po_nudge_out *out) {
    if (!h || !p || !in || !out || in->B < 0 || in->N < 0 || in->W < 0 || p->skip_states < 0) return false;
    auto room = [](double v) { return std::isfinite(v) && v >= 0; };
    if (!std::isfinite(p->margin) || !room(p->t_before) || !room(p->t_after) || !room(p->min_width)) return false;
    if (in->W == 0 && (in->side_prev || out->side)) return false;
    if (out->bounds && out->bounds == in->bounds) return false;
    if (!agent_lists_shape_ok(in->agents, in->B)) return false;
    return in->B == 0 || (in->ref_x && in->ref_y && in->ref_z && in->t && in->bounds && out->bounds && out->status);
}

int po_nudge_batch_device(po_handle h, const po_nudge_params *p, const po_nudge_in *in, const po_nudge_out *out) {
    if (!nudge_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing to carve: no launch, whatever the handle holds
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    po::DevNudge D{};
    D.B = in->B; D.N = in->N; D.W = in->W; D.S = in->agents->S; D.n_agents = in->agents->n_agents; D.skip_states = p->skip_states;
    D.ref_x = in->ref_x; D.ref_y = in->ref_y; D.ref_z = in->ref_z; D.n_points = in->n_points; D.ok = in->ok; D.t = in->t; D.bounds_in = in->bounds;
    D.set_of = in->set_of; D.agents = in->agents->agents; D.first = in->agents->first; D.side_prev = in->side_prev;
    const po_params &q = h->params;
    for (int j = 0; j < 4; ++j) D.d[j] = q.d[j];
    D.radius = std::sqrt((q.car_length / 8) * (q.car_length / 8) + (q.car_width / 2) * (q.car_width / 2)) + q.safety_margin;  // po_bounds_batch's
    D.margin = p->margin; D.t_before = p->t_before; D.t_after = p->t_after; D.min_width = p->min_width;
    D.status = out->status; D.ok_out = out->ok_out; D.bounds = out->bounds; D.side = out->side; D.first_blocked_state = out->first_blocked_state;
    D.first_blocked_agent = out->first_blocked_agent; D.width_min = out->width_min;
    HIP_TRY(po_launch_nudge(&D, h->stream));
    return PO_OK;
}

int po_nudge_batch(po_handle h, const po_nudge_params *p, const po_nudge_in *in, const po_nudge_out *out) {
    if (!nudge_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing is staged, launched or written
    if (!agent_lists_host_ok(in->agents, in->set_of, in->B)) return PO_ERR_INVALID;
    const size_t B = in->B, bn = B * (size_t)in->N, bw = B * (size_t)in->W;
    Stage S;
    const Slot<double> rx = S.in(in->ref_x, bn), ry = S.in(in->ref_y, bn), rz = S.in(in->ref_z, bn), t = S.in(in->t, bn), bin = S.in(in->bounds, 8 * bn);
    const Slot<int> np = S.in(in->n_points, B), ok = S.in(in->ok, B), set_of = S.in(in->set_of, B);
    StagedAgents ag;
    stage_agent_lists(S, in->agents, &ag);
    const Slot<int> sprev = S.in(in->side_prev, bw);
    const Slot<int> status = S.out(out->status, B), ok_out = S.out_opt(out->ok_out, B), side = S.out_opt(out->side, bw);
    const Slot<int> fs = S.out_opt(out->first_blocked_state, B), fa = S.out_opt(out->first_blocked_agent, B);
    const Slot<double> bounds = S.out(out->bounds, 8 * bn), wmin = S.out_opt(out->width_min, B);
    return staged_call(h, S, &po_handle_s::post_buf, false, [&] {
        const po_agent_lists dl = ag.dev(in->agents);
        const po_nudge_in d{in->B, in->N, in->W, rx, ry, rz, np, ok, t, bin, set_of, &dl, sprev};
        const po_nudge_out o{status, ok_out, bounds, side, fs, fa, wmin};
        return po_nudge_batch_device(h, p, &d, &o);
    });
}

// ---- timed trajectory (po_trajectory.hip) --------------------------------------------------------
void po_default_trajectory_params(po_trajectory_params *p) {
    if (!p) return;
    *p = po_trajectory_params{0.0, 0.1, 50, 0, {0, 0, 0, 0}, {0, 0, 0, 0}, 8, 7, PO_AGENT_HOLD_AFTER};  // a starting point nobody has tuned
}

// What both entries can check without reading through a pointer of the structs (testable without a GPU)
static bool trajectory_args_ok(po_handle h, const po_trajectory_params *p, const po_trajectory_in *in, const po_trajectory_out *out) {
    if (!h || !p || !in || !out || in->B < 0 || in->N < 0) return false;
    if (!std::isfinite(p->t0) || !std::isfinite(p->dt) || !(p->dt > 0) || p->K < 1 || p->n_discs < 0 || p->n_discs > PO_TRAJ_MAX_DISCS) return false;
    for (int d = 0; d < p->n_discs; ++d)
        if (!std::isfinite(p->disc_offset[d]) || !std::isfinite(p->disc_radius[d]) || p->disc_radius[d] < 0) return false;
    if (p->agent_pts < 1 || p->agent_pts > PO_AGENT_MAX_PTS || p->agent_stride < 1 || (long long)(p->agent_pts - 1) * p->agent_stride >= p->K) return false;
    if (p->agent_flags & ~(PO_AGENT_HOLD_BEFORE | PO_AGENT_HOLD_AFTER)) return false;
    const size_t B = in->B, bn = B * (size_t)in->N, bk = B * (size_t)p->K;
    if (B > 0 && (!in->states || !in->v || !in->t || !out->status || !out->states || (p->n_discs > 0 && !out->agents))) return false;
    // no output may overlap an input: byte ranges over the full extent of each array (B = 0: every extent is empty)
    struct Range { const void *p; size_t bytes; };
    const Range ins[] = {{in->states, 5 * bn * sizeof(double)}, {in->n_states, B * sizeof(int)}, {in->ok, B * sizeof(int)}, {in->v, bn * sizeof(double)},
                         {in->t, bn * sizeof(double)}};
    const Range outs[] = {{out->status, B * sizeof(int)}, {out->states, 5 * bk * sizeof(double)}, {out->v, bk * sizeof(double)}, {out->a, bk * sizeof(double)},
                          {out->t, bk * sizeof(double)}, {out->index, bk * sizeof(int)}, {out->first_held, B * sizeof(int)},
                          {out->agents, B * (size_t)p->n_discs * sizeof(po_agent)}};
    for (const Range &o : outs)
        for (const Range &i : ins) {
            if (!o.p || !i.p || !o.bytes || !i.bytes) continue;
            const uintptr_t ob = (uintptr_t)o.p, ib = (uintptr_t)i.p;
            if (ob < ib + i.bytes && ib < ob + o.bytes) return false;
        }
    return true;
}

int po_trajectory_batch_device(po_handle h, const po_trajectory_params *p, const po_trajectory_in *in, const po_trajectory_out *out) {
    if (!trajectory_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing to sample: no launch, whatever the handle holds
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    po::DevTrajectory D{};
    D.B = in->B; D.N = in->N; D.K = p->K; D.D = p->n_discs; D.P = p->agent_pts; D.stride = p->agent_stride; D.flags = p->agent_flags;
    D.states = in->states; D.n_states = in->n_states; D.ok = in->ok; D.v = in->v; D.t = in->t;
    D.t0 = p->t0; D.dt = p->dt;
    for (int d = 0; d < p->n_discs; ++d) { D.off[d] = p->disc_offset[d]; D.rad[d] = p->disc_radius[d]; }
    D.status = out->status; D.o_states = out->states; D.o_v = out->v; D.o_a = out->a; D.o_t = out->t; D.index = out->index; D.first_held = out->first_held;
    D.agents = p->n_discs > 0 ? out->agents : nullptr;
    HIP_TRY(po_launch_trajectory(&D, h->stream));
    return PO_OK;
}

int po_trajectory_batch(po_handle h, const po_trajectory_params *p, const po_trajectory_in *in, const po_trajectory_out *out) {
    if (!trajectory_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing is staged, launched or written
    const size_t B = in->B, bn = B * (size_t)in->N, bk = B * (size_t)p->K;
    Stage S;
    const Slot<double> states = S.in(in->states, 5 * bn), v = S.in(in->v, bn), t = S.in(in->t, bn);
    const Slot<int> ns = S.in(in->n_states, B), ok = S.in(in->ok, B);
    const Slot<int> status = S.out(out->status, B), index = S.out_opt(out->index, bk), fh = S.out_opt(out->first_held, B);
    const Slot<double> os = S.out(out->states, 5 * bk), ov = S.out_opt(out->v, bk), oa = S.out_opt(out->a, bk), ot = S.out_opt(out->t, bk);
    const Slot<po_agent> agents = S.out_opt(p->n_discs > 0 ? out->agents : nullptr, B * (size_t)p->n_discs);
    return staged_call(h, S, &po_handle_s::post_buf, false, [&] {
        const po_trajectory_in d{in->B, in->N, states, ns, ok, v, t};
        const po_trajectory_out o{status, os, ov, oa, ot, index, fh, agents};
        return po_trajectory_batch_device(h, p, &d, &o);
    });
}

// ---- stop, wait, go: station-time plans that resume, sampled in time (po_stgo.hip) ---------------
void po_default_stgo_params(po_stgo_params *p) {
    if (!p) return;
    po_stplan_params s;
    po_default_stplan_params(&s);
    *p = po_stgo_params{s.dt, s.K, s.stride, s.U, s.margin, s.a_max, s.b_max, s.v_max, s.w_acc, s.w_slow, 0.0, 0.1, 81};  // a starting point nobody has tuned
}

// What both entries can check without reading through a pointer of the structs (testable without a GPU)
static bool stgo_args_ok(po_handle h, const po_stgo_params *p, const po_stgo_in *in, const po_stgo_out *out) {
    if (!h || !p || !in || !out || in->B < 0 || in->N < 0) return false;
    auto pos = [](double v) { return std::isfinite(v) && v > 0; };
    auto wgt = [](double v) { return std::isfinite(v) && v >= 0; };
    if (!pos(p->dt) || !pos(p->a_max) || !pos(p->b_max) || !pos(p->v_max) || !wgt(p->w_acc) || !wgt(p->w_slow) || !std::isfinite(p->margin)) return false;
    if (p->K < 1 || p->K > PO_ST_MAX_LAYERS || p->stride < 1 || p->U < 1 || p->U > PO_ST_MAX_STEP) return false;
    if (!std::isfinite(p->t0) || !pos(p->dts) || p->Q < 1) return false;
    if (!agent_lists_shape_ok(in->agents, in->B)) return false;
    const size_t B = in->B, bn = B * (size_t)in->N, bq = B * (size_t)p->Q;
    if (B > 0 && (!in->states || !in->v0 || !out->status || !out->states)) return false;
    // no output may overlap an input: byte ranges over the full extent of each array (B = 0: every extent is empty)
    struct Range { const void *p; size_t bytes; };
    const Range ins[] = {{in->states, 5 * bn * sizeof(double)}, {in->n_states, B * sizeof(int)}, {in->ok, B * sizeof(int)}, {in->v0, B * sizeof(double)},
                         {in->v_cap, bn * sizeof(double)}, {in->set_of, B * sizeof(int)}};
    const Range outs[] = {{out->status, B * sizeof(int)}, {out->ok_out, B * sizeof(int)}, {out->n_layers, B * sizeof(int)}, {out->cost, B * sizeof(double)},
                          {out->station, B * (PO_ST_MAX_LAYERS + 1) * sizeof(int)}, {out->cells, B * (size_t)p->K * PO_ST_MAX_STATIONS * sizeof(int)},
                          {out->n_resumes, B * sizeof(int)}, {out->states, 5 * bq * sizeof(double)}, {out->v, bq * sizeof(double)}, {out->a, bq * sizeof(double)},
                          {out->t, bq * sizeof(double)}, {out->index, bq * sizeof(int)}, {out->first_held, B * sizeof(int)}, {out->end, B * sizeof(int)}};
    for (const Range &o : outs)
        for (const Range &i : ins) {
            if (!o.p || !i.p || !o.bytes || !i.bytes) continue;
            const uintptr_t ob = (uintptr_t)o.p, ib = (uintptr_t)i.p;
            if (ob < ib + i.bytes && ib < ob + o.bytes) return false;
        }
    return true;
}

int po_stgo_batch_device(po_handle h, const po_stgo_params *p, const po_stgo_in *in, const po_stgo_out *out) {
    if (!stgo_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing to plan: no launch, whatever the handle holds
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    po::DevStgo D{};
    D.B = in->B; D.N = in->N; D.S = in->agents->S; D.n_agents = in->agents->n_agents;
    D.states = in->states; D.n_states = in->n_states; D.ok = in->ok; D.v0 = in->v0; D.v_cap = in->v_cap; D.set_of = in->set_of;
    D.agents = in->agents->agents; D.first = in->agents->first;
    D.dt = p->dt; D.K = p->K; D.stride = p->stride; D.U = p->U; D.margin = p->margin; D.a_max = p->a_max; D.b_max = p->b_max; D.v_max = p->v_max;
    D.w_acc = p->w_acc; D.w_slow = p->w_slow; D.t0 = p->t0; D.dts = p->dts; D.Q = p->Q;
    const int mb = in->N > 0 ? (in->N - 1) / p->stride + 1 : 1;  // no path of the call has more stations: the LDS is sized from it
    D.Mb = mb > PO_ST_MAX_STATIONS ? PO_ST_MAX_STATIONS : mb;
    D.status = out->status; D.ok_out = out->ok_out; D.n_layers = out->n_layers; D.cost = out->cost; D.station = out->station; D.cells = out->cells;
    D.n_resumes = out->n_resumes; D.o_states = out->states; D.o_v = out->v; D.o_a = out->a; D.o_t = out->t; D.index = out->index;
    D.first_held = out->first_held; D.end = out->end;
    const po::DevCar car = make_car(h->params);
    HIP_TRY(po_launch_stgo(&car, &D, h->stream));
    return PO_OK;
}

int po_stgo_batch(po_handle h, const po_stgo_params *p, const po_stgo_in *in, const po_stgo_out *out) {
    if (!stgo_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing is staged, launched or written
    if (!agent_lists_host_ok(in->agents, in->set_of, in->B)) return PO_ERR_INVALID;
    const size_t B = in->B, bn = B * (size_t)in->N, bq = B * (size_t)p->Q;
    Stage S;
    const Slot<double> states = S.in(in->states, 5 * bn), v0 = S.in(in->v0, B), cap = S.in(in->v_cap, bn);
    const Slot<int> ns = S.in(in->n_states, B), ok = S.in(in->ok, B), set_of = S.in(in->set_of, B);
    StagedAgents ag;
    stage_agent_lists(S, in->agents, &ag);
    const Slot<int> status = S.out(out->status, B), ok_out = S.out_opt(out->ok_out, B), nl = S.out_opt(out->n_layers, B), nres = S.out_opt(out->n_resumes, B);
    const Slot<int> station = S.out_opt(out->station, B * (PO_ST_MAX_LAYERS + 1)), cells = S.out_opt(out->cells, B * (size_t)p->K * PO_ST_MAX_STATIONS);
    const Slot<int> index = S.out_opt(out->index, bq), fh = S.out_opt(out->first_held, B), end = S.out_opt(out->end, B);
    const Slot<double> cost = S.out_opt(out->cost, B), os = S.out(out->states, 5 * bq), ov = S.out_opt(out->v, bq), oa = S.out_opt(out->a, bq), ot = S.out_opt(out->t, bq);
    return staged_call(h, S, &po_handle_s::post_buf, false, [&] {
        const po_agent_lists dl = ag.dev(in->agents);
        const po_stgo_in d{in->B, in->N, states, ns, ok, v0, cap, set_of, &dl};
        const po_stgo_out o{status, ok_out, nl, cost, station, cells, nres, os, ov, oa, ot, index, fh, end};
        return po_stgo_batch_device(h, p, &d, &o);
    });
}

// ---- speed QP: a jerk-limited s(t) inside a plan's tunnel (po_speedqp.hip) -----------------------
void po_default_speedqp_params(po_speedqp_params *p) {
    if (!p) return;
    po_stgo_params g;
    po_default_stgo_params(&g);
    *p = po_speedqp_params{g.dt, g.K, g.stride, g.v_max, g.dts, g.Q, 2.0, 3.0, 4.0, 1.0, 1.0, 1.0, 0.1, 1e-6, 1.6, 1e-4, 1e-4, 2000, 25, 1};  // a starting point nobody has tuned
}

// What both entries can check without reading through a pointer of the structs (testable without a GPU)
static bool speedqp_args_ok(po_handle h, const po_speedqp_params *p, const po_speedqp_in *in, const po_speedqp_out *out) {
    if (!h || !p || !in || !out || in->B < 0 || in->N < 0) return false;
    auto pos = [](double v) { return std::isfinite(v) && v > 0; };
    auto wgt = [](double v) { return std::isfinite(v) && v >= 0; };
    if (!pos(p->dt) || !pos(p->v_max) || !pos(p->dts) || !pos(p->a_max) || !pos(p->b_max) || !pos(p->j_max) || !pos(p->rho) || !pos(p->sigma)) return false;
    if (p->K < 1 || p->K > PO_ST_MAX_LAYERS || p->stride < 1 || p->Q < 2 || p->Q > PO_SQP_MAX_SAMPLES) return false;
    if (!wgt(p->w_s) || !wgt(p->w_a) || !wgt(p->w_j) || !(p->w_s + p->w_a + p->w_j > 0)) return false;
    if (!(p->alpha > 0 && p->alpha < 2) || !wgt(p->eps_abs) || !wgt(p->eps_rel)) return false;
    if (p->max_iter < 1 || p->check_every < 1 || (p->adaptive_rho != 0 && p->adaptive_rho != 1)) return false;
    const size_t B = in->B, bn = B * (size_t)in->N, bq = B * (size_t)p->Q;
    if (B > 0 && (!in->states || !in->v0 || !in->station || !in->n_layers || !in->ref_states || !out->status || !out->states)) return false;
    // no output may overlap an input: byte ranges over the full extent of each array (B = 0: every extent is empty)
    struct Range { const void *p; size_t bytes; };
    const Range ins[] = {{in->states, 5 * bn * sizeof(double)}, {in->n_states, B * sizeof(int)}, {in->ok, B * sizeof(int)}, {in->v0, B * sizeof(double)},
                         {in->v_cap, bn * sizeof(double)}, {in->station, B * (PO_ST_MAX_LAYERS + 1) * sizeof(int)}, {in->n_layers, B * sizeof(int)},
                         {in->cells, B * (size_t)p->K * PO_ST_MAX_STATIONS * sizeof(int)}, {in->ref_states, 5 * bq * sizeof(double)}};
    const Range outs[] = {{out->status, B * sizeof(int)}, {out->iters, B * sizeof(int)}, {out->n_fact, B * sizeof(int)}, {out->r_prim, B * sizeof(double)},
                          {out->r_dual, B * sizeof(double)}, {out->n_q, B * sizeof(int)}, {out->states, 5 * bq * sizeof(double)}, {out->v, bq * sizeof(double)},
                          {out->a, bq * sizeof(double)}, {out->jerk, bq * sizeof(double)}, {out->t, bq * sizeof(double)}, {out->lo, bq * sizeof(double)},
                          {out->hi, bq * sizeof(double)}, {out->index, bq * sizeof(int)}};
    for (const Range &o : outs)
        for (const Range &i : ins) {
            if (!o.p || !i.p || !o.bytes || !i.bytes) continue;
            const uintptr_t ob = (uintptr_t)o.p, ib = (uintptr_t)i.p;
            if (ob < ib + i.bytes && ib < ob + o.bytes) return false;
        }
    return true;
}

int po_speedqp_batch_device(po_handle h, const po_speedqp_params *p, const po_speedqp_in *in, const po_speedqp_out *out) {
    if (!speedqp_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing to solve: no launch, whatever the handle holds
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    po::DevSpeedQp D{};
    D.B = in->B; D.N = in->N; D.K = p->K; D.stride = p->stride; D.Q = p->Q;
    D.dt = p->dt; D.v_max = p->v_max; D.dts = p->dts; D.a_max = p->a_max; D.b_max = p->b_max; D.j_max = p->j_max; D.w_s = p->w_s; D.w_a = p->w_a; D.w_j = p->w_j;
    D.rho = p->rho; D.sigma = p->sigma; D.alpha = p->alpha; D.eps_abs = p->eps_abs; D.eps_rel = p->eps_rel;
    D.max_iter = p->max_iter; D.check_every = p->check_every; D.adaptive_rho = p->adaptive_rho;
    D.states = in->states; D.n_states = in->n_states; D.ok = in->ok; D.v0 = in->v0; D.v_cap = in->v_cap; D.station = in->station; D.n_layers = in->n_layers;
    D.cells = in->cells; D.ref_states = in->ref_states;
    D.status = out->status; D.iters = out->iters; D.n_fact = out->n_fact; D.r_prim = out->r_prim; D.r_dual = out->r_dual; D.n_q = out->n_q;
    D.o_states = out->states; D.o_v = out->v; D.o_a = out->a; D.o_jerk = out->jerk; D.o_t = out->t; D.o_lo = out->lo; D.o_hi = out->hi; D.index = out->index;
    HIP_TRY(po_launch_speedqp(&D, h->stream));
    return PO_OK;
}

int po_speedqp_batch(po_handle h, const po_speedqp_params *p, const po_speedqp_in *in, const po_speedqp_out *out) {
    if (!speedqp_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing is staged, launched or written
    const size_t B = in->B, bn = B * (size_t)in->N, bq = B * (size_t)p->Q, W = PO_ST_MAX_LAYERS + 1;
    for (size_t b = 0; b < B; ++b) {  // the plan as the host entry takes it: in range (the device entry reads it clamped)
        const int nl = in->n_layers[b];
        if (nl < 0 || nl > p->K) return PO_ERR_INVALID;
        for (int k = 0; nl >= 1 && k <= nl; ++k)
            if (in->station[b * W + k] < 0 || in->station[b * W + k] > PO_ST_MAX_STATIONS - 1) return PO_ERR_INVALID;
    }
    Stage S;
    const Slot<double> states = S.in(in->states, 5 * bn), v0 = S.in(in->v0, B), cap = S.in(in->v_cap, bn), ref = S.in(in->ref_states, 5 * bq);
    const Slot<int> ns = S.in(in->n_states, B), ok = S.in(in->ok, B), station = S.in(in->station, B * W), nl = S.in(in->n_layers, B);
    const Slot<int> cells = S.in(in->cells, B * (size_t)p->K * PO_ST_MAX_STATIONS);
    const Slot<int> status = S.out(out->status, B), iters = S.out_opt(out->iters, B), nf = S.out_opt(out->n_fact, B), nq = S.out_opt(out->n_q, B);
    const Slot<int> index = S.out_opt(out->index, bq);
    const Slot<double> rp = S.out_opt(out->r_prim, B), rd = S.out_opt(out->r_dual, B), os = S.out(out->states, 5 * bq), ov = S.out_opt(out->v, bq);
    const Slot<double> oa = S.out_opt(out->a, bq), oj = S.out_opt(out->jerk, bq), ot = S.out_opt(out->t, bq), lo = S.out_opt(out->lo, bq), hi = S.out_opt(out->hi, bq);
    return staged_call(h, S, &po_handle_s::post_buf, false, [&] {
        const po_speedqp_in d{in->B, in->N, states, ns, ok, v0, cap, station, nl, cells, ref};
        const po_speedqp_out o{status, iters, nf, rp, rd, nq, os, ov, oa, oj, ot, lo, hi, index};
        return po_speedqp_batch_device(h, p, &d, &o);
    });
}

// ---- agent sets (po_agentsets.hip) ----------------------------------------------------------------
void po_default_agentsets_params(po_agentsets_params *p) {
    if (!p) return;
    *p = po_agentsets_params{5.0, 0.0, 0.0, 0.0, 8.0, 0};  // a starting point nobody has tuned
}

// Source 1 is optional: NULL, or a list with no pool or no record, contributes nothing (and then none of its pointers is looked at)
static bool agentsets_src1_used(const po_agent_lists *L) { return L && L->S > 0 && L->n_agents > 0; }

// What both entries can check without reading through a pointer of the structs (testable without a GPU)
static bool agentsets_args_ok(po_handle h, const po_agentsets_params *p, const po_agentsets_in *in, const po_agentsets_out *out) {
    if (!h || !p || !in || !out || in->B < 0 || in->N < 0 || out->capacity < 0 || p->owner_div < 0) return false;
    auto room = [](double v) { return std::isfinite(v) && v >= 0; };
    if (!room(p->reach) || !room(p->t_before) || !room(p->t_after) || !std::isfinite(p->win_lo) || !std::isfinite(p->win_hi) || !(p->win_lo <= p->win_hi)) return false;
    const po_agent_lists *L0 = in->src[0], *L1 = in->src[1];
    if (!agent_lists_shape_ok(L0, in->B)) return false;
    if (!agent_lists_shape_ok(L1, 0) || (agentsets_src1_used(L1) && !agent_lists_shape_ok(L1, in->B))) return false;
    if (L0 && agentsets_src1_used(L1) && (long long)L0->n_agents + L1->n_agents > std::numeric_limits<int>::max()) return false;  // src_index is an int
    if (in->B > 0 && (!in->states || !out->first || !out->count || !out->status || (out->capacity > 0 && !out->agents))) return false;
    // out->agents may not overlap a source array: byte ranges over the full extent of each
    for (const po_agent_lists *L : {L0, L1}) {
        if (!L || !L->agents || L->n_agents <= 0 || !out->agents || out->capacity <= 0) continue;
        const uintptr_t ob = (uintptr_t)out->agents, ib = (uintptr_t)L->agents;
        if (ob < ib + (size_t)L->n_agents * sizeof(po_agent) && ib < ob + (size_t)out->capacity * sizeof(po_agent)) return false;
    }
    return true;
}

int po_agentsets_batch_device(po_handle h, const po_agentsets_params *p, const po_agentsets_in *in, const po_agentsets_out *out) {
    if (!agentsets_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing to compose: no launch, whatever the handle holds
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    po::DevAgentSets D{};
    D.B = in->B; D.N = in->N; D.capacity = out->capacity; D.owner_div = p->owner_div;
    D.states = in->states; D.n_states = in->n_states; D.ok = in->ok; D.t = in->t; D.pool_of = in->pool_of; D.owner = in->owner;
    for (int s = 0; s < PO_SETS_SOURCES; ++s) {
        const po_agent_lists *L = in->src[s];
        if (s == 1 && !agentsets_src1_used(L)) continue;  // S = 0: the kernels skip the source
        D.agents[s] = L->agents; D.first[s] = L->first; D.n_agents[s] = L->n_agents; D.S[s] = L->S;
    }
    D.reach = p->reach; D.t_before = p->t_before; D.t_after = p->t_after; D.win_lo = p->win_lo; D.win_hi = p->win_hi;
    D.o_agents = out->agents; D.o_first = out->first; D.count = out->count; D.status = out->status; D.o_set_of = out->set_of; D.src_index = out->src_index;
    D.total = out->total;
    HIP_TRY(po_launch_agentsets(&D, h->stream));
    return PO_OK;
}

int po_agentsets_batch(po_handle h, const po_agentsets_params *p, const po_agentsets_in *in, const po_agentsets_out *out) {
    if (!agentsets_args_ok(h, p, in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;  // nothing is staged, launched or written
    const bool two = agentsets_src1_used(in->src[1]);
    if (!agent_lists_host_ok(in->src[0], in->pool_of, in->B) || (two && !agent_lists_host_ok(in->src[1], in->pool_of, in->B))) return PO_ERR_INVALID;
    const size_t B = in->B, bn = B * (size_t)in->N, cap = (size_t)out->capacity;
    Stage S;
    const Slot<double> states = S.in(in->states, 5 * bn), t = S.in(in->t, bn);
    const Slot<int> ns = S.in(in->n_states, B), ok = S.in(in->ok, B), pool = S.in(in->pool_of, B), owner = S.in(in->owner, (size_t)in->src[0]->n_agents);
    StagedAgents ag[PO_SETS_SOURCES];
    stage_agent_lists(S, in->src[0], &ag[0]);
    if (two) stage_agent_lists(S, in->src[1], &ag[1]);
    // agents and src_index are written up to first[B] only: they travel in both directions, so the slots behind keep the caller's bytes
    const Slot<po_agent> agents = S.inout(cap > 0 ? out->agents : nullptr, cap);
    const Slot<int> sidx = S.inout(cap > 0 ? out->src_index : nullptr, cap);
    const Slot<int> first = S.out(out->first, B + 1), count = S.out(out->count, B), status = S.out(out->status, B), set_of = S.out_opt(out->set_of, B);
    const Slot<long long> total = S.out_opt(out->total, 1);
    return staged_call(h, S, &po_handle_s::post_buf, false, [&] {
        const po_agent_lists d0 = ag[0].dev(in->src[0]), d1 = two ? ag[1].dev(in->src[1]) : po_agent_lists{};
        const po_agentsets_in d{in->B, in->N, states, ns, ok, t, {&d0, two ? &d1 : nullptr}, pool, owner};
        const po_agentsets_out o{out->capacity, agents, first, count, status, set_of, sidx, total};
        return po_agentsets_batch_device(h, p, &d, &o);
    });
}

// ---- corridor-bounds producer ------------------------------------------------------------------------------------
static bool bounds_args_ok(po_handle h, const po_bounds_in *in, const double *bounds, const int *n_valid) {
    if (!h || !in || in->B < 0 || in->N < 1 || in->K < 3) return false;
    return in->B == 0 || (in->ref_x && in->ref_y && in->ref_z && in->ref_s && in->knot_s && in->knot_x && in->knot_y && bounds && n_valid);
}

int po_bounds_batch_device(po_handle h, const po_bounds_in *in, double *bounds, int *n_valid) {
    if (!bounds_args_ok(h, in, bounds, n_valid)) return PO_ERR_INVALID;
    Lock g(h->mu);
    if (!h->maps.d || !assignment_covers(h, in->B)) return PO_ERR_INVALID;  // po_set_map first; an assignment covers every instance
    if (in->B == 0) return PO_OK;
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = h->coef_buf.ensure(sizeof(double) * (size_t)in->B * 2 * 6 * in->K)) return rc;
    po::DevBounds D{};
    D.B = in->B; D.N = in->N; D.K = in->K;
    D.ref_x = in->ref_x; D.ref_y = in->ref_y; D.ref_z = in->ref_z; D.ref_s = in->ref_s; D.n_points = in->n_points;
    D.knot_s = in->knot_s; D.knot_x = in->knot_x; D.knot_y = in->knot_y; D.n_knots = in->n_knots;
    const po_params &p = h->params;
    for (int j = 0; j < 4; ++j) D.d[j] = p.d[j];
    D.radius = std::sqrt((p.car_length / 8) * (p.car_length / 8) + (p.car_width / 2) * (p.car_width / 2)) + p.safety_margin;  // planning_flags.cpp:9
    D.coef = static_cast<double *>(h->coef_buf.p);
    HIP_TRY(po_launch_bounds(&h->maps, &D, bounds, n_valid, h->stream));
    return PO_OK;
}

int po_bounds_batch(po_handle h, const po_bounds_in *in, double *bounds, int *n_valid) {
    if (!bounds_args_ok(h, in, bounds, n_valid)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;
    const size_t B = in->B, bn = B * in->N, bk = B * in->K;
    Stage S;
    const Slot<double> rx = S.in(in->ref_x, bn), ry = S.in(in->ref_y, bn), rz = S.in(in->ref_z, bn), rs = S.in(in->ref_s, bn);
    const Slot<double> ks = S.in(in->knot_s, bk), kx = S.in(in->knot_x, bk), ky = S.in(in->knot_y, bk);
    const Slot<int> np = S.in(in->n_points, B), nk = S.in(in->n_knots, B);
    const Slot<double> d_bounds = S.out(bounds, 8 * bn);
    const Slot<int> d_nvalid = S.out(n_valid, B);
    return staged_call(h, S, &po_handle_s::bnd_buf, false, [&] {
        const po_bounds_in d{in->B, in->N, in->K, rx, ry, rz, rs, np, ks, kx, ky, nk};
        return po_bounds_batch_device(h, &d, d_bounds, d_nvalid);
    });
}

// ---- reference-smoothing QPs -----------------------------------------------------------------------
int po_smooth_dims(int kind, int P, int *n, int *m) {
    int nn, mm;
    if (kind == PO_SMOOTH_TENSION2) { if (P < 3) return PO_ERR_INVALID; nn = 4 * P - 1; mm = 3 * (P - 1) + 2; }  // tension_smoother_2.cpp:177-178
    else if (kind == PO_SMOOTH_TENSION) { if (P < 3) return PO_ERR_INVALID; nn = 3 * P; mm = 3 * P; }            // tension_smoother.cpp:201-202
    else if (kind == PO_SMOOTH_POST) { if (P < 4) return PO_ERR_INVALID; nn = 3 * P; mm = 3 * P - 2; }           // reference_path_smoother.cpp:536,544-545
    else return PO_ERR_INVALID;
    if (n) *n = nn;
    if (m) *m = mm;
    return PO_OK;
}

static int smooth_args_ok(const po_smooth_in *in, const po_smooth_out *out) {
    if (!in || !out || in->B < 0) return 0;
    if (po_smooth_dims(in->kind, in->P, nullptr, nullptr)) return 0;
    if (in->B == 0) return 1;
    if (!in->s || !out->x || !out->info) return 0;
    if (in->kind == PO_SMOOTH_POST) return in->lb && in->ub && in->l0;
    return in->x && in->y && in->angle && in->k && out->y && out->s;
}

int po_smooth_batch_device(po_handle h, const po_smooth_in *in, const po_smooth_out *out) {
    if (!h || !smooth_args_ok(in, out)) return PO_ERR_INVALID;
    Lock g(h->mu);
    if (in->kind == PO_SMOOTH_TENSION && (!h->maps.d || !assignment_covers(h, in->B))) return PO_ERR_INVALID;  // po_set_map first (clearance of every point)
    if (in->B == 0) return PO_OK;
    if (po_smooth_lds_bytes(in->kind, in->P) > 160 * 1024) return PO_ERR_UNSUPPORTED;
    HIP_TRY(hipSetDevice(h->device));
    po::DevSmooth D{};
    D.kind = in->kind; D.B = in->B; D.P = in->P; D.n_points = in->n_points;
    D.x = in->x; D.y = in->y; D.angle = in->angle; D.k = in->k; D.s = in->s; D.lb = in->lb; D.ub = in->ub; D.l0 = in->l0;
    D.out_x = out->x; D.out_y = out->y; D.out_s = out->s; D.info = out->info; D.raw = out->raw;
    int nmax = 0;
    po_smooth_dims(in->kind, in->P, &nmax, nullptr);
    D.raw_stride = nmax;
    const po_params &p = h->params;
    const double w[6] = {p.t2_w_dev, p.t2_w_curv, p.t2_w_curv_rate, p.cart_w_curv, p.cart_w_curv_rate, p.cart_w_dev};
    for (int i = 0; i < 6; ++i) D.w[i] = w[i];
    D.sigma = p.sigma; D.alpha = p.alpha; D.rho0 = p.rho0; D.eps_abs = p.eps_abs; D.eps_rel = p.eps_rel;
    D.eps_pinf = p.eps_prim_inf; D.eps_dinf = p.eps_dual_inf; D.adapt_tol = p.adapt_tol;
    D.max_iter = p.max_iter; D.check_every = p.check_every; D.adapt_every = p.adapt_every; D.scaling = p.scaling;
    D.scratch_stride = po_smooth_scratch_doubles(in->kind, in->P);
    if (int rc = h->smooth_buf.ensure(sizeof(double) * D.scratch_stride * (size_t)in->B)) return rc;
    D.scratch = static_cast<double *>(h->smooth_buf.p);
    D.maps = h->maps;
    D.perm_bits = 0;
    D.seq_band = h->env_smooth_seq ? 1 : 0; D.waves = h->env_smooth_waves; D.nopad = h->env_smooth_nopad ? 1 : 0;  // developer A/B switches (read once at po_create)
    if (!h->env_identity && in->B > 8)
        while ((1 << D.perm_bits) < in->B) ++D.perm_bits;
    const bool dbg = h->env_smooth_debug;  // dev tool: per-phase cycle totals of instance 0..B-1 printed to stderr
    if (dbg) {
        if (int rc = h->dbg_buf.ensure(sizeof(long long) * 8 * (size_t)in->B)) return rc;
        D.dbg_cycles = static_cast<long long *>(h->dbg_buf.p);
    }
    if (h->timed) HIP_TRY(hipEventRecord(h->ev0, h->stream));
    HIP_TRY(po_launch_smooth(&D, &h->smooth_variant_used, h->stream));
    if (dbg) {
        std::vector<long long> hc(8 * (size_t)in->B);
        HIP_TRY(hipMemcpyAsync(hc.data(), D.dbg_cycles, sizeof(long long) * hc.size(), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        double tot[8] = {0};
        for (int b = 0; b < in->B; ++b) for (int i = 0; i < 8; ++i) tot[i] += (double)hc[8 * (size_t)b + i];
        std::fprintf(stderr, "po_smooth kind %d: mean cycles/instance setup %.0f factor %.0f rhs %.0f solve %.0f update %.0f check %.0f out %.0f\n", in->kind,
                     tot[0] / in->B, tot[1] / in->B, tot[2] / in->B, tot[3] / in->B, tot[4] / in->B, tot[5] / in->B, tot[6] / in->B);
    }
    if (h->timed) HIP_TRY(hipEventRecord(h->ev1, h->stream));
    return PO_OK;
}

int po_smooth_batch(po_handle h, const po_smooth_in *in, const po_smooth_out *out) {
    if (!h || !smooth_args_ok(in, out)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;
    int nmax = 0;
    po_smooth_dims(in->kind, in->P, &nmax, nullptr);
    const size_t B = in->B, np = B * in->P;
    Stage S;
    const Slot<double> x = S.in(in->x, np), y = S.in(in->y, np), angle = S.in(in->angle, np), k = S.in(in->k, np), s = S.in(in->s, np);
    const Slot<double> lb = S.in(in->lb, np), ub = S.in(in->ub, np), l0 = S.in(in->l0, B);
    const Slot<int> n_points = S.in(in->n_points, B);
    // y / s: the device arrays always exist and the kernel writes them (a null host pointer only skips the copy back); raw: not wanted = not declared, the kernel skips it
    const Slot<double> ox = S.out(out->x, np), oy = S.out(out->y, np), os = S.out(out->s, np);
    const Slot<po_info> oinfo = S.out(out->info, B);
    const Slot<double> oraw = S.out_opt(out->raw, B * (size_t)nmax);
    return staged_call(h, S, &po_handle_s::smooth_io, false, [&] {
        const po_smooth_in d{in->kind, in->B, in->P, n_points, x, y, angle, k, s, lb, ub, l0};
        const po_smooth_out dout{ox, oy, os, oinfo, oraw};
        return po_smooth_batch_device(h, &d, &dout);
    });
}

// ---- reference re-sampling, limits, DP lattice search -----------------------------------------------
static bool resample_args_ok(po_handle h, const po_spline_in *in, int N, const double *ref_x, const double *ref_y, const double *ref_z, const double *ref_k,
                             const double *ref_s, const int *n_points) {
    return h && spline_args_ok(in) && N >= 1 && (in->B == 0 || (ref_x && ref_y && ref_z && ref_k && ref_s && n_points));
}
static bool limits_args_ok(po_handle h, int B, int N, const double *v, const double *a, const double *max_k, const double *max_kp) {
    return h && B >= 0 && N >= 1 && (B == 0 || (v && a && max_k && max_kp));
}
static bool dp_search_args_ok(po_handle h, const po_spline_in *in, const double *start, int L, const double *layer_s, const double *lb, const double *ub,
                              const double *l0, const int *n_layers) {
    return h && spline_args_ok(in) && L >= 1 && (in->B == 0 || (start && layer_s && lb && ub && l0 && n_layers));
}

int po_resample_batch_device(po_handle h, const po_spline_in *in, double ds_smaller, double ds_larger, int N, double *ref_x, double *ref_y,
                             double *ref_z, double *ref_k, double *ref_s, int *n_points) {
    if (!resample_args_ok(h, in, N, ref_x, ref_y, ref_z, ref_k, ref_s, n_points)) return PO_ERR_INVALID;
    if (!(ds_smaller <= ds_larger) || !(ds_smaller > 0)) return PO_ERR_INVALID;  // CHECK_LE(delta_s_smaller, delta_s_larger)
    if (in->B == 0) return PO_OK;
    if (po_spline_lds_bytes(in->K) > 64 * 1024) return PO_ERR_UNSUPPORTED;
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    const po::DevSpline D = make_dev_spline(in);
    po::DevResample R{ds_smaller, ds_larger, h->params.enable_dynamic_segmentation, N, ref_x, ref_y, ref_z, ref_k, ref_s, n_points};
    HIP_TRY(po_launch_resample(&D, &R, h->stream));
    return PO_OK;
}

int po_limits_batch_device(po_handle h, int B, int N, const int *n_points, const double *v, const double *a, double *max_k, double *max_kp) {
    if (!limits_args_ok(h, B, N, v, a, max_k, max_kp)) return PO_ERR_INVALID;
    if (B == 0) return PO_OK;
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(po_launch_limits(B, N, n_points, v, a, max_k, max_kp, h->params.mu, h->params.max_curvature_rate, h->stream));
    return PO_OK;
}

int po_dp_search_batch_device(po_handle h, const po_spline_in *in, const double *start, int L, double *layer_s, double *lb, double *ub, double *l0,
                              int *n_layers) {
    if (!dp_search_args_ok(h, in, start, L, layer_s, lb, ub, l0, n_layers)) return PO_ERR_INVALID;
    const po_params &p = h->params;
    if (!(p.search_lat_spacing > 0) || !(p.search_long_spacing > 0) || !(p.search_lateral_range > 0) ||
        2 * p.search_lateral_range / p.search_lat_spacing + 1 > 64) return PO_ERR_UNSUPPORTED;  // one wave per path: <= 64 lateral samples
    Lock g(h->mu);
    if (!h->maps.d || !assignment_covers(h, in->B)) return PO_ERR_INVALID;  // po_set_map first; an assignment covers every instance
    if (in->B == 0) return PO_OK;
    if (po_dp_lds_bytes(in->K, L) > 160 * 1024) return PO_ERR_UNSUPPORTED;
    HIP_TRY(hipSetDevice(h->device));
    const po::DevSpline D = make_dev_spline(in);
    po::DevSearch Q{p.search_lateral_range, p.search_long_spacing, p.search_lat_spacing, start, L, layer_s, lb, ub, l0, n_layers};
    HIP_TRY(po_launch_dp_search(&h->maps, &D, &Q, h->env_dp_one_wave ? 1 : 0, &h->dp_waves_used, h->stream));
    return PO_OK;
}

// host-pointer wrappers: stage the spline batch, run the device entry, copy back
namespace {
struct StagedSpline {
    Slot<double> s, x, y, length;
    Slot<int> n_knots;
    po_spline_in dev(const po_spline_in *in) const { return po_spline_in{in->B, in->K, s, x, y, n_knots, length}; }  // (once the block is reserved)
};
void stage_spline_batch(Stage &S, const po_spline_in *in, StagedSpline *q) {  // declares the arrays of a po_spline_in on S
    const size_t B = in->B, bk = B * in->K;
    q->s = S.in(in->knot_s, bk); q->x = S.in(in->knot_x, bk); q->y = S.in(in->knot_y, bk); q->length = S.in(in->length, B); q->n_knots = S.in(in->n_knots, B);
}
}  // namespace

int po_resample_batch(po_handle h, const po_spline_in *in, double ds_smaller, double ds_larger, int N, double *ref_x, double *ref_y, double *ref_z,
                      double *ref_k, double *ref_s, int *n_points) {
    if (!resample_args_ok(h, in, N, ref_x, ref_y, ref_z, ref_k, ref_s, n_points)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;
    const size_t B = in->B, bn = B * N;
    Stage S;
    StagedSpline sp;
    stage_spline_batch(S, in, &sp);
    const Slot<double> x = S.out(ref_x, bn), y = S.out(ref_y, bn), z = S.out(ref_z, bn), k = S.out(ref_k, bn), s = S.out(ref_s, bn);
    const Slot<int> np = S.out(n_points, B);
    return staged_call(h, S, &po_handle_s::plan_io, false, [&] {
        const po_spline_in d = sp.dev(in);
        return po_resample_batch_device(h, &d, ds_smaller, ds_larger, N, x, y, z, k, s, np);
    });
}

int po_limits_batch(po_handle h, int B, int N, const int *n_points, const double *v, const double *a, double *max_k, double *max_kp) {
    if (!limits_args_ok(h, B, N, v, a, max_k, max_kp)) return PO_ERR_INVALID;
    if (B == 0) return PO_OK;
    const size_t bn = (size_t)B * N;
    Stage S;
    const Slot<double> d_v = S.in(v, bn), d_a = S.in(a, bn), d_k = S.out(max_k, bn), d_kp = S.out(max_kp, bn);
    const Slot<int> d_np = S.in(n_points, B);
    return staged_call(h, S, &po_handle_s::plan_io, false, [&] { return po_limits_batch_device(h, B, N, d_np, d_v, d_a, d_k, d_kp); });
}

int po_dp_search_batch(po_handle h, const po_spline_in *in, const double *start, int L, double *layer_s, double *lb, double *ub, double *l0, int *n_layers) {
    if (!dp_search_args_ok(h, in, start, L, layer_s, lb, ub, l0, n_layers)) return PO_ERR_INVALID;
    if (in->B == 0) return PO_OK;
    const size_t B = in->B, bl = B * L;
    Stage S;
    StagedSpline sp;
    stage_spline_batch(S, in, &sp);
    const Slot<double> d_start = S.in(start, 3 * B);
    const Slot<double> d_s = S.out(layer_s, bl), d_lb = S.out(lb, bl), d_ub = S.out(ub, bl), d_l0 = S.out(l0, B);
    const Slot<int> d_n = S.out(n_layers, B);
    return staged_call(h, S, &po_handle_s::plan_io, false, [&] {
        const po_spline_in d = sp.dev(in);
        return po_dp_search_batch_device(h, &d, d_start, L, d_s, d_lb, d_ub, d_l0, d_n);
    });
}

int po_map_sample_layer(po_handle h, int k, int n, const double *xy, double *dist, int *inside) {
    if (!h || n < 0 || (n > 0 && (!xy || !dist || !inside))) return PO_ERR_INVALID;
    Lock call(h->call_mu);  // (post_buf is the staging block of po_postcheck_batch / po_densify_batch too)
    Lock g(h->mu);
    if (!h->maps.d || k < 0 || k >= h->maps.M) return PO_ERR_INVALID;
    if (n == 0) return PO_OK;
    HIP_TRY(hipSetDevice(h->device));
    Stage S;
    const Slot<double> d_xy = S.in(xy, 2 * (size_t)n), d_dist = S.out(dist, n);
    const Slot<int> d_inside = S.out(inside, n);
    PO_TRY(S.upload(h, h->post_buf));
    HIP_TRY(po_launch_map_sample(&h->maps, k, n, d_xy, d_dist, d_inside, h->stream));
    return S.copy_out(h);
}

int po_map_sample(po_handle h, int n, const double *xy, double *dist, int *inside) { return po_map_sample_layer(h, 0, n, xy, dist, inside); }

const char *po_strerror(int code) {
    switch (code) {
        case PO_OK: return "ok";
        case PO_ERR_INVALID: return "invalid argument";
        case PO_ERR_HIP: return "HIP runtime error (see po_last_hip_error)";
        case PO_ERR_UNSUPPORTED: return "unsupported configuration (path too long for the on-chip tile)";
        case PO_ERR_NOMEM: return "out of memory";
        default: return "unknown error";
    }
}
const char *po_last_hip_error(void) { return g_hip_err.c_str(); }
#define PO_STR2(x) #x
#define PO_STR(x) PO_STR2(x)
const char *po_version(void) { return "po_hip " PO_STR(PO_ABI_VERSION) " (gfx950)"; }

}  // extern "C"
