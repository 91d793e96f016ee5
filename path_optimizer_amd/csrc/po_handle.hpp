// po_handle.hpp — what the host files of libpo_hip.so (po_capi.cpp, po_solve.cpp, po_plan.cpp) share: error plumbing, the owning buffers, the annotated locks, the handle, the
// staging helper of the host-pointer entries (Stage), the one staged call they all make and the spline argument check.  Private: not part of include/po_hip.h, and
// nothing here is exported (hidden visibility).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/po_hip.h"
#include "po_launch.hpp"
#include "po_map.hpp"

#pragma GCC visibility push(hidden)

bool hip_ok(hipError_t e, const char *what);  // po_capi.cpp: false + the text po_last_hip_error() returns
#define HIP_TRY(x)                                   \
    do {                                             \
        if (!hip_ok((x), #x)) return PO_ERR_HIP;     \
    } while (0)
#define PO_TRY(x)                     \
    do {                              \
        const int rc_ = (x);          \
        if (rc_ != PO_OK) return rc_; \
    } while (0)

// The handle's resources own what they hold and are not copyable: po_handle_s releases them member by member, in reverse order of declaration.
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};
struct Stream : NoCopy {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
};
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};
struct DevBuf : NoCopy {  // grow-only device buffer
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return PO_OK;
        release();
        if (!hip_ok(hipMalloc(&p, bytes), "hipMalloc")) return PO_ERR_NOMEM;
        cap = bytes;
        return PO_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    ~DevBuf() { release(); }
};
struct HostBuf : NoCopy {  // grow-only PINNED host buffer (hipHostMalloc): the staging area of the host-pointer entry — DMA engines read / write it directly,
                           // so the H2D / D2H copies run at PCIe speed and asynchronously (a copy from pageable memory is staged by the runtime, synchronously)
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return PO_OK;
        release();
        if (!hip_ok(hipHostMalloc(&p, bytes, hipHostMallocDefault), "hipHostMalloc")) return PO_ERR_NOMEM;
        cap = bytes;
        return PO_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    ~HostBuf() { release(); }
};

// The locks, annotated for clang's thread-safety analysis (-Wthread-safety is an error for the host files: an unlocked access to a guarded member does not build).
#define PO_GUARDED_BY(m) __attribute__((guarded_by(m)))
#define PO_REQUIRES(m) __attribute__((requires_capability(m)))
#define PO_ACQUIRED_AFTER(m) __attribute__((acquired_after(m)))
class __attribute__((capability("mutex"))) Mutex : NoCopy {
    std::mutex m_;

public:
    void lock() __attribute__((acquire_capability())) { m_.lock(); }
    void unlock() __attribute__((release_capability())) { m_.unlock(); }
};
class __attribute__((scoped_lockable)) Lock : NoCopy {
    Mutex &m_;

public:
    explicit Lock(Mutex &m) __attribute__((acquire_capability(m))) : m_(m) { m_.lock(); }
    ~Lock() __attribute__((release_capability())) { m_.unlock(); }
};

struct po_handle_s {
    // Two locks, always taken in the order call_mu -> mu, and every member says which one guards it:
    // mu       guards whatever a device-pointer entry reads, writes or grows while it enqueues its launches: the stream, the map stack and the world, the developer
    //          switches, the read-backs and the timing record, and the scratch blocks of the device entries;
    // call_mu  is the CALL lock: every host-pointer entry (and po_plan_batch*, whose stages share the plan arena) holds it from before its first ensure() until its
    //          last read-back has been synchronised, so staging, launch and read-back of one call are atomic with respect to every other call on the handle.  It
    //          guards the blocks only those entries touch: the staging blocks and the plan arena.
    // No guard: what po_create sets and nothing changes afterwards (device, params, wave_slots, own_stream, the event handles).
    Mutex call_mu;
    Mutex mu PO_ACQUIRED_AFTER(call_mu);
    int device = 0;
    po_params params{};
    // Declared AHEAD of every buffer: members are destroyed in reverse order, so the buffers are freed first, then the events, the stream last
    // (po_destroy has set the device and synchronised the stream before).
    Stream own_stream;
    PO_GUARDED_BY(mu) hipStream_t stream = nullptr;
    Event ev0, ev1;
    Event evh[4];  // host-pointer entry: start, H2D done, (ev0 .. ev1 = the solve), D2H done; evh[3]: solve phase mark (po_last_phase_ms)
    Event evp[2];  // split scheduling (refine = 2): end of the warm-start launches, end of the Newton launch
    PO_GUARDED_BY(mu) bool timed = false, timed_host = false, timed_phases = false;
    PO_GUARDED_BY(mu) double host_pack_ms = 0.0, host_unpack_ms = 0.0;
    PO_GUARDED_BY(call_mu) HostBuf pin_in, pin_out;   // pinned staging of the host-pointer entry
    PO_GUARDED_BY(mu) int host_threads = 0;      // pack / unpack threads (0: min(8, hardware threads); po_debug_set "host_threads")
    PO_GUARDED_BY(mu) DevBuf pol_buf;  // per-lane ADMM state handed from the solve kernels to newton_kernel / polish_kernel (po_params.refine / polish)
    PO_GUARDED_BY(mu) DevBuf fb_buf;   // refine = 2: the work list of newton_fallback_kernel
    PO_GUARDED_BY(mu) DevBuf nw_state_buf, nw_idx_buf;  // sliced Newton launches: the parked paths' blocks; keys [B] + list [B + 1] (+ the constant-class kernels' lists)
    PO_GUARDED_BY(mu) bool nw_slice_forced = false;
    PO_GUARDED_BY(mu) int nw_last_B = 0;  // ... and the batch size of the last sliced solve (po_debug_get "newton_parked")
    int wave_slots = 1024;  // paths the device runs at a time (one wave per SIMD: 4 per CU); batches below two rounds of that are not sliced (no queueing tail to remove)
    PO_GUARDED_BY(mu) bool fixed_length = true;  // take the length-specialised kernels where the batch has one (po_debug_set "fixed_length"; 0: always the generic kernels).  Same results.
    PO_GUARDED_BY(mu) int fixed_used = 0;        // ... and whether the last solve ran them (po_debug_get "fixed_length_used")
    // ... with the standard row classes as compile-time constants in their Newton launches, for the paths that have those classes (po_debug_set "fixed_classes"; 0: the
    // kernels without the constants for every path).  Same results.  Their lists live in nw_idx_buf behind keys and list (std_lists, po_device.hpp); std_flag_at: where
    // in that block the last solve flagged the std_B paths they took (-1: it did not run them; po_debug_get "fixed_classes_used")
    PO_GUARDED_BY(mu) bool fixed_classes = true;
    PO_GUARDED_BY(mu) int std_B = 0;
    PO_GUARDED_BY(mu) long std_flag_at = -1, std_left2_at = -1;  // (std_left2_at: where the second list of parked paths starts, sliced solves; -1: there is one list)
    PO_GUARDED_BY(mu) int dp_waves_used = 0;     // waves per instance of the last DP lattice search: 8 or 1 (0: none yet; po_debug_get "dp_waves_used")
    PO_GUARDED_BY(mu) int smooth_variant_used = 0;  // instantiation of the last smoothing launch: 100 * kind + 10 * waves per QP + WPE, e.g. 143 = <TENSION, 4, 3> (0: none yet; po_debug_get "smooth_variant_used")
    PO_GUARDED_BY(mu) int nw_slice = 8;  // steps of the first of the two Newton launches (po_debug_set "newton_slice"; 0: one launch).  Scheduling only.
    PO_GUARDED_BY(mu) HostBuf fb_host; // ... and the pinned word its count is read back into (refine_chain = 2)
    // developer switches (po_debug_set; the library reads no environment variable): identity_order (block i solves path i), debug_cycles (per-phase shader
    // clocks of path 0 on stderr; synchronises), smoothing / DP-search A/B switches
    PO_GUARDED_BY(mu) bool env_identity = false, env_cycles = false, env_smooth_seq = false, env_smooth_nopad = false, env_smooth_debug = false, env_dp_one_wave = false;
    PO_GUARDED_BY(mu) int env_smooth_waves = 0;
    // the staging blocks of the host-pointer entries, the arena of po_plan_batch*; edt_io: staging of the occupancy, obstacle-list and scene entries
    PO_GUARDED_BY(call_mu) DevBuf in_buf, out_buf, asm_buf, post_buf, bnd_buf, smooth_io, plan_io, plan_arena, plan_host, edt_io;
    // scratch of the device-pointer entries; edt_buf: occupancy -> distance transform, the 16-bit intermediate (2 bytes per cell)
    PO_GUARDED_BY(mu) DevBuf scale_buf, dbg_buf, map_buf, coef_buf, smooth_buf, edt_buf;
    PO_GUARDED_BY(mu) DevBuf raster_buf;  // obstacle lists -> map stack: the M occupancy images between the rasteriser and the transform (1 byte per cell)
    // The map stack: M layers in map_buf, their centres in map_pos_buf when they differ, the instance -> layer table in map_assign_buf.
    // maps is the view the kernels get; maps.d == nullptr until a map is set (maps.M survives a failed re-install: "same M keeps the assignment" is judged against it).
    PO_GUARDED_BY(mu) DevBuf map_pos_buf, map_assign_buf;
    PO_GUARDED_BY(mu) po::DevMaps maps{};
    // The world grid: one static occupancy image of the site in world_buf; world.cells == nullptr until one is set.  The scene entries read it.
    PO_GUARDED_BY(mu) DevBuf world_buf;
    PO_GUARDED_BY(mu) po_occupancy world{};
    PO_GUARDED_BY(mu) int world_outside = 0;
    PO_GUARDED_BY(mu) DevBuf select_buf;  // score and select: the clamped group table [G + 1] and, when the caller wants no cost array, cost [B]
};

// A grow-only block that launches already enqueued on the handle's stream may still read: they are finished before the old block is released.
inline int grow_after_sync(po_handle h, DevBuf &buf, size_t bytes) PO_REQUIRES(h->mu) {
    if (bytes <= buf.cap) return PO_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return buf.ensure(bytes);
}

// A batch of B instances on the handle's map stack: with an assignment installed, every instance needs an entry of the table.
inline bool assignment_covers(const po_handle_s *h, int B) PO_REQUIRES(h->mu) { return !h->maps.layer_of || B <= h->maps.n_assign; }

// ---- Stage: the format of one staging block of a host-pointer entry.  The entry DECLARES its arrays, in any order, and gets a slot for each; reserve() sizes the
// block from those declarations and grows the DevBuf it lives in, copy_in() enqueues one H2D copy per declared input, copy_out() one D2H copy per wanted output and
// synchronises.  A slot converts to its device pointer once the block is reserved, so no entry computes an offset.  Every slot is aligned to 16 bytes.
//   in(host, n)      n elements copied from host; host == nullptr: the array is absent, takes no room, and the slot is a null pointer
//   out(host, n)     n elements the kernel writes, copied to host by copy_out(); host == nullptr: the device array exists all the same, only the copy is skipped
//   out_opt(host, n) an optional output: host == nullptr: the caller does not want it, it is not declared, and the slot is a null pointer that the kernel skips
//   inout(host, n)   an output the kernel writes only in part: copied from host and back, so what is not written keeps the caller's bytes; host == nullptr: as out_opt
//   scratch(n)       n elements that travel in neither direction
// Copies go from / to the caller's own memory on the handle's stream, under mu; the block itself is under the lock its member names.
class Stage;
template <typename T> struct Slot {
    const Stage *stage = nullptr;
    size_t item = 0;
    T *ptr() const;
    operator T *() const { return ptr(); }
};
class Stage : NoCopy {
    struct Item { size_t off, bytes; const void *src; void *dst; };
    std::vector<Item> items_;
    size_t bytes_ = 0;
    char *base_ = nullptr;
    template <typename T> friend struct Slot;
    template <typename T> Slot<T> add(size_t n, const void *src, void *dst) {
        bytes_ = (bytes_ + 15) & ~(size_t)15;
        items_.push_back({bytes_, sizeof(T) * n, src, dst});
        bytes_ += sizeof(T) * n;
        return {this, items_.size() - 1};
    }

public:
    template <typename T> Slot<T> in(const T *host, size_t n) { return host ? add<T>(n, host, nullptr) : Slot<T>{}; }
    template <typename T> Slot<T> out(T *host, size_t n) { return add<T>(n, nullptr, host); }
    template <typename T> Slot<T> out_opt(T *host, size_t n) { return host ? out(host, n) : Slot<T>{}; }
    template <typename T> Slot<T> inout(T *host, size_t n) { return host ? add<T>(n, host, host) : Slot<T>{}; }
    template <typename T> Slot<T> scratch(size_t n) { return add<T>(n, nullptr, nullptr); }
    size_t bytes() const { return bytes_; }
    // f(offset, bytes, host source or nullptr, host destination or nullptr) for every declared array, in order: for an entry that moves the block itself and keeps a
    // mirror of it at the same offsets (po_solve_batch: its pinned blocks and pipelined copy)
    template <typename F> void each(F f) const {
        for (const Item &it : items_) f(it.off, it.bytes, it.src, it.dst);
    }
    int reserve(po_handle h, DevBuf &buf, bool after_sync = false) PO_REQUIRES(h->mu) {
        PO_TRY(after_sync ? grow_after_sync(h, buf, bytes_) : buf.ensure(bytes_));
        base_ = static_cast<char *>(buf.p);
        return PO_OK;
    }
    int copy_in(po_handle h) const PO_REQUIRES(h->mu) {
        for (const Item &it : items_)
            if (it.src) HIP_TRY(hipMemcpyAsync(base_ + it.off, it.src, it.bytes, hipMemcpyHostToDevice, h->stream));
        return PO_OK;
    }
    int upload(po_handle h, DevBuf &buf, bool after_sync = false) PO_REQUIRES(h->mu) {  // reserve + copy_in
        PO_TRY(reserve(h, buf, after_sync));
        return copy_in(h);
    }
    int copy_out(po_handle h) const PO_REQUIRES(h->mu) {
        for (const Item &it : items_)
            if (it.dst) HIP_TRY(hipMemcpyAsync(it.dst, base_ + it.off, it.bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return PO_OK;
    }
};
template <typename T> T *Slot<T>::ptr() const { return stage ? reinterpret_cast<T *>(stage->base_ + stage->items_[item].off) : nullptr; }

// ---- The staged call: what every host-pointer entry does once its arguments are checked and its arrays are declared on S.  The call lock makes staging, launch
// and read-back one atomic unit; mu is held while the handle's fields are read and the copies are enqueued, and released around the device twin, which takes it
// itself.  `block` names the staging block S lives in (a member pointer: the block is only touched here, under both locks).  `precheck` runs under mu before
// anything is staged, for an entry that must refuse on the handle's state with nothing touched.
struct NoPrecheck {
    int operator()(po_handle) const { return PO_OK; }
};
template <typename Twin, typename Precheck = NoPrecheck>
int staged_call(po_handle h, Stage &S, DevBuf po_handle_s::*block, bool after_sync, Twin twin, Precheck precheck = Precheck{}) {
    Lock call(h->call_mu);
    {
        Lock g(h->mu);
        PO_TRY(precheck(h));
        HIP_TRY(hipSetDevice(h->device));
        PO_TRY(S.upload(h, h->*block, after_sync));
    }
    PO_TRY(twin());
    Lock g(h->mu);
    return S.copy_out(h);
}

// ---- a batch of splines (po_spline_in): one argument check, one DevSpline.  `length` is what ReferencePath attaches to the spline; segmentRawReference and the
// post-smoothing projection do not read it (need_length = false).
inline bool spline_args_ok(const po_spline_in *in, bool need_length = true) {
    return in && in->B >= 0 && in->K >= 3 && (in->B == 0 || (in->knot_s && in->knot_x && in->knot_y && (in->length || !need_length)));
}
inline po::DevSpline make_dev_spline(const po_spline_in *in) {  // (coef = nullptr: the spline coefficients are fitted in LDS by each consumer kernel)
    return po::DevSpline{in->B, in->K, in->knot_s, in->knot_x, in->knot_y, in->n_knots, in->length, nullptr};
}

#pragma GCC visibility pop
