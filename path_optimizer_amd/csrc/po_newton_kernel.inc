// po_newton_kernel.inc — the text of the Newton launch's kernel.  po_fast.inc includes it once per kernel compiled from it, with PO_NW_KERNEL = the kernel's name and
// PO_NW_CK = whether the phase takes the standard row classes as compile-time constants (refine_phase_newton's CK): newton_kernel (false) and newton_kernel_std
// (true; fixed lengths only, DESIGN.md section 36).  Two kernels from ONE text, not a body function that both call: called from newton_kernel it changed the code the compiler emits for every
// Newton object (by reference and by value alike), and those objects keep their device code byte for byte (tools/device_text_diff.py).
template <int F, int SPL, int NT, int NWX = 1, int PH = 1, int NFIX = 0> __global__ PO_KERNEL_ATTR __launch_bounds__(NT) void PO_NW_KERNEL(DevBatch in, DevParams P) {
    constexpr bool CK = PO_NW_CK;  // (nothing else differs: the engine hands newton_kernel_std only paths whose classes are the standard ones)
    using FX = Fast<F, SPL, NT, true, NWX, NFIX>;
    extern __shared__ double smem[];
    // SLICED LAUNCHES (in.nw_phase; the engine's default on one-wave shapes, DESIGN.md section 11): phase 1 runs every path for at most P.ref_nw_slice Newton steps — every path takes
    // that many, so the launch has no tail — and parks what is not finished (state block of its own, a priority key); nw_sort_kernel orders the parked paths by expected
    // remaining work, longest first; phase 2 (workgroup i takes entry i of that list; workgroups start in index order) finishes them.  The tail of a single launch — a
    // 35-step path that happens to start last while the mean is 14 — was 30 % of it.  The same operations in the same order: statuses and certificates do not depend on the slicing, solutions agree to round-off (two separately compiled kernels).
    // PH = 1 with P.ref_nw_slice = 0 (no parking block: po_debug_set "newton_slice" 0) is the single launch.
#ifdef PO_NW_TRACE
    const long long tk0_ = __builtin_readcyclecounter();
#endif
    int b;
    if constexpr (PH == 2) {
        if ((int)blockIdx.x >= in.nw_list[0]) return;
        b = in.nw_list[1 + blockIdx.x];
    } else b = in.order ? in.order[blockIdx.x] : perm_index(blockIdx.x, in.perm_bits, in.B);
    if ((unsigned)b >= (unsigned)in.B) return;
    po_info *oi = in.out_info + b;
    const bool slicing = PH == 2 || P.ref_nw_slice > 0;
    if (oi->status != PO_STATUS_SOLVED) return;  // (non-finite inputs, out of iterations, infeasible: reported as the solve left them)
    FX fx(P, in, smem, b);
    typename FX::LS st;
    fx.load(st);
    // (the state block is read BEFORE the LDS set-up: behind its barriers the 70 loads would start a round trip of their own after those of load() and scale_to_lds())
    double *state = in.pol_state + (size_t)b * in.pol_stride;
    double *pstate = slicing ? in.nw_state + (size_t)b * in.nw_stride : nullptr, *pscal = slicing ? pstate + (size_t)FX::kParkDoubles * NT : nullptr;
    if constexpr (PH == 2) fx.template park_io<false>(st, pstate); else fx.template state_io<false>(st, state);
    for (int i = fx.tid; i < fx.L.total; i += NT) smem[i] = 0.0;
    __syncthreads();
    fx.scale_to_lds();
    // (wave-uniform and alive until the kernel's last lines: scalar registers — uni(), po_device.hpp)
    const int lo_it = uni(oi->iters), lo_nref = uni(oi->n_refactor);
    const double lo_rho = uni(oi->rho), rp0 = uni(oi->r_prim), rd0 = uni(oi->r_dual);
    const int rounds = P.ref_rounds > 1 ? P.ref_rounds : 1, rounds_total = rounds + P.ref_extra;
    const bool last = 1 >= rounds_total;
#ifdef PO_NW_TRACE
    const long long tk1_ = __builtin_readcyclecounter();
#endif
    const RefineOut ro = refine_phase_newton<F, SPL, NT, NWX, PH, NFIX, CK>(fx, st, P, lo_rho, rp0, rd0, slicing ? P.ref_nw_slice : 1 << 30, pscal, slicing ? in.nw_keys + b : nullptr);
    __syncthreads();
#ifdef PO_NW_TRACE
    const long long tk2_ = __builtin_readcyclecounter();
    if (fx.b == 0 && fx.tid == 0) printf("  dev kernel PH %d: entry %lld cycles (load, LDS set-up, state block), phase %lld (%d steps)\n", PH, tk1_ - tk0_, tk2_ - tk1_, ro.it);
#endif
    if constexpr (PH == 1) if (ro.parked) { fx.template park_io<true>(st, pstate); return; }  // (po_info and the state block of the solved point stay as the warm start left them)
    const bool hand_back = !ro.stop && !last;
    // the state block after this kernel is read by the fallback rounds (a path handed back) and by polish_kernel: a finished path's state is not stored otherwise
    // (147 MB of writes per BASELINE batch).  Attempt not taken: the solved point stays in the block, and comes back into st for the outputs below
    if (ro.take) { if (hand_back || P.polish) fx.template state_io<true>(st, state); }
    else if (!hand_back) fx.template state_io<false>(st, state);
    if (hand_back) {
        if (fx.tid == 0) {
            oi->status = kStatusDeferred - 1; oi->iters = lo_it + ro.it; oi->status_polish = lo_it; oi->n_refactor = lo_nref + ro.nfac;
            if (ro.take) { oi->r_prim = ro.R.rp; oi->r_dual = ro.R.rd; oi->obj = ro.R.obj; }
            oi->status_refine = -1;
            in.fb_list[1 + atomicAdd(in.fb_list, 1)] = b;  // newton_fallback_kernel takes it from here
        }
        return;
    }
    fx.output_pass(st);  // (the warm start left them to this kernel: DevBatch::nw_follows)
    if (fx.tid == 0) {
        oi->iters = lo_it + ro.it; oi->n_refactor = lo_nref + ro.nfac;
        if (ro.take) { oi->r_prim = ro.R.rp; oi->r_dual = ro.R.rd; oi->obj = ro.R.obj; }
        oi->status_refine = ro.stop ? 1 : -1;
    }
}
