// po_fast.inc — the fused, register-resident solve of one path per workgroup (included by po_solve_common.hpp inside namespace po).  This comment is the MAP of the
// file: its sections, each under a banner `==== [name] ====` (search for the bracketed name) that says what the section reads, writes and serves.
//
// One struct, Fast<F, SPL, NT, TWO, NWX, NFIX>, is the per-lane view of a path: every lane keeps the state of its own stages (x, the one-number-per-row v, bounds,
// transition coefficients, slack-elimination data: LaneState) in registers for the whole kernel — the inputs are read from HBM once, coalesced — and LDS (LayoutF) holds
// only what is indexed across lanes: the block-LDL' factor, the scan tables and small exchange buffers.  Every member is forced inline; the kernels are what the compiler sees.
//
//   F     formulation (F_KP, F_KPC, F_K: FormTraits, po_device.hpp)
//   SPL   stage slots per lane
//   NT    threads per workgroup (64: one wave; 128 / 256: several)
//   TWO   false: SINGLE-LEVEL mapping — the substitution is one sequential chain over all stages (any keep; the fall-back of the shapes below)
//         true:  TWO-LEVEL mapping — a lane's stages are a chunk, the chunks are solved in parallel and their boundaries by a scan over lanes
//   NWX   lane layout of the two-level mapping: 1 one lane per chunk; 2 role-split (a chunk on two lanes), 3 role-split of an odd keep; 4 / 5 multi-group (keep 1 / 2:
//         several control groups per lane).  The details are at the top of [fast_core]
//   NFIX  path length at compile time for the LDS layout and the global offsets (0: at run time); KP, NWX 1 only ([fast_core], DESIGN.md section 19)
//
// Kernels ([kernels]; instantiated by po_solve_form.hip from the table of po_solve_common.hpp, launched by po_kernels.hip):
//   solve_kernel_fast<F, SPL, NT, TWO, UNI, NWX, NFIX>   load, ADMM loop (UNI: the variant for wave-uniform row classes), output — also the warm start of the Newton launches
//   newton_kernel / newton_kernel_std<..., PH, NFIX>     the Newton refinement (po_params.refine = 2), single or sliced in two phases; _std: standard row classes as constants
//   newton_std_select_kernel                             which paths of a fixed-length batch have the standard classes
//   newton_fallback_kernel                               later rounds of the paths a Newton launch handed back
//   polish_kernel                                        OSQP's polish (po_params.polish)
//
// THE ORDER IS PART OF THE CODE.  The sections from [fast_core] to [output] are ONE struct body: a member function may be used before its definition, a nested type
// (Cert, Tr, ChunkEl, ChunkRun, FwdGroup, ...) may not, so a section that is ever cut out into a file of its own is cut where it stands and included there.  The
// shipped kernels are verified for the register allocation they have, so an edit that only moves or documents text is gated by the device code itself:
// tools/device_text_diff.py against a build of the parent must report 0 differ (DESIGN.md section 38).
//
//   before the struct   [layout]            dev macros; LaneState, LayoutF, lds_bytes_fast; bcast, path_n, path_c        (all the host dispatcher uses)
//                       [row_fns]           row functors of the polish and of the reclassification
//   the struct          [fast_core]         parameters, lane geometry, row-class and scale accessors, load(); then:
//                         [single_level]      !TWO: factor_blocks, factor_chain, rhs_pass, chain_solve, update_pass (Cert), residual_pass, rescale_pass
//                         [two_prims]         TWO:  chunk geometry, 9-records, factor accessors, DPP moves, xchg / wshfl, apply_E*, mul_G*
//                         [two_factor]              factor_blocks_two, transition (Tr)
//                         [two_pivot_scan]          the pivot chain as a scan over chunks: factor_pivots_scan (NW 1), factor_pivots_scan2 (NW 2)
//                         [two_factor_chain]        factor_chain_two: scan or sequential recursion, then the scan tables of the solve
//                         [two_sweeps]              chunk-local sweeps, the role-split hand-off, the one-wave boundary scans, solve_split (NW 2)
//                         [two_rhs]                 rhs_pass_two, classify
//                         [two_solve]               solve_two (NW 1)
//                         [two_update]              update_pass_two, nbr_x, residual_pass_two
//                         [newton_passes]           state_io / park_io, block reductions, reclass_pass, the Newton passes nw_*
//                         [polish_passes]           pol_init, pol_reset, pol_eval
//                         [output]                  output_pass
//   after the struct    [loops]             admm_loop, refine_phase_newton
//                       [kernels]           the kernels above (newton_kernel's text: po_newton_kernel.inc, included twice)

// ==================== [layout] ====================
// what exists before the struct Fast, and all of po_fast.inc that the host dispatcher (po_kernels.hip) uses: the dev macros, the per-lane state
// (LaneState), the map of the workgroup's dynamic LDS (LayoutF; lds_bytes_fast is its host-side size, used by lds_of) and three free helpers.  Live for every instantiation.
//
// LaneState is plain registers: nothing here is indexed at run time (every loop over it is unrolled), which is what lets the compiler split it.  Who writes what:
//   load()                          lb, ub, maxk, kin / dsin / kout / dsout, trin / trout, bin0, mkp, cls / clse / clsc (bound_classes); zeroes the rest
//   rhs passes                      bx, bxu (right-hand side), gs / gsu;   the solves: bx, bxu (solution), bnext, bprev
//   update passes                   x, u, su, vl, vd, vdo, vend, vc
//   factor_blocks / _two            hi, hv, hiu, hus (general variant; the UNI variant reads them from LDS, rrb)
//   reclass_pass                    cls / clse / clsc (refinement);   the polish and a parked Newton path: pc / pce / pcc
// LayoutF, in doubles from the LDS base S.  SINGLE-LEVEL (!two): bz, bu, tk (rhs / solution), fac, facu (factor); wt = bz (factor scratch, idle while factorising).
// TWO-LEVEL: fac, facu (factor, 9-records: idx9(), [two_prims]), phi (scan tables, one 9-record region per level), ex (multi-wave mailboxes and reduction scratch),
// rseg, mail (segmented scan, NT > 64 and one lane per chunk), hx0 / hx1 (role-split hand-off slots).  ALIASES THAT MATTER: wt = bz = phi — the (k, ds, trig) table of
// the sequential factorisation and the [N][2] + [N] scratch of output_pass lie on the scan tables, which are rebuilt by every factor_chain_two and dead once the last
// solve has run; role-split: ex = hx1 — a block reduction (block_any, block_sum2, the residual passes) overwrites hand-off slot 1, so it never runs inside solve_split.
// Both mappings: cst (LDS copy of the path's equilibration block, scale_to_lds) and rrb (per-factorisation uniform row steps and, UNI, slack-elimination data).
// Before the kernel zeroes its LDS, the first words at S also carry the block votes of inputs_have_nan() and classify().
//
// The dev macros are defined HERE, once, for every section: none relies on a macro that another happens to define (function-local helper macros are #undef'd where they end).
#ifndef PO_KERNEL_ATTR  // dev: an occupancy attribute on every solve kernel of a build (e.g. -DPO_KERNEL_ATTR='__attribute__((amdgpu_waves_per_eu(2,2)))')
#define PO_KERNEL_ATTR
#endif
// the lane id through an empty asm: what derives from it is recomputed after this point, not hoisted (admm_loop, [loops])
#define PO_FRESH_LANE_ID(fx) asm volatile("" : "+v"((fx).tid))
#ifdef PO_MARKS  // dev: phase markers in the assembly listing (hipcc -S -DPO_MARKS)
#define PO_MARK(name) asm volatile("; PO_MARK " name)
#else
#define PO_MARK(name)
#endif
#ifdef PO_NW_TRACE  // dev: cycles of the parts of a factorisation into Fast::dbgc (factor_chain_two, which declares tf_; printed by refine_phase_newton)
#define PO_FC_TICK(i) { const long long n_ = __builtin_readcyclecounter(); dbgc[i] += n_ - tf_; tf_ = n_; }
#else
#define PO_FC_TICK(i)
#endif

// G: control groups per lane (1, or — multi-group mapping of keep 1 / 2, KP only — SPL / keep)
template <int F, int SPL, int G = 1> struct LaneState {
    using T = FormTraits<F>;
    static_assert(G == 1 || (T::HAS_U && !T::HAS_SU && T::NCTL == 1), "several controls per lane: KP");
    double x[SPL][3 + T::NS];
    double vl[SPL][T::NLOC];
    double vd[SPL][T::NDYN];     // v of the rows INTO stage q (transition j-1 -> j, or the initial-state rows)
    double vdo[T::NDYN];         // copy of the next thread's vd[0] (transition out of this thread's last stage)
    double vend[2];
    double lb[SPL][4], ub[SPL][4], maxk[SPL];
    double kin[SPL], dsin[SPL];  // reference curvature / arc-length step of the incoming transition (j-1)
    double kout, dsout;          // ... of the transition out of the last owned stage
    double trin[F == F_K ? SPL : 1][2], trout[2];  // K: cached trigonometric coefficients of those transitions
    double hi[SPL][T::NS], hv[SPL][T::NS][3], gs[SPL][T::NS];
    double bin0[3];              // initial-state bounds (thread 0 only)
    unsigned cls[SPL], clse, clsc;  // packed row classes (2 bits/row): stage-local rows, end rows, control rows
    unsigned pc[SPL], pce, pcc;     // polish only: active-set codes (2 bits/row: 0 inactive, 1 active at l, 2 active at u), same packing
    double bx[SPL][3], bxu[G];   // two-level solve: rhs in, solution out (own stages / own controls)
    double bnext[3], bprev[4];   // neighbour chunks' boundary values (next first stage; previous last stage + control)
    // the lane's controls (group g of the lane: control clane * G + g)
    double u[G], su, vc[G][3], hiu, hus, gsu, mkp;
};

template <int F> struct LayoutF {
    using T = FormTraits<F>;
    int bz, bu, tk, fac, facu, wt, cst, rrb, total;
    // two-level mode
    int TP, nlev, phi, beta, ybd, bfirst, xlast, ex, rseg, mail, nsm;  // nsm: segment slots (threads / 8)
    int hx0, hx1;  // role-split mapping (nw == 2): the two hand-off slots [4][TP] between the two lanes of a chunk
    bool seg;
    // spl = stages per LANE; nw = lanes ("roles") a chunk is split over: 1, or 2 — the role-split mapping of keep 6 .. 8: chunk = control group = 2 spl stages (2 spl - 1 when
    // `keep` is odd: role B's last slot is empty), role A = chunk stages 0 .. spl-1 on lane t, role B = the rest + (normally) the control on lane t + nt / 2
    __host__ __device__ LayoutF(int N, int C, int spl, bool two, int nt, int nw = 1, int ch = 0, int g = 1) {
        hx0 = hx1 = 0;
        if (nw == 2) { spl = ch > 0 ? ch : 2 * spl; nt = 64; }  // chunk-level tables exactly as in the one-wave mapping (ch = stages per chunk)
        int o = 0;
        if (!two) {
            bz = o; o += 3 * N + 3;       // rhs/solution [N][3] (+pad: prefetch reads one past the end)
            bu = o; o += C + 1;
            tk = o; o += N + 1;           // per-transition contribution to the control rhs
            fac = o; o += 18 * N + 18;
            facu = o; o += 4 * C + 4;
            wt = bz;                      // factor scratch wtgt_j (step A -> step B) aliases bz (idle during factorisation)
            TP = nlev = phi = beta = ybd = bfirst = xlast = ex = rseg = mail = nsm = 0; seg = false;
        } else {
            TP = (N + spl - 1) / spl;     // chunks (threads that own at least one stage)
            nlev = 0;
            while ((1 << nlev) < TP) ++nlev;  // Kogge-Stone levels over the chunk boundaries
            TP += TP & 1;                 // even: every 9-record region stays 16-byte aligned
            fac = o; o += 9 * spl * TP;   // per own stage q one 9-record region (Ginv 0..5 | w 6..8), see idx9()
            facu = o; o += 4 * TP * g;    // SoA [g][4][TP]: pu_inv, lx[3] of group g of every lane
            phi = o;                      // prefix products P^(l)_t, one 9-record region per level
            // multi-wave blocks use the segmented scan (8-lane segments): tables Q^(0..2), Q^incl, Q^suf instead of nlev levels
            seg = nt > 64;
            // one wave: row-segmented tables for the DPP scans (rows of 16 lanes): in-row Kogge-Stone levels 0..3, Q^incl (4), Q^suf (5)
            { const int need = 9 * TP * (seg ? 5 : 6), scratch = 4 * N + 4; o += (need > scratch ? need : scratch) + ((need > scratch ? need : scratch) & 1); }
            ex = o; if (nt > 64) o += 64;          // multi-wave blocks: wave-boundary mailboxes of the neighbour exchange [2][4][waves] and the
                                                   // cross-wave reduction scratch (13 per wave); everything inside a wave moves on DPP
            nsm = (TP + 7) >> 3;                   // segments of 8 chunks
            rseg = o; if (seg) o += 5 * nsm * 9;   // segment-level prefix products R^(l)_g, [5][nsm][9]
            mail = o; if (seg) o += 2 * nsm * 3;   // segment totals, forward / backward scan
            if (nw == 2) {  // hand-off slots [4][TP]; the cross-wave reduction scratch (ex) aliases slot 1
                hx0 = o; o += 4 * TP; hx1 = o; o += 4 * TP;
                ex = hx1;
            }
            wt = phi; bz = phi;           // scratch aliases: factor-time (k, ds, trig) table [N][4] / output pass [N][2]
            beta = ybd = bfirst = xlast = bu = tk = 0;
        }
        if (!two) { rseg = mail = nsm = 0; seg = false; }
        cst = o; o += kScStride;          // LDS copy of the per-path equilibration block (uniform reads: broadcast)
        rrb = o; o += 32;                 // per-factorisation uniform values: rho~ of local rows [0..8], control rows [9..11], dynamics rows [12..14];
                                          // uniform row classes only: slack elimination data hi[s] at [16 + s], hv[s][0..2] at [18 + 3 s]
        total = o;
    }
};
// nwx: 1 one lane per chunk, 2 role-split (chunk = 2 spl stages), 3 role-split of an odd keep (chunk = 2 spl - 1 stages), 4 / 5 multi-group (spl / 1, spl / 2 groups per lane)
template <int F> size_t lds_bytes_fast(int N, int C, int spl, bool two, int nt, int nwx = 1) { return sizeof(double) * (size_t)LayoutF<F>(N, C, spl, two, nt, (nwx == 2 || nwx == 3) ? 2 : 1, (nwx == 2 || nwx == 3) ? 2 * spl - (nwx == 3 ? 1 : 0) : 0, nwx == 4 ? spl : (nwx == 5 ? spl / 2 : 1)).total; }

__device__ __forceinline__ double bcast(double v, int k) {  // value of lane k (k uniform) to every lane
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, k);
    hi = __builtin_amdgcn_readlane(hi, k);
    return __hiloint2double(hi, lo);
}

// ragged batches: every path may have its own number of points (arrays keep the stride in.N)
__device__ __forceinline__ int path_n(const DevBatch &in, int b) {
    if (!in.n_points) return in.N;
    const int n = in.n_points[b];
    return n < 2 ? 2 : (n > in.N ? in.N : n);
}
template <int F> __device__ __forceinline__ int path_c(const DevBatch &in, int b) {
    if (F == F_K) return 0;
    if (!in.n_points) return in.C;
    return (path_n(in, b) + in.keep - 2) / in.keep;
}

// ==================== [row_fns] ====================
// the row functors that belong to Fast's later phases (the ones of the ADMM iteration itself are in po_device.hpp): handed to local_rows / end_rows /
// ctl_rows, which call row<MASK>(r, coefficients, l, u) once per constraint row of a stage or control.  They touch no LDS: they read and write the lane-state words they
// are pointed at (st.vl / vend / vc, the packed codes st.pc*) and their own accumulators.  TWO only (the phases that use them exist on the two-level mapping only).
//   PolWrap, PolInitFn, PolResetFn, PolEvalFn, PolRes    the polish: [polish_passes], and PolWrap around the inner functors of the <POL> passes
//                                                        (factor_blocks_two, rhs_pass_two, update_pass_two); polish_kernel
//   ReclassFn                                            reclass_pass ([newton_passes]): refine_phase_newton, at every step (mode 3) and on leaving the phase (mode 2)
// ---- polish (OSQP polish.c, po_params.polish) ----------------------------------------------------------------------------------
// The reduced KKT system of the polish, [[P + dI, Aa'], [Aa, -dI]] on the rows Aa of the active set, is in condensed form
// (P + dI + Aa' Aa / d) x = -q + Aa' b / d: the SAME block-tridiagonal matrix the ADMM iteration factorises, with sigma -> delta, the row step of an
// active row -> 1 / delta (on the scaled problem, like OSQP: W_r / delta), an inactive row dropped, and every active row an equality at the
// bound it is active at.  One step of OSQP's iterative refinement on the regularised system is exactly one more iteration of the same recursion
// with alpha = 1 (proximal method of multipliers), so the polish runs the general (non-uniform) passes through this wrapper: it hands the
// inner functor b = l or u twice for an active row and skips an inactive one.
template <class Inner> struct PolWrap {
    Inner &in;
    unsigned pc;
    template <int MASK, class TL, class TU> __device__ __forceinline__ void row(int r, double c0, double c1, double c2, double c3, double c4, TL l, TU u) {
        const unsigned code = (pc >> (2 * r)) & 3u;
        if (code == 0u) return;
        const double b = code == 1u ? (double)l : (double)u;
        in.template row<MASK>(r, c0, c1, c2, c3, c4, b, b);
    }
};
constexpr unsigned kPolAllEq = 0x55555555u;  // row class "equality" for every row (what the inner functors see during the polish)
// initial active set from the ADMM state (form_Ared: z - l < -y / u - z < y; in the one-number-per-row form z = clip(v), y = rho (v - z),
// that is v < l / v > u); equality rows always active, free rows never
struct PolInitFn {
    const double *v;
    unsigned cls, pc;
    template <int MASK, class TL, class TU> __device__ __forceinline__ void row(int r, double, double, double, double, double, TL l, TU u) {
        const unsigned c = (cls >> (2 * r)) & 3u;
        const double vv = v[r];
        const unsigned code = c == 1u ? 1u : (c == 2u ? 0u : (vv < (double)l ? 1u : (vv > (double)u ? 2u : 0u)));
        pc |= code << (2 * r);
    }
};
// restart of a polish pass: y = 0, i.e. v = b on the active rows
struct PolResetFn {
    double *v;
    unsigned pc;
    template <int MASK, class TL, class TU> __device__ __forceinline__ void row(int r, double, double, double, double, double, TL l, TU u) {
        const unsigned code = (pc >> (2 * r)) & 3u;
        if (code) v[r] = code == 1u ? (double)l : (double)u;
    }
};
// the polished point: the active set it implies (form_Ared's test on z = Ax and the polished duals), project_normalcone, residuals
struct PolEvalFn {
    double x[5], aty[5];
    const double *v, *W;
    unsigned cls, pc_old, pc_new;
    double idelta, rp, nAx, nz;
    int changes;
    template <int MASK, class TL, class TU> __device__ __forceinline__ void row(int r, double c0, double c1, double c2, double c3, double c4, TL l, TU u) {
        const double c[5] = {c0, c1, c2, c3, c4};
        double ax = 0;
#pragma unroll
        for (int a = 0; a < 5; ++a)
            if (MASK >> a & 1) ax += c[a] * x[a];
        const unsigned code = (pc_old >> (2 * r)) & 3u, k = (cls >> (2 * r)) & 3u;
        const double b = code == 1u ? (double)l : (double)u;
        const double yw = code ? (v[r] - b) * idelta : 0.0;  // y_r / W_r (scaled dual over the scaled row norm: what OSQP compares)
        const unsigned ncode = k == 1u ? 1u : (k == 2u ? 0u : ((ax - (double)l < -yw) ? 1u : (((double)u - ax < yw) ? 2u : 0u)));
        changes += ncode != code;
        pc_new |= ncode << (2 * r);
        const double t = ax + yw, z = clipd(t, l, u), yn = W[r] * (t - z);
        rp = fmax(rp, fabs(ax - z)); nAx = fmax(nAx, fabs(ax)); nz = fmax(nz, fabs(z));
#pragma unroll
        for (int a = 0; a < 5; ++a)
            if (MASK >> a & 1) aty[a] += yn * c[a];
    }
};
struct PolRes { double rp, rd, obj; int changes, bad; };
// Refinement (po_params.refine): new step class of every row from its ACTIVITY — equality rows stay 1, free rows 2, an inequality row is 0 (step rho) while
// it is active (v outside [l, u]: z at the bound, y of the matching sign) and 2 (step rho_min) while it is not — and v re-expressed for the new step
// (z and y kept: v = z + (step_old / step_new)(v - z)).  mode 1: rows that hold class 0 keep it (the set only grows); mode 2: back to the bound types.
struct ReclassFn {
    // v: a COPY of the row group's step-scaled duals (copied in and out by reclass_pass), not a pointer into the lane state: a functor that is re-pointed
    // from group to group carries a phi of addresses into the LaneState, and a lane state whose address is merged like that is not split into registers
    // (measured on the two-wave refinement builds: the whole second LaneState stayed in scratch, 1.26 KB per lane; a refinement iteration cost three plain ones)
    double v[9];
    unsigned cls_type, cls_old, cls_new;
    double req_o, req_n;  // step of an equality row before / after (1e3 rho; the Newton refinement has its own)
    double rho_o, rho_n;  // rho before / after: a row's step is rho, rho_eq = 1e3 rho or rho_min by class (the row's own W cancels in the ratio).  No
                          // {rho, rho_eq, rho_min} tables: the optimiser turns a three-way select over an array into a computed index, which pins the
                          // whole functor (and the rows it carries) in scratch
    int mode, changes;
    template <int MASK, class TL, class TU> __device__ __forceinline__ void row(int r, double, double, double, double, double, TL l, TU u) {
        const unsigned k = (cls_type >> (2 * r)) & 3u, co = (cls_old >> (2 * r)) & 3u;
        const double vv = v[r], z = clipd(vv, l, u);
        // active: v outside [l, u] by more than rounding noise (a row that sits on its bound with a numerically zero multiplier has v - z ~ 1e-19 of either
        // sign: counting that as a multiplier costs a refactorisation for nothing)
        // mode 3 (Newton refinement, refine = 2): v IS w = a.x + y / rho — active means outside the bounds by more than rounding noise (a slack that sits
        // on its bound comes out as +-1e-19; whether such a row is in the Newton matrix must not hang on that sign), and v is not re-expressed
        const bool act = fabs(vv - z) > (mode == 3 ? 1e-15 : 1e-9) * (1.0 + fabs(z));
        const unsigned cn = k ? k : ((mode == 2 || act || (mode == 1 && co == 0u)) ? 0u : 2u);
        const double s_old = co == 2u ? kRhoMin : (co == 1u ? req_o : rho_o), s_new = cn == 2u ? kRhoMin : (cn == 1u ? req_n : rho_n);
        if (mode != 3 && s_old != s_new) v[r] = z + (s_old / s_new) * (vv - z);
        changes += cn != co;
        cls_new |= cn << (2 * r);
    }
};

// ==================== [fast_core] ====================
// the struct Fast opens here, with what every mapping and phase uses; the sections up to [output] are the rest of its body, and the struct closes after [output].
// Live for every instantiation.  Here: the template parameters and what derives from them (NW, ODD, CH, HW, GK, NG, kFixC), the lane geometry (clane, wrole, stage, cs,
// cidx, has_ctl, the group predicates, psel), the accessors of the uniform row data (rrb: uhi, uhv, uhi_at, k_rr*; cls_of, kpc_c3) and of the equilibration block
// (sc -> global, then LDS cst after scale_to_lds: Wloc .. cD, eq_row_step / eq_row_scale), stage_in / dyn_in / dyn_out, and the one-time load().
//   LDS     scale_to_lds writes cst; inputs_have_nan votes through the first words at S (NT > 64; before the kernel zeroes its LDS); the rrb accessors only read
//   lanes   load() fills the inputs' part of LaneState from HBM, zeroes the iterate and sets cls / clse / clsc (bound_classes) and nan_in
//   called  by every kernel of [kernels] right after constructing the object: load(), [inputs_have_nan()], scale_to_lds(); the accessors by every pass
// NW = 1: lane t owns the whole chunk t (SPL stages = one control group, or K's SPL nodes).
// NW = 2: ROLE-SPLIT mapping (round 5; keep_control_steps_ 5 .. 8, where one lane per group spills hundreds of registers): chunk t = control group t = CH = 2 SPL - ODD stages
//         lives on TWO lanes — role A (lane t of the first half of the block) owns chunk stages 0 .. SPL-1, role B (lane t of the second half) owns chunk stages SPL .. CH-1 in
//         its slots ODD .. SPL-1 (odd keep: slot 0 of role B is empty) and, for every chunk with at least SPL transitions, the control (own_role()).  Chunk-level data (factor,
//         scan tables, boundary scans) are exactly those of the one-lane mapping with CH stages per chunk; per-lane state is that of SPL stages, so keep 8 runs in the registers
//         of the keep-4 kernel.  NT = 64: both roles share ONE wave (lanes 0..31 / 32..63, <= 32 chunks); NT = 128: one wave per role (<= 64 chunks).  What crosses the role
//         boundary inside a sweep is a 3-vector (+ the running control accumulator) through an LDS slot.  See solve_split().
// NWX (what the kernels are instantiated with): 1 = one lane per chunk, 2 = role-split, 3 = role-split of an odd keep.
// NFIX: the path length at COMPILE time (0: at run time), for the LDS LAYOUT and the global offsets: LayoutF — TP, every table offset, the row counts of the scans — is then a
// constant of the instantiation and the LDS addresses are immediates; the same LayoutF / state block / parking block as at run time, so a path may cross between a fixed and a
// generic kernel (fall-back rounds, polish, a resumed path).  C, the number of controls, is the constant kFixC as well: it only decides which lanes own a control
// (`cidx(g) < C`), no floating-point block hangs on it.  N ITSELF stays a run-time value on purpose: with N a constant the compiler merges the per-stage
// `stage(q) < N` regions and drops the copies of the final-stage rows that cannot occur, which changes where multiply-adds are contracted — 10 % fewer instructions still, but the
// results then differ from the generic kernels' in the last bits and a path in 4 096 takes one Newton step more (DESIGN.md section 19).  The fixed instantiations also keep the
// wave-uniform row steps of a pass in scalar registers (eq_row_step() / eq_row_scale()).  Layout, C and where uniform values live: bit for bit the generic kernels' results.
// The launchers take such an instantiation only for a non-ragged batch of exactly that length.
template <int F, int SPL, int NT, bool TWO, int NWX = 1, int NFIX = 0> struct Fast {
    static_assert(NFIX == 0 || (F == F_KP && TWO && NWX == 1 && NFIX >= 2 && NFIX <= NT * SPL), "fixed length: KP, one lane per chunk, a length the shape covers");
    static constexpr int kFixC = NFIX > 0 ? (NFIX + SPL - 2) / SPL : 0;  // controls of a path of NFIX points (keep == SPL on this shape: path_c())
    static constexpr int NW = (NWX == 2 || NWX == 3) ? 2 : 1, ODD = NWX == 3 ? 1 : 0;
    static_assert(NWX >= 1 && NWX <= 5, "NWX");
    static_assert(NW == 1 || (NW == 2 && TWO && (NT == 64 || NT == 128) && SPL >= 2 && FormTraits<F>::HAS_U), "role-split mapping: KP / KPC, two-level");
    static constexpr int CH = SPL * NW - ODD;  // stages per chunk
    static constexpr int HW = NT / NW;         // lanes per role
    // NWX 4 / 5: MULTI-GROUP mapping (round 5; keep_control_steps_ 1 / 2, KP): one lane per chunk of SPL stages that holds SPL / GK whole control groups of GK stages —
    // keep 1 at N = 200 then needs 50 lanes instead of 200 (one wave, 38 KB of LDS, four paths per CU instead of one).  Every other mapping: one group per chunk.
    static constexpr int GK = NWX == 4 ? 1 : (NWX == 5 ? 2 : CH);           // stages per control group (multi-group mapping: 1 / 2; else the chunk)
    static constexpr int NG = (NWX == 4 || NWX == 5) ? SPL / GK : 1;         // control groups per lane
    static_assert(NG * GK == SPL || NG == 1, "multi-group mapping: the chunk holds whole groups");
    using T = FormTraits<F>;
    using LS = LaneState<F, SPL, NG>;
    const DevParams &P;
    const DevBatch &in;
    LayoutF<F> L;
    double *S;
    int N, C, keep, tid, b;
    // chunk lane and wave role, derived from tid on every use (NOT stored: what derives from the lane id must stay re-computable per pass, see PO_FRESH_LANE_ID)
    __device__ __forceinline__ int clane() const { return NW == 1 ? tid : (tid & (HW - 1)); }
    __device__ __forceinline__ int wrole() const { return NW == 1 ? 0 : (tid >= HW ? 1 : 0); }
    // role-split mapping: first slot of this lane that holds a stage (1 for role B of an odd keep), and which role holds the chunk's control: the one in which its elimination falls —
    // after the group's last transition, i.e. role B whenever the chunk has >= SPL transitions (every full chunk), role A for a final chunk with fewer
    __device__ __forceinline__ int qoff() const { return (NW == 2 && ODD) ? wrole() : 0; }
    __device__ __forceinline__ int own_role() const { return NW == 1 ? 0 : (nq_chunk() >= SPL ? 1 : 0); }
    size_t po;
    double elo, ehi;
    const double *sc;  // per-path equilibration block
    unsigned pat_loc = 0, pat_ctl = 0;  // wave-uniform row-class patterns (valid when classify() returned true)
    unsigned pat_last = 0;              // K: pattern of the final stage (its e_phi row carries the end-heading window, its steering row is absent)
    mutable int nan_in = 0;             // set by load(): a NaN among this lane's inputs (read once, right after load(); see inputs_have_nan())
    // step of an equality row: OSQP's 1e3 x rho — except inside the Newton refinement (refine = 2), which sets its own fixed penalty (po_params.refine_newton_rho_eq) here for
    // the duration of the phase.  The object is fully inlined, so everywhere before the phase this is the constant 0 and folds away.
    mutable double nw_req = 0.0;
#ifdef PO_NW_TRACE
    mutable long long dbgc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // dev: cycles of the parts of a factorisation
#endif
    __device__ __forceinline__ double eq_step(double rho) const { return nw_req > 0.0 ? nw_req : kRhoEqOverIneq * rho; }

    // (forced inline: outlined — which the inliner does once the kernel is large enough — `this` escapes, the object lives in scratch, and every LDS access
    // through S degrades to a flat load: 17.5 -> 41.7 ms per BASELINE batch)
    __device__ __forceinline__ Fast(const DevParams &P_, const DevBatch &in_, double *S_, int b_)
        : P(P_), in(in_), L(NFIX > 0 ? NFIX : path_n(in_, b_), NFIX > 0 ? kFixC : path_c<F>(in_, b_), SPL, TWO, NT, NW, CH, NG), S(S_), N(path_n(in_, b_)),
          C(NFIX > 0 ? kFixC : path_c<F>(in_, b_)), keep(in_.keep), tid(threadIdx.x), b(b_), po((size_t)b_ * (NFIX > 0 ? NFIX : in_.N)) {
        sc = in_.scale + (size_t)b_ * kScStride;
        elo = -kInf; ehi = kInf;
        if (P.end_heading) {  // solver_kp_as_input.cpp:193-202
            const double psi = wrap_angle(in.goal_z[b] - in.ref_z[po + N - 1]);
            if (psi < 70 * kPi / 180) { elo = uni(psi - 5 * kPi / 180); ehi = uni(psi + 5 * kPi / 180); }  // (uniform, used by the path's LAST lane only, alive for the whole kernel: uni(), po_device.hpp)
        }
    }
    // From here on the equilibration block is read from LDS: a ds_read broadcast (~64 cycles) instead of a global load
    // (the compiler cannot prove the global block read-only, so it re-fetches it with VMEM loads in every pass).
    __device__ __forceinline__ void scale_to_lds() {
        for (int i = tid; i < kScStride; i += NT) S[L.cst + i] = sc[i];
        __syncthreads();
        sc = S + L.cst;
    }
    static constexpr int kNoStage = 0x3fffffff;  // slot without a stage (role B, slot 0, odd keep): every pass skips j >= N
    __device__ __forceinline__ int stage(int q) const {
        if constexpr (NW == 2 && ODD) { if (wrole() == 1 && q == 0) return kNoStage; }
        return clane() * CH + wrole() * SPL + q - qoff();
    }
    __device__ __forceinline__ int cs(int q) const { return wrole() * SPL + q - qoff(); }                // index of own stage q inside its chunk
    __device__ __forceinline__ int cidx(int g) const { return clane() * NG + g; }                          // control of the lane's group g
    __device__ __forceinline__ bool has_ctl(int g = 0) const { return wrole() == own_role() && cidx(g) < C; }    // this lane owns that control
    // group (of the lane) that the transition INTO / OUT OF own stage q belongs to (compile-time after unrolling; one group per lane: 0)
    static __device__ __forceinline__ constexpr int gIn(int q) { return NG == 1 ? 0 : (q > 0 ? (q - 1) / GK : 0); }
    static __device__ __forceinline__ constexpr int gOut(int q) { return NG == 1 ? 0 : q / GK; }
    // is the transition out of own stage q the last of its group?  (nq: own transitions that exist)
    __device__ __forceinline__ bool grp_end(int q, int nq) const { return NG == 1 ? q + 1 == nq : ((q + 1) % GK == 0 || q + 1 == nq); }
    // does the transition INTO / OUT OF own stage q belong to the own chunk's control group?  (the transition into chunk stage 0 is the previous group's)
    __device__ __forceinline__ bool in_own_group(int q) const { return cs(q) > 0; }
    __device__ __forceinline__ bool out_own_group(int q) const { return cs(q) == CH - 1; }
    // own (the value at slot q - 1) or nbr (the neighbouring lane's): a compile-time choice except for slot 1 of the role-split mapping of an odd keep
    __device__ __forceinline__ double psel(int q, double own, double nbr) const {
        if constexpr (NW == 2 && ODD) return q == 0 ? nbr : (q == 1 ? (wrole() == 1 ? nbr : own) : own);
        else return q > 0 ? own : nbr;
    }
    // Uniform row classes (classify()): the slack-elimination data of a stage depend on the row steps and on constants only, i.e. they
    // are the same number for every stage of every lane.  The UNI variants of the passes read them from LDS (written once per
    // factorisation) instead of keeping SPL * NS * 4 doubles per lane in registers — the kernel sits at the 512-register limit.
    __device__ __forceinline__ double uhi(int s_) const { return S[L.rrb + 16 + s_]; }
    __device__ __forceinline__ double uhv(int s_, int a) const { return S[L.rrb + 18 + 3 * s_ + a]; }
    // KPC: the only row whose class depends on the stage is the box of the curvature slack, 0 <= Sk <= max(kappa_max - max_k_i, 0): an equality where
    // the speed-dependent limit max_k_i reaches kappa_max (solver_kp_as_input_constrained.cpp:174-176).  The uniform variant keeps that one class per
    // stage — recomputed from max_k_i, which is in registers anyway — and everything that depends on it in two copies (row step, 1 / H_ss of that slack).
    static constexpr unsigned kKpcRow3 = 3u << 6;
    __device__ __forceinline__ unsigned kpc_c3(const LS &st, int q) const { return row_class(0.0, fmax(P.kmax - st.maxk[q], 0.0), Eloc()[3]); }
    template <bool UNI> __device__ __forceinline__ unsigned cls_of(const LS &st, int q) const {
        if constexpr (UNI && F == F_K) return stage(q) == N - 1 ? pat_last : pat_loc;
        if constexpr (UNI && F == F_KPC) return pat_loc | (kpc_c3(st, q) << 6);
        return UNI ? pat_loc : st.cls[q];
    }
    // 1 / H_ss of slack s_ at own stage q (uniform variant)
    __device__ __forceinline__ double uhi_at(int s_, const LS &st, int q) const {
        if constexpr (F == F_KPC) { if (s_ == 1) return kpc_c3(st, q) ? S[L.rrb + 25] : S[L.rrb + 17]; }
        return uhi(s_);
    }
    // K, uniform variant: the two row steps that are not the same on every stage (written per factorisation next to the uniform ones)
    __device__ __forceinline__ double k_rr2_end() const { return S[L.rrb + 15]; }
    __device__ __forceinline__ double k_rr0_last() const { return S[L.rrb + 24]; }
    // scale-block accessors (uniform addresses -> scalar loads)
    __device__ __forceinline__ const double *Wloc() const { return sc + kScW; }
    __device__ __forceinline__ const double *Eloc() const { return sc + kScE; }
    // K: the first and the last steering variable (stages 0 and N-2) and their box rows have their own Ruiz factors (po_scale.hpp)
    __device__ __forceinline__ bool k_end(int j) const { return F == F_K && (j == 0 || j == N - 2); }
    __device__ __forceinline__ const double *Wloc(int j) const { return sc + kScW + (k_end(j) ? kScAlt : 0); }
    __device__ __forceinline__ const double *Eloc(int j) const { return sc + kScE + (k_end(j) ? kScAlt : 0); }
    __device__ __forceinline__ double sig(int v, int j) const { return sc[kScSig + ((v == 2 && k_end(j)) ? kKEndVar : v)]; }
    __device__ __forceinline__ double cD(int v, int j) const { return sc[kScCD + ((v == 2 && k_end(j)) ? kKEndVar : v)]; }
    __device__ __forceinline__ const double *Wdyn() const { return sc + kScW + T::NLOC; }
    __device__ __forceinline__ const double *Edyn() const { return sc + kScE + T::NLOC; }
    // a pass's step of dynamics row r (rho_eq x its weight) and the row's equilibration factor: the same for every lane and alive for the whole pass.  The fixed-length
    // kernels keep them in scalar registers (uni(), po_device.hpp) — fewer vector registers to spill around the row loops; the generic kernels leave them where they were.
    __device__ __forceinline__ double eq_row_step(double rho_eq, int r) const { const double v = rho_eq * Wdyn()[r]; if constexpr (NFIX > 0) return uni(v); else return v; }
    __device__ __forceinline__ double eq_row_scale(int r) const { const double v = Edyn()[r]; if constexpr (NFIX > 0) return uni(v); else return v; }
    __device__ __forceinline__ const double *Wctl() const { return sc + kScW + T::NLOC + T::NDYN; }
    __device__ __forceinline__ const double *Ectl() const { return sc + kScE + T::NLOC + T::NDYN; }
    __device__ __forceinline__ const double *Wend() const { return sc + kScW + T::NLOC + T::NDYN + T::NCTL; }
    __device__ __forceinline__ const double *Eend() const { return sc + kScE + T::NLOC + T::NDYN + T::NCTL; }
    __device__ __forceinline__ double sig(int v) const { return sc[kScSig + v]; }
    __device__ __forceinline__ double cD(int v) const { return sc[kScCD + v]; }
    __device__ __forceinline__ StageIn stage_in(const LS &st, int q) const {
        StageIn s;
#pragma unroll
        for (int c = 0; c < 4; ++c) { s.lb[c] = st.lb[q][c]; s.ub[c] = st.ub[q][c]; }
        s.maxk = st.maxk[q];
        s.elo = elo; s.ehi = ehi; s.j = stage(q); s.N = N; s.last = (stage(q) == N - 1);
        return s;
    }
    __device__ __forceinline__ Dyn<F> dyn_in(const LS &st, int q) const { return make_dyn_tr<F>(st.kin[q], st.dsin[q], st.trin[F == F_K ? q : 0], P); }
    __device__ __forceinline__ Dyn<F> dyn_out(const LS &st, int q) const {
        return q + 1 < SPL ? make_dyn_tr<F>(st.kin[q + 1 < SPL ? q + 1 : q], st.dsin[q + 1 < SPL ? q + 1 : q], st.trin[F == F_K ? (q + 1 < SPL ? q + 1 : q) : 0], P)
                           : make_dyn_tr<F>(st.kout, st.dsout, st.trout, P);
    }

    // ---- one-time load of everything this thread owns (coalesced HBM reads) ----
    // row classes are a function of the (scaled) bounds only: fixed for the whole solve
    __device__ __forceinline__ void bound_classes(LS &st) const {
        st.clse = st.clsc = 0;
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            st.cls[q] = 0;
            if (stage(q) < N) {
                const StageIn si = stage_in(st, q);
                ClassFn cf{0u, Eloc(stage(q))};
                local_rows<F>(si, P, cf);
                st.cls[q] = cf.cls;
                if (T::NEND && si.last) { ClassFn ce{0u, Eend()}; end_rows<F>(si, P, ce); st.clse = ce.cls; }
            }
        }
        if constexpr (T::HAS_U) { ClassFn cc{0u, Ectl()}; ctl_rows<F>(st.mkp, cc); st.clsc = cc.cls; }
    }
    __device__ __forceinline__ void load(LS &st) const {
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
#pragma unroll
            for (int a = 0; a < 3 + T::NS; ++a) st.x[q][a] = 0;
#pragma unroll
            for (int r = 0; r < T::NLOC; ++r) st.vl[q][r] = 0;
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) st.vd[q][r] = 0;
#pragma unroll
            for (int s = 0; s < T::NS; ++s) { st.hi[q][s] = 0; st.gs[q][s] = 0; st.hv[q][s][0] = st.hv[q][s][1] = st.hv[q][s][2] = 0; }
            st.maxk[q] = 0; st.kin[q] = 0; st.dsin[q] = 1.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) { st.lb[q][c] = -1; st.ub[q][c] = 1; }
            if (j < N) {
                const double4 *bp = reinterpret_cast<const double4 *>(in.bounds + (po + j) * 8);
                const double4 b0 = bp[0], b1 = bp[1];
                st.lb[q][0] = b0.x; st.ub[q][0] = b0.y; st.lb[q][1] = b0.z; st.ub[q][1] = b0.w;
                st.lb[q][2] = b1.x; st.ub[q][2] = b1.y; st.lb[q][3] = b1.z; st.ub[q][3] = b1.w;
                if constexpr (F == F_KPC) st.maxk[q] = in.max_k[po + j];
                if (j >= 1) { st.kin[q] = in.ref_k[po + j - 1]; st.dsin[q] = __dsub_rn(in.ref_s[po + j], in.ref_s[po + j - 1]); }
            }
        }
        const int jl = stage(SPL - 1);
        st.kout = 0; st.dsout = 1.0;
        if (jl + 1 < N) { st.kout = in.ref_k[po + jl]; st.dsout = __dsub_rn(in.ref_s[po + jl + 1], in.ref_s[po + jl]); }
        st.trout[0] = st.trout[1] = 0;
        if constexpr (F == F_K) {
            k_trig(st.kout, st.dsout, P, st.trout);
#pragma unroll
            for (int q = 0; q < SPL; ++q) k_trig(st.kin[q], st.dsin[q], P, st.trin[q]);
        } else { st.trin[0][0] = st.trin[0][1] = 0; }
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) st.vdo[r] = 0;
        st.vend[0] = st.vend[1] = 0;
        st.bin0[0] = st.bin0[1] = st.bin0[2] = 0;
        if constexpr (F == F_K) { st.bin0[0] = -in.x0[b * 3 + 1]; st.bin0[1] = -in.x0[b * 3 + 0]; }
        else { st.bin0[0] = -in.x0[b * 3 + 0]; st.bin0[1] = -in.x0[b * 3 + 1]; st.bin0[2] = -in.x0[b * 3 + 2]; }
        st.su = st.hiu = st.hus = st.gsu = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g) { st.u[g] = 0; st.bxu[g] = 0; st.vc[g][0] = st.vc[g][1] = st.vc[g][2] = 0; }
        st.mkp = (F == F_KPC && has_ctl()) ? in.max_kp[po + clane()] : 0.0;
        bound_classes(st);
        // NaN among the inputs this lane read.  A NaN BOUND would otherwise vanish silently (fmin / fmax drop a NaN operand: the row would act as
        // unbounded and the path come back "solved" with an obstacle ignored); NaN curvature / arc length / start state reach the iterate and are
        // caught there as well, but are reported before any work is done.
        int nn = nan_bits(st.kout) | nan_bits(st.dsout) | nan_bits(st.bin0[0]) | nan_bits(st.bin0[1]) | nan_bits(st.bin0[2]) | nan_bits(st.mkp);
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            nn |= nan_bits(st.kin[q]) | nan_bits(st.dsin[q]) | nan_bits(st.maxk[q]);
#pragma unroll
            for (int c = 0; c < 4; ++c) nn |= nan_bits(st.lb[q][c]) | nan_bits(st.ub[q][c]);
        }
        if (tid == 0) nn |= nan_bits(in.goal_z[b]) | nan_bits(in.ref_z[po + N - 1]);
        nan_in = nn;
    }
    // block-uniform: did any lane read a NaN input?  (uses the first words of the still unused dynamic LDS, like classify())
    __device__ __forceinline__ bool inputs_have_nan() const {
        const bool wave_bad = __any(nan_in) != 0;
        if constexpr (NT > 64) {
            if ((tid & 63) == 0) S[tid >> 6] = wave_bad ? 1.0 : 0.0;
            __syncthreads();
            bool any_bad = false;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) any_bad = any_bad || S[w] != 0.0;
            __syncthreads();
            return any_bad;
        } else return wave_bad;
    }

// ==================== [single_level] ====================
// members of Fast, part 1: the SINGLE-LEVEL mapping (TWO == false; NWX 1, NFIX 0).  Every lane owns SPL consecutive stages and control `tid`
// for any keep; the linear solve is ONE sequential substitution over all N stages on lanes 0..3 of wave 0 (one matrix row per lane, operands through v_readlane,
// factor rows prefetched).  The shapes the two-level mapping does not cover run here.  Nothing in this section is instantiated when TWO, except rescale_pass at its end,
// which both mappings use (registers only).
//   LDS     fac [N][18] = (G -> Ginv 0..5 | E -> L 6..14 | ws -> l_u 15..17), facu [C][4] = (1 / p_u, l_x): written by factor_blocks, replaced in place by factor_chain;
//           wt (= bz: idle while factorising) and tk: factor_blocks' hand-over to factor_chain; bz, bu, tk: right-hand side (rhs_pass) -> solution (chain_solve),
//           read back by update_pass; residual_pass publishes x through bz / bu (publish_x); the cross-wave reductions (NT > 64) go through wt = bz as well
//   lanes   reads the inputs load() left; factor_blocks writes hi, hv, hiu, hus; rhs_pass gs, gsu; update_pass x, u, su and every v; rescale_pass every v
//   called  admm_loop<UNI = false> ([loops]) from solve_kernel_fast<.., TWO = false, ..>: factor_blocks + factor_chain per factorisation, then per iteration
//           rhs_pass -> chain_solve -> update_pass<CERT>, residual_pass at the checks, rescale_pass when rho changes
// Cert (declared here) is also the return type of update_pass_two: this section stays ahead of [two_update].
    // ---- factor step A: per-stage blocks into LDS (18 doubles per stage: G 0..5 | E 6..14 | ws 15..17; the control's pivot in facu) ----
    __device__ __forceinline__ void factor_blocks(LS &st, double rho) const {
        const double rho_eq = kRhoEqOverIneq * rho;
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            HessFn h(rho, rho_eq, Wloc(j), Eloc(j), st.cls[q]);
            local_rows<F>(si, P, h);
            if (T::NEND && si.last) { h.W = Wend(); h.E = Eend(); h.cls = st.clse; end_rows<F>(si, P, h); }
            h.H[HessFn::idx(0, 0)] += sig(0, j) + p_diag_node<F>(0, j, N, P);
            h.H[HessFn::idx(1, 1)] += sig(1, j) + p_diag_node<F>(1, j, N, P);
            h.H[HessFn::idx(2, 2)] += sig(2, j) + p_diag_node<F>(2, j, N, P);
            h.H[HessFn::idx(3, 3)] += sig(3, j) + P.w_s1;
            h.H[HessFn::idx(4, 4)] += sig(4, j) + P.w_s2;
            double G[6] = {h.H[HessFn::idx(0, 0)], h.H[HessFn::idx(0, 1)], h.H[HessFn::idx(0, 2)],
                           h.H[HessFn::idx(1, 1)], h.H[HessFn::idx(1, 2)], h.H[HessFn::idx(2, 2)]};
#pragma unroll
            for (int s = 0; s < T::NS; ++s) {
                const double hi = 1.0 / h.H[HessFn::idx(3 + s, 3 + s)];
                const double hv[3] = {h.H[HessFn::idx(0, 3 + s)], h.H[HessFn::idx(1, 3 + s)], h.H[HessFn::idx(2, 3 + s)]};
                st.hi[q][s] = hi; st.hv[q][s][0] = hv[0]; st.hv[q][s][1] = hv[1]; st.hv[q][s][2] = hv[2];
                G[0] -= hv[0] * hv[0] * hi; G[1] -= hv[0] * hv[1] * hi; G[2] -= hv[0] * hv[2] * hi;
                G[3] -= hv[1] * hv[1] * hi; G[4] -= hv[1] * hv[2] * hi; G[5] -= hv[2] * hv[2] * hi;
            }
            double re[T::NDYN];  // equality rows: rho_eq * E^2 / c per dynamics row
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) {
                re[r] = eq_row_step(rho_eq, r);
                const int t = dyn_tau<F>(r);
                G[t == 0 ? 0 : (t == 1 ? 3 : 5)] += re[r];
            }
            double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, ws[3] = {0, 0, 0}, wt[3] = {0, 0, 0};
            if (j < N - 1) {
                const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const int t = dyn_tau<F>(r);
                    G[0] += re[r] * d.f[r][0] * d.f[r][0]; G[1] += re[r] * d.f[r][0] * d.f[r][1]; G[2] += re[r] * d.f[r][0] * d.f[r][2];
                    G[3] += re[r] * d.f[r][1] * d.f[r][1]; G[4] += re[r] * d.f[r][1] * d.f[r][2]; G[5] += re[r] * d.f[r][2] * d.f[r][2];
#pragma unroll
                    for (int c = 0; c < 3; ++c) { E[t * 3 + c] += -re[r] * d.f[r][c]; ws[c] += re[r] * d.beta[r] * d.f[r][c]; }
                    wt[t] += -re[r] * d.beta[r];  // M[u_{c(j)}, Z_{j+1}]
                }
                if constexpr (F == F_K) { if (j + 1 <= N - 2) E[8] += -P.w_cr; }
            }
            double *f = S + L.fac + 18 * j;
#pragma unroll
            for (int i = 0; i < 6; ++i) f[i] = G[i];
#pragma unroll
            for (int i = 0; i < 9; ++i) f[6 + i] = E[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) { f[15 + i] = ws[i]; S[L.wt + 3 * j + i] = wt[i]; }
            // beta^2 contribution of transition j to its control's pivot (summed by the control's owner below)
            double bb = 0;
            if (j < N - 1) { const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) bb += re[r] * d.beta[r] * d.beta[r]; }
            S[L.tk + j] = bb;
        }
        __syncthreads();
        if constexpr (T::HAS_U) {
            if (tid < C) {
                HessFn h(rho, rho_eq, Wctl(), Ectl(), st.clsc);
                ctl_rows<F>(st.mkp, h);
                double huu = h.H[HessFn::idx(2, 2)] + sig(5) + P.w_u;
                if constexpr (T::HAS_SU) {
                    const double hi = 1.0 / (h.H[HessFn::idx(3, 3)] + sig(6) + P.w_su);
                    st.hiu = hi; st.hus = h.H[HessFn::idx(2, 3)];
                    huu -= st.hus * st.hus * hi;
                }
                const int i0 = tid * keep, i1 = min(i0 + keep, N - 1);
                for (int i = i0; i < i1; ++i) huu += S[L.tk + i];
                S[L.facu + 4 * tid] = huu;
            }
        }
        __syncthreads();
    }

    // ---- factor step B: sequential block LDL' on broadcast LDS reads (wave 0; lane 0 stores) ----
    __device__ __forceinline__ void factor_chain() const {
        if (tid < 64) {
            double G[6], w[3] = {0, 0, 0}, pu = 0;
            const double *f0 = S + L.fac;
#pragma unroll
            for (int i = 0; i < 6; ++i) G[i] = f0[i];
            if constexpr (T::HAS_U) { w[0] = f0[15]; w[1] = f0[16]; w[2] = f0[17]; pu = S[L.facu]; }
            int c = 0, gcnt = 0;
            for (int j = 0; j < N; ++j) {
                double *f = S + L.fac + 18 * j;
                double Gi[6];
                inv3_sym(G, Gi);
                if (j == N - 1) {
                    if (tid == 0) {
#pragma unroll
                        for (int i = 0; i < 6; ++i) f[i] = Gi[i];
                    }
                    break;
                }
                double E[9], Gn[6], wsn[3], wn[3];
#pragma unroll
                for (int i = 0; i < 9; ++i) E[i] = f[6 + i];
#pragma unroll
                for (int i = 0; i < 6; ++i) Gn[i] = f[18 + i];
#pragma unroll
                for (int i = 0; i < 3; ++i) { wsn[i] = f[18 + 15 + i]; wn[i] = S[L.wt + 3 * j + i]; }
                const double Gf[9] = {Gi[0], Gi[1], Gi[2], Gi[1], Gi[3], Gi[4], Gi[2], Gi[4], Gi[5]};
                double Ln[9];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) Ln[r * 3 + k] = E[r * 3 + 0] * Gf[k] + E[r * 3 + 1] * Gf[3 + k] + E[r * 3 + 2] * Gf[6 + k];
                Gn[0] -= Ln[0] * E[0] + Ln[1] * E[1] + Ln[2] * E[2];
                Gn[1] -= Ln[0] * E[3] + Ln[1] * E[4] + Ln[2] * E[5];
                Gn[2] -= Ln[0] * E[6] + Ln[1] * E[7] + Ln[2] * E[8];
                Gn[3] -= Ln[3] * E[3] + Ln[4] * E[4] + Ln[5] * E[5];
                Gn[4] -= Ln[3] * E[6] + Ln[4] * E[7] + Ln[5] * E[8];
                Gn[5] -= Ln[6] * E[6] + Ln[7] * E[7] + Ln[8] * E[8];
                double lu[3] = {0, 0, 0};
                if constexpr (T::HAS_U) {
                    lu[0] = Gf[0] * w[0] + Gf[1] * w[1] + Gf[2] * w[2];
                    lu[1] = Gf[3] * w[0] + Gf[4] * w[1] + Gf[5] * w[2];
                    lu[2] = Gf[6] * w[0] + Gf[7] * w[1] + Gf[8] * w[2];
#pragma unroll
                    for (int r = 0; r < 3; ++r) wn[r] -= E[r * 3 + 0] * lu[0] + E[r * 3 + 1] * lu[1] + E[r * 3 + 2] * lu[2];
                    pu -= lu[0] * w[0] + lu[1] * w[1] + lu[2] * w[2];
                    ++gcnt;
                    if (gcnt == keep || j == N - 2) {
                        gcnt = 0;
                        const double pi = 1.0 / pu;
                        const double lx[3] = {wn[0] * pi, wn[1] * pi, wn[2] * pi};
                        Gn[0] -= lx[0] * wn[0]; Gn[1] -= lx[0] * wn[1]; Gn[2] -= lx[0] * wn[2];
                        Gn[3] -= lx[1] * wn[1]; Gn[4] -= lx[1] * wn[2]; Gn[5] -= lx[2] * wn[2];
                        if (tid == 0) { double *fu = S + L.facu + 4 * c; fu[0] = pi; fu[1] = lx[0]; fu[2] = lx[1]; fu[3] = lx[2]; }
                        ++c;
                        if (j + 1 <= N - 2) { w[0] = wsn[0]; w[1] = wsn[1]; w[2] = wsn[2]; pu = S[L.facu + 4 * c]; }
                    } else {
                        w[0] = wn[0] + wsn[0]; w[1] = wn[1] + wsn[1]; w[2] = wn[2] + wsn[2];
                    }
                }
                __builtin_amdgcn_wave_barrier();
                if (tid == 0) {
#pragma unroll
                    for (int i = 0; i < 6; ++i) f[i] = Gi[i];
#pragma unroll
                    for (int i = 0; i < 9; ++i) f[6 + i] = Ln[i];
                    f[15] = lu[0]; f[16] = lu[1]; f[17] = lu[2];
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) G[i] = Gn[i];
            }
        }
        __syncthreads();
    }

    // ---- rhs pass (registers -> b in LDS) ----
    __device__ __forceinline__ void rhs_pass(LS &st, double rho, bool first) const {
        const double rho_eq = kRhoEqOverIneq * rho;
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            RhsFn fn;
            fn.rho = rho; fn.rho_eq = rho_eq; fn.first = first; fn.W = Wloc(j); fn.E = Eloc(j); fn.cls = st.cls[q];
#pragma unroll
            for (int a = 0; a < 5; ++a) fn.g[a] = a < 3 + T::NS ? sig(a, j) * st.x[q][a] : 0.0;
            fn.v = st.vl[q]; fn.stride = 1;
            local_rows<F>(si, P, fn);
            if (T::NEND && si.last) { fn.v = st.vend; fn.W = Wend(); fn.E = Eend(); fn.cls = st.clse; end_rows<F>(si, P, fn); }
            double re[T::NDYN];
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) re[r] = eq_row_step(rho_eq, r);
            // rows into stage j
            double tkj = 0;
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) { const double t = first ? 0.0 : re[r] * (2.0 * st.bin0[r] - st.vd[q][r]); fn.g[dyn_tau<F>(r)] -= t; }
            } else {
                const Dyn<F> d = dyn_in(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double t = first ? 0.0 : re[r] * (2.0 * d.b[r] - st.vd[q][r]);
                    fn.g[dyn_tau<F>(r)] -= t;
                    tkj += t * d.beta[r];
                }
            }
            if constexpr (T::HAS_U) { if (j >= 1) S[L.tk + j - 1] = tkj; }  // contribution of transition j-1 to b_u
            // rows out of stage j
            if (j < N - 1) {
                const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double vv = q + 1 < SPL ? st.vd[q + 1 < SPL ? q + 1 : q][r] : st.vdo[r];
                    const double t = first ? 0.0 : re[r] * (2.0 * d.b[r] - vv);
                    fn.g[0] += t * d.f[r][0]; fn.g[1] += t * d.f[r][1]; fn.g[2] += t * d.f[r][2];
                }
            }
#pragma unroll
            for (int s = 0; s < T::NS; ++s) {
                const double w = fn.g[3 + s] * st.hi[q][s];
                fn.g[0] -= st.hv[q][s][0] * w; fn.g[1] -= st.hv[q][s][1] * w; fn.g[2] -= st.hv[q][s][2] * w;
                st.gs[q][s] = fn.g[3 + s];
            }
            S[L.bz + 3 * j + 0] = fn.g[0]; S[L.bz + 3 * j + 1] = fn.g[1]; S[L.bz + 3 * j + 2] = fn.g[2];
        }
        if constexpr (T::HAS_U) {
            __syncthreads();
            if (tid < C) {
                RhsFn fn;
                fn.rho = rho; fn.rho_eq = rho_eq; fn.first = first; fn.W = Wctl(); fn.E = Ectl(); fn.cls = st.clsc;
                fn.g[0] = fn.g[1] = fn.g[4] = 0;
                fn.g[2] = sig(5) * st.u[0];
                fn.g[3] = T::HAS_SU ? sig(6) * st.su : 0.0;
                fn.v = st.vc[0]; fn.stride = 1;
                ctl_rows<F>(st.mkp, fn);
                const int i0 = tid * keep, i1 = min(i0 + keep, N - 1);
                for (int i = i0; i < i1; ++i) fn.g[2] += S[L.tk + i];
                if constexpr (T::HAS_SU) { fn.g[2] -= st.hus * fn.g[3] * st.hiu; st.gsu = fn.g[3]; }
                S[L.bu + tid] = fn.g[2];
            }
        }
        __syncthreads();
    }

    // ---- chain solve on lanes 0..3 of wave 0: lane r holds row r of [Ln; lu] (forward) / column r (backward) ----
    // keep == 4 fast path: one control group (4 transitions) per loop trip, the next group's factor rows and
    // right-hand sides prefetched a whole group ahead so that no LDS latency sits on the dependent chain;
    // every lane stores (lane 3 to a dummy slot) so the loop body never touches the exec mask.
    __device__ __forceinline__ void chain_forward_generic(int j0, double &y0, double &y1, double &y2, double &acc, int &c, int gcnt) const {
        double *bz = S + L.bz, *bu = S + L.bu;
        const double *fac = S + L.fac, *facu = S + L.facu;
        const int r = tid, rr = r < 3 ? r : 0;
        for (int j = j0; j < N - 1; ++j) {
            const double *f = fac + 18 * j;
            double res = (r < 3 ? bz[3 * (j + 1) + rr] : acc);
            res = fma(-f[6 + 3 * r], y0, res); res = fma(-f[7 + 3 * r], y1, res); res = fma(-f[8 + 3 * r], y2, res);
            if constexpr (T::HAS_U) {
                ++gcnt;
                if (gcnt == keep || j == N - 2) {
                    gcnt = 0;
                    const double yu = bcast(res, 3);
                    const double lxr = facu[4 * c + 1 + rr];
                    if (r == 3) bu[c] = yu;
                    ++c;
                    const double nacc = bu[c];
                    res = r < 3 ? fma(-lxr, yu, res) : nacc;
                }
                acc = res;
            }
            if (r < 3) bz[3 * (j + 1) + r] = res;
            y0 = bcast(res, 0); y1 = bcast(res, 1); y2 = bcast(res, 2);
        }
    }
    __device__ __forceinline__ void chain_backward_generic(int j0, int jstop, double &x0, double &x1, double &x2, int &c, int gcnt, bool gend) const {
        double *bz = S + L.bz, *bu = S + L.bu;
        const double *fac = S + L.fac, *facu = S + L.facu;
        const int r = tid, rr = r < 3 ? r : 0;
        double xu = 0;
        if constexpr (T::HAS_U) { if (!gend && c < C) xu = bu[c]; }
        for (int j = j0; j >= jstop; --j) {
            const double *f = fac + 18 * j;
            if constexpr (T::HAS_U) {
                if (gend) {
                    --c;
                    const double *fu = facu + 4 * c;
                    xu = bu[c];
                    xu = fma(-fu[1], x0, xu); xu = fma(-fu[2], x1, xu); xu = fma(-fu[3], x2, xu);
                    if (r == 3) bu[c] = xu;
                }
                --gcnt;
                gend = (gcnt == 0);
                if (gend) gcnt = keep;
            }
            double res = bz[3 * j + rr];
            res = fma(-f[6 + rr], x0, res); res = fma(-f[9 + rr], x1, res); res = fma(-f[12 + rr], x2, res);
            if constexpr (T::HAS_U) res = fma(-f[15 + rr], xu, res);
            if (r < 3) bz[3 * j + r] = res;
            x0 = bcast(res, 0); x1 = bcast(res, 1); x2 = bcast(res, 2);
        }
    }

    struct FwdGroup { double cf[4][3], base[4], lx, nacc; };
    __device__ __forceinline__ void load_fwd_group(FwdGroup &g, int c) const {
        const double *bz = S + L.bz, *bu = S + L.bu;
        const double *fac = S + L.fac, *facu = S + L.facu;
        const int r = tid, rr = r < 3 ? r : 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = 4 * c + s;
            const double *f = fac + 18 * j + 6 + 3 * r;
            g.cf[s][0] = f[0]; g.cf[s][1] = f[1]; g.cf[s][2] = f[2];
            g.base[s] = bz[3 * (j + 1) + rr];
        }
        g.lx = facu[4 * c + 1 + rr];
        g.nacc = bu[c + 1];
    }
    struct BwdGroup { double cf[4][4], base[4], fu[3], ybu; };
    __device__ __forceinline__ void load_bwd_group(BwdGroup &g, int c) const {
        const double *bz = S + L.bz, *bu = S + L.bu;
        const double *fac = S + L.fac, *facu = S + L.facu;
        const int r = tid, rr = r < 3 ? r : 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = 4 * c + s;
            const double *f = fac + 18 * j + 6 + rr;
            g.cf[s][0] = f[0]; g.cf[s][1] = f[3]; g.cf[s][2] = f[6]; g.cf[s][3] = f[9];
            g.base[s] = bz[3 * j + rr];
        }
        g.fu[0] = facu[4 * c + 1]; g.fu[1] = facu[4 * c + 2]; g.fu[2] = facu[4 * c + 3];
        g.ybu = bu[c];
    }

    __device__ __forceinline__ void chain_solve() const {
        double *bz = S + L.bz, *bu = S + L.bu;
        const double *fac = S + L.fac, *facu = S + L.facu;
        const bool g4 = T::HAS_U && keep == 4;
        const int cfull = g4 ? (N - 1) / 4 : 0;  // groups with all 4 transitions
        if (tid < 4) {
            const int r = tid;
            double y0 = bz[0], y1 = bz[1], y2 = bz[2];
            double acc = T::HAS_U ? bu[0] : 0.0;
            int c = 0;
            if (g4 && cfull > 0) {
                double *dummy = S + L.tk;  // lane 3's store target (tk is dead during the solve)
                double *st_bz = r < 3 ? bz + r : dummy;
                const int st_mul = r < 3 ? 3 : 0;
                FwdGroup cur, nxt;
                load_fwd_group(cur, 0);
                for (; c < cfull; ++c) {
                    load_fwd_group(nxt, c + 1 < cfull ? c + 1 : c);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int j = 4 * c + s;
                        double res = (r < 3 ? cur.base[s] : acc);
                        res = fma(-cur.cf[s][0], y0, res); res = fma(-cur.cf[s][1], y1, res); res = fma(-cur.cf[s][2], y2, res);
                        if (s == 3) {
                            const double yu = bcast(res, 3);
                            bu[c] = yu;  // all four lanes store the same value
                            res = r < 3 ? fma(-cur.lx, yu, res) : cur.nacc;
                        }
                        acc = res;
                        st_bz[st_mul * (j + 1)] = res;
                        y0 = bcast(res, 0); y1 = bcast(res, 1); y2 = bcast(res, 2);
                    }
                    cur = nxt;
                }
                chain_forward_generic(4 * cfull, y0, y1, y2, acc, c, 0);
            } else {
                chain_forward_generic(0, y0, y1, y2, acc, c, 0);
            }
        }
        __syncthreads();
        // ---------------- diagonal: y <- D^-1 y (all threads) ----------------
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const double *f = fac + 18 * j;
            const double a0 = bz[3 * j], a1 = bz[3 * j + 1], a2 = bz[3 * j + 2];
            bz[3 * j] = f[0] * a0 + f[1] * a1 + f[2] * a2;
            bz[3 * j + 1] = f[1] * a0 + f[3] * a1 + f[4] * a2;
            bz[3 * j + 2] = f[2] * a0 + f[4] * a1 + f[5] * a2;
        }
        if constexpr (T::HAS_U) { if (tid < C) bu[tid] *= facu[4 * tid]; }
        __syncthreads();
        // ---------------- backward: L' x = y ----------------
        if (tid < 4) {
            const int r = tid;
            double x0 = bz[3 * (N - 1)], x1 = bz[3 * (N - 1) + 1], x2 = bz[3 * (N - 1) + 2];
            int c = C;
            if (g4 && cfull > 0) {
                // partial last group (transitions 4*cfull .. N-2), then full groups cfull-1 .. 0
                if (4 * cfull < N - 1) chain_backward_generic(N - 2, 4 * cfull, x0, x1, x2, c, (N - 1) - 4 * cfull, true);
                // after the generic part c == cfull
                double *dummy = S + L.tk;
                double *st_bz = r < 3 ? bz + r : dummy;
                const int st_mul = r < 3 ? 3 : 0;
                BwdGroup cur, nxt;
                load_bwd_group(cur, cfull - 1);
                for (c = cfull - 1; c >= 0; --c) {
                    load_bwd_group(nxt, c > 0 ? c - 1 : 0);
                    double xu = cur.ybu;
                    xu = fma(-cur.fu[0], x0, xu); xu = fma(-cur.fu[1], x1, xu); xu = fma(-cur.fu[2], x2, xu);
                    bu[c] = xu;
#pragma unroll
                    for (int s = 3; s >= 0; --s) {
                        const int j = 4 * c + s;
                        double res = cur.base[s];
                        res = fma(-cur.cf[s][0], x0, res); res = fma(-cur.cf[s][1], x1, res); res = fma(-cur.cf[s][2], x2, res);
                        res = fma(-cur.cf[s][3], xu, res);
                        st_bz[st_mul * j] = res;
                        x0 = bcast(res, 0); x1 = bcast(res, 1); x2 = bcast(res, 2);
                    }
                    cur = nxt;
                }
            } else {
                int gcnt = 0;
                if constexpr (T::HAS_U) gcnt = (N - 1) - (C - 1) * keep;
                chain_backward_generic(N - 2, 0, x0, x1, x2, c, gcnt, true);
            }
        }
        __syncthreads();
    }

    struct Cert { double ndy, sup, natdy; };

    // ---- update pass: recover slacks, ztilde = A xtilde, v += alpha (ztilde - zc), x += alpha (xtilde - x) ----
    // CERT: also evaluate the ingredients of OSQP's primal infeasibility certificate on this iteration's delta_y.
    template <bool CERT> __device__ __forceinline__ Cert update_pass(LS &st, bool first, double rho) const {
        const double al = P.alpha;
        const double rho_eq = kRhoEqOverIneq * rho;
        const double *bz = S + L.bz, *bu = S + L.bu;
        double *tk = S + L.tk;
        Cert ct = {0, 0, 0};
        double re[T::NDYN], dy_next[T::NDYN];  // dy of the rows into the stage processed just before (q+1)
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) { re[r] = eq_row_step(rho_eq, r); dy_next[r] = 0; }
#pragma unroll
        for (int q = SPL - 1; q >= 0; --q) {  // descending: the rows OUT of stage q are the rows INTO q+1, handled one step earlier
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            typename std::conditional<CERT, UpdCertFn, UpdFn>::type fn;
            fn.alpha = al; fn.first = first;
            if constexpr (CERT) {
                fn.rho = rho; fn.rho_eq = rho_eq; fn.W = Wloc(j); fn.E = Eloc(j); fn.cls = st.cls[q]; fn.ndy = 0; fn.sup = 0;
#pragma unroll
                for (int a = 0; a < 5; ++a) fn.ady[a] = 0;
            }
            fn.xt[0] = bz[3 * j]; fn.xt[1] = bz[3 * j + 1]; fn.xt[2] = bz[3 * j + 2];
            fn.xt[3] = fn.xt[4] = 0;
#pragma unroll
            for (int s = 0; s < T::NS; ++s)
                fn.xt[3 + s] = (st.gs[q][s] - (st.hv[q][s][0] * fn.xt[0] + st.hv[q][s][1] * fn.xt[1] + st.hv[q][s][2] * fn.xt[2])) * st.hi[q][s];
            fn.v = st.vl[q]; fn.stride = 1;
            local_rows<F>(si, P, fn);
            if (T::NEND && si.last) {
                fn.v = st.vend;
                if constexpr (CERT) { fn.W = Wend(); fn.E = Eend(); fn.cls = st.clse; }
                end_rows<F>(si, P, fn);
            }
            double dy_out[T::NDYN];  // rows out of stage q
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) dy_out[r] = dy_next[r];
            if (q == SPL - 1 && j < N - 1) {  // identical update of the copy of the next thread's incoming rows
                const Dyn<F> d = dyn_out(st, q);
                const double ut = T::HAS_U ? bu[ctl_index(j, keep)] : 0.0;
                const double nx[3] = {bz[3 * j + 3], bz[3 * j + 4], bz[3 * j + 5]};
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double zt = d.f[r][0] * fn.xt[0] + d.f[r][1] * fn.xt[1] + d.f[r][2] * fn.xt[2] + d.beta[r] * ut - nx[dyn_tau<F>(r)];
                    const double dv = al * (zt - (first ? 0.0 : d.b[r]));
                    st.vdo[r] += dv;
                    if (CERT) dy_out[r] = re[r] * dv;
                }
            }
            double dy_in[T::NDYN], bsum = 0, tkv = 0;
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double dv = al * (-fn.xt[dyn_tau<F>(r)] - (first ? 0.0 : st.bin0[r]));
                    st.vd[q][r] += dv;
                    dy_in[r] = re[r] * dv; bsum += st.bin0[r] * dy_in[r];
                }
            } else {
                const Dyn<F> d = dyn_in(st, q);
                const double p0 = bz[3 * j - 3], p1 = bz[3 * j - 2], p2 = bz[3 * j - 1];
                const double ut = T::HAS_U ? bu[ctl_index(j - 1, keep)] : 0.0;
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double zt = d.f[r][0] * p0 + d.f[r][1] * p1 + d.f[r][2] * p2 + d.beta[r] * ut - fn.xt[dyn_tau<F>(r)];
                    const double dv = al * (zt - (first ? 0.0 : d.b[r]));
                    st.vd[q][r] += dv;
                    dy_in[r] = re[r] * dv; bsum += d.b[r] * dy_in[r];
                    tkv += dy_in[r] * d.beta[r];
                }
            }
            if constexpr (CERT) {
                if constexpr (T::HAS_U) { if (j >= 1) tk[j - 1] = tkv; }  // (A' dy) contribution of transition j-1 to its control
                // equality rows: dy unrestricted, u.dy+ + l.dy- = b.dy ; A'dy on this stage's variables
                double ad[5];
#pragma unroll
                for (int a = 0; a < 5; ++a) ad[a] = fn.ady[a];
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) { ad[dyn_tau<F>(r)] -= dy_in[r]; fn.ndy = fmax(fn.ndy, fabs(dy_in[r])); }
                if (j < N - 1) {
                    const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                    for (int r = 0; r < T::NDYN; ++r) { ad[0] += dy_out[r] * d.f[r][0]; ad[1] += dy_out[r] * d.f[r][1]; ad[2] += dy_out[r] * d.f[r][2]; }
                }
#pragma unroll
                for (int a = 0; a < 3 + T::NS; ++a) ct.natdy = fmax(ct.natdy, fabs(ad[a]));
                ct.ndy = fmax(ct.ndy, fn.ndy);
                ct.sup += fn.sup + bsum;
            }
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) dy_next[r] = dy_in[r];
#pragma unroll
            for (int a = 0; a < 3 + T::NS; ++a) st.x[q][a] += al * (fn.xt[a] - st.x[q][a]);
        }
        if constexpr (CERT && T::HAS_U) __syncthreads();  // tk complete
        if constexpr (T::HAS_U) {
            if (tid < C) {
                typename std::conditional<CERT, UpdCertFn, UpdFn>::type fn;
                fn.alpha = al; fn.first = first;
                if constexpr (CERT) {
                    fn.rho = rho; fn.rho_eq = rho_eq; fn.W = Wctl(); fn.E = Ectl(); fn.cls = st.clsc; fn.ndy = 0; fn.sup = 0;
#pragma unroll
                    for (int a = 0; a < 5; ++a) fn.ady[a] = 0;
                }
                fn.xt[0] = fn.xt[1] = fn.xt[4] = 0;
                fn.xt[2] = bu[tid];
                fn.xt[3] = T::HAS_SU ? (st.gsu - st.hus * fn.xt[2]) * st.hiu : 0.0;
                fn.v = st.vc[0]; fn.stride = 1;
                ctl_rows<F>(st.mkp, fn);
                st.u[0] += al * (fn.xt[2] - st.u[0]);
                if constexpr (T::HAS_SU) st.su += al * (fn.xt[3] - st.su);
                if constexpr (CERT) {
                    double dytk = 0;
                    const int i0 = tid * keep, i1 = min(i0 + keep, N - 1);
                    for (int i = i0; i < i1; ++i) dytk += tk[i];
                    ct.natdy = fmax(ct.natdy, fabs(fn.ady[2] + dytk));
                    if constexpr (T::HAS_SU) ct.natdy = fmax(ct.natdy, fabs(fn.ady[3]));
                    ct.ndy = fmax(ct.ndy, fn.ndy);
                    ct.sup += fn.sup;
                }
            }
        }
        __syncthreads();  // bz/bu are rewritten by the next rhs pass (and, with CERT, by the reduction scratch below)
        if constexpr (CERT) {
            ct.ndy = wave_max(ct.ndy); ct.natdy = wave_max(ct.natdy); ct.sup = wave_sum(ct.sup);
            if constexpr (NT > 64) {
                double *red = S + L.wt;
                const int w = tid >> 6;
                if ((tid & 63) == 0) { red[w * 3] = ct.ndy; red[w * 3 + 1] = ct.natdy; red[w * 3 + 2] = ct.sup; }
                __syncthreads();
                ct.ndy = 0; ct.natdy = 0; ct.sup = 0;
                for (int k = 0; k < NT / 64; ++k) { ct.ndy = fmax(ct.ndy, red[k * 3]); ct.natdy = fmax(ct.natdy, red[k * 3 + 1]); ct.sup += red[k * 3 + 2]; }
                __syncthreads();
            }
        }
        return ct;
    }

    // ---- publish x into LDS (bz: node comps, bu: controls) for neighbour reads ----
    __device__ __forceinline__ void publish_x(const LS &st) const {
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j < N) { S[L.bz + 3 * j] = st.x[q][0]; S[L.bz + 3 * j + 1] = st.x[q][1]; S[L.bz + 3 * j + 2] = st.x[q][2]; }
        }
        if constexpr (T::HAS_U) { if (tid < C) S[L.bu + tid] = st.u[0]; }
        __syncthreads();
    }

    __device__ __forceinline__ Resid residual_pass(const LS &st, double rho) const {
        const double rho_eq = kRhoEqOverIneq * rho;
        publish_x(st);
        const double *bz = S + L.bz, *bu = S + L.bu;
        double *tk = S + L.tk;
        double m[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rp rd nAx nz nPx nAty | same, scaled
        double ob = 0;  // x'Px
        int bad = 0;    // a non-finite primal or dual value anywhere (see nonfinite_bits)
        double re[T::NDYN], ed[T::NDYN];
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) { re[r] = eq_row_step(rho_eq, r); ed[r] = eq_row_scale(r); }
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            ResFn fn;
            fn.rho = rho; fn.rho_eq = rho_eq; fn.W = Wloc(j); fn.E = Eloc(j); fn.cls = st.cls[q];
            fn.rp = fn.nAx = fn.nz = fn.rps = fn.nAxs = fn.nzs = 0;
#pragma unroll
            for (int a = 0; a < 5; ++a) { fn.x[a] = a < 3 + T::NS ? st.x[q][a] : 0.0; fn.aty[a] = 0; }
            fn.v = st.vl[q]; fn.stride = 1;
            local_rows<F>(si, P, fn);
            if (T::NEND && si.last) { fn.v = st.vend; fn.W = Wend(); fn.E = Eend(); fn.cls = st.clse; end_rows<F>(si, P, fn); }
            double bin[3] = {0, 0, 0}, ax[3] = {0, 0, 0}, ytk = 0;
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) { bin[r] = st.bin0[r]; ax[r] = -fn.x[dyn_tau<F>(r)]; }
            } else {
                const Dyn<F> d = dyn_in(st, q);
                const double p0 = bz[3 * j - 3], p1 = bz[3 * j - 2], p2 = bz[3 * j - 1];
                const double uu = T::HAS_U ? bu[ctl_index(j - 1, keep)] : 0.0;
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    bin[r] = d.b[r];
                    ax[r] = d.f[r][0] * p0 + d.f[r][1] * p1 + d.f[r][2] * p2 + d.beta[r] * uu - fn.x[dyn_tau<F>(r)];
                    ytk += re[r] * (st.vd[q][r] - d.b[r]) * d.beta[r];
                }
            }
            if constexpr (T::HAS_U) { if (j >= 1) tk[j - 1] = ytk; }
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) {
                const double y = re[r] * (st.vd[q][r] - bin[r]);
                const double a0 = fabs(ax[r] - bin[r]), a1 = fabs(ax[r]), a2 = fabs(bin[r]);
                fn.rp = fmax(fn.rp, a0); fn.nAx = fmax(fn.nAx, a1); fn.nz = fmax(fn.nz, a2);
                fn.rps = fmax(fn.rps, ed[r] * a0); fn.nAxs = fmax(fn.nAxs, ed[r] * a1); fn.nzs = fmax(fn.nzs, ed[r] * a2);
                fn.aty[dyn_tau<F>(r)] -= y;
            }
            if (j < N - 1) {
                const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double vv = q + 1 < SPL ? st.vd[q + 1 < SPL ? q + 1 : q][r] : st.vdo[r];
                    const double y = re[r] * (vv - d.b[r]);
                    fn.aty[0] += y * d.f[r][0]; fn.aty[1] += y * d.f[r][1]; fn.aty[2] += y * d.f[r][2];
                }
            }
            double px[5];
            px[0] = p_diag_node<F>(0, j, N, P) * fn.x[0];
            px[1] = 0.0;
            px[2] = p_diag_node<F>(2, j, N, P) * fn.x[2];
            if constexpr (F == F_K) {
                if (j <= N - 2) {
                    if (j >= 1) px[2] -= P.w_cr * bz[3 * (j - 1) + 2];
                    if (j + 1 <= N - 2) px[2] -= P.w_cr * bz[3 * (j + 1) + 2];
                }
            }
            px[3] = P.w_s1 * fn.x[3];
            px[4] = T::NS > 1 ? P.w_s2 * fn.x[4] : 0.0;
#pragma unroll
            for (int a = 0; a < 3 + T::NS; ++a) {
                ob += fn.x[a] * px[a];
                bad |= nonfinite_bits(fn.x[a]) | nonfinite_bits(px[a] + fn.aty[a]);
                const double g0 = fabs(px[a] + fn.aty[a]), g1 = fabs(px[a]), g2 = fabs(fn.aty[a]), cd = cD(a, j);
                m[1] = fmax(m[1], g0); m[4] = fmax(m[4], g1); m[5] = fmax(m[5], g2);
                m[7] = fmax(m[7], cd * g0); m[10] = fmax(m[10], cd * g1); m[11] = fmax(m[11], cd * g2);
            }
            m[0] = fmax(m[0], fn.rp); m[2] = fmax(m[2], fn.nAx); m[3] = fmax(m[3], fn.nz);
            m[6] = fmax(m[6], fn.rps); m[8] = fmax(m[8], fn.nAxs); m[9] = fmax(m[9], fn.nzs);
        }
        __syncthreads();
        if constexpr (T::HAS_U) {
            if (tid < C) {
                ResFn fn;
                fn.rho = rho; fn.rho_eq = rho_eq; fn.W = Wctl(); fn.E = Ectl(); fn.cls = st.clsc;
                fn.rp = fn.nAx = fn.nz = fn.rps = fn.nAxs = fn.nzs = 0;
                fn.x[0] = fn.x[1] = fn.x[4] = 0; fn.x[2] = st.u[0]; fn.x[3] = T::HAS_SU ? st.su : 0.0;
#pragma unroll
                for (int a = 0; a < 5; ++a) fn.aty[a] = 0;
                fn.v = st.vc[0]; fn.stride = 1;
                ctl_rows<F>(st.mkp, fn);
                const int i0 = tid * keep, i1 = min(i0 + keep, N - 1);
                for (int i = i0; i < i1; ++i) fn.aty[2] += tk[i];
                const double pxv[2] = {P.w_u * fn.x[2], T::HAS_SU ? P.w_su * fn.x[3] : 0.0};
#pragma unroll
                for (int a = 0; a < 1 + T::HAS_SU; ++a) {
                    ob += fn.x[2 + a] * pxv[a];
                    bad |= nonfinite_bits(fn.x[2 + a]) | nonfinite_bits(pxv[a] + fn.aty[2 + a]);
                    const double g0 = fabs(pxv[a] + fn.aty[2 + a]), g1 = fabs(pxv[a]), g2 = fabs(fn.aty[2 + a]), cd = cD(5 + a);
                    m[1] = fmax(m[1], g0); m[4] = fmax(m[4], g1); m[5] = fmax(m[5], g2);
                    m[7] = fmax(m[7], cd * g0); m[10] = fmax(m[10], cd * g1); m[11] = fmax(m[11], cd * g2);
                }
                m[0] = fmax(m[0], fn.rp); m[2] = fmax(m[2], fn.nAx); m[3] = fmax(m[3], fn.nz);
                m[6] = fmax(m[6], fn.rps); m[8] = fmax(m[8], fn.nAxs); m[9] = fmax(m[9], fn.nzs);
            }
        }
        // wavefront shuffle reductions
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = wave_max(m[i]);
        ob = wave_sum(ob);
        bad = __any(bad) ? 1 : 0;
        if constexpr (NT > 64) {  // combine the waves of the block through LDS
            __syncthreads();
            double *red = S + L.wt;
            const int w = tid >> 6;
            if ((tid & 63) == 0) {
#pragma unroll
                for (int i = 0; i < 12; ++i) red[w * 14 + i] = m[i];
                red[w * 14 + 12] = ob; red[w * 14 + 13] = bad ? 1.0 : 0.0;
            }
            __syncthreads();
            ob = 0;
            for (int k = 0; k < NT / 64; ++k) {
#pragma unroll
                for (int i = 0; i < 12; ++i) m[i] = fmax(m[i], red[k * 14 + i]);
                ob += red[k * 14 + 12];
                bad |= red[k * 14 + 13] != 0.0;
            }
        }
        __syncthreads();
        Resid R = {m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11], 0.5 * ob, bad};
        return R;
    }

    template <bool UNI = false> __device__ __forceinline__ void rescale_pass(LS &st, double ratio) const {
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            RescaleFn fn;
            fn.ratio = ratio; fn.v = st.vl[q]; fn.stride = 1; fn.cls = cls_of<UNI>(st, q);
            local_rows<F>(si, P, fn);
            if (T::NEND && si.last) { fn.v = st.vend; fn.cls = st.clse; end_rows<F>(si, P, fn); }
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) st.vd[q][r] = st.bin0[r] + ratio * (st.vd[q][r] - st.bin0[r]);
            } else {
                const Dyn<F> d = dyn_in(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) st.vd[q][r] = d.b[r] + ratio * (st.vd[q][r] - d.b[r]);
            }
            if (q == SPL - 1 && j < N - 1) {
                const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) st.vdo[r] = d.b[r] + ratio * (st.vdo[r] - d.b[r]);
            }
        }
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g)
                if (has_ctl(g)) { RescaleFn fn; fn.ratio = ratio; fn.v = st.vc[g]; fn.stride = 1; fn.cls = st.clsc; ctl_rows<F>(st.mkp, fn); }
        }
    }


// ==================== [two_prims] ====================
// members of Fast, part 2: the primitives of the TWO-LEVEL mapping, shared by all of its lane layouts (NWX 1 .. 5) and by every later section.
// TWO only.  Chunk geometry (nq_* / nst_*: the transitions / stages of the own chunk, and of the own lane's share of it, that exist); the 9-record layout of fac and
// phi (idx9, load9 / store9: four 16-byte pairs + a single per lane) with the accessors FA / FAt (fac), FU / FUg / FUc (facu), PL (phi), RS (rseg); lane moves of a
// double (dpp_mov / dpp_mov0, xchg, wshfl); the regenerated coupling block (apply_E, apply_Et) and Ginv products (mul_Gr, mul_G).
//   LDS     the accessors address fac, facu, phi, rseg; xchg uses the mailboxes at ex (NT > 64 only: one barrier); nothing else is touched
//   lanes   no LaneState field is read or written here
//   called  from every two-level section below ([two_*], [newton_passes], [polish_passes])
    // =====================================================================================================
    // TWO-LEVEL MODE (keep == SPL, or no held controls): thread t's chunk == control group t.
    //
    //  * factor stored per stage as (Ginv_j, w_j): the coupling block E_j = M[Z_{j+1},Z_j] is never stored — it
    //    is 5 numbers regenerated from (ds_j, k_ref_j):  L_j = E_j Ginv_j,  l_u = Ginv_j w_j.
    //  * local sweeps inside a chunk run lane-parallel on registers + the thread's own (SoA) factor columns;
    //  * the 3-vector at each chunk boundary obeys  s_t = beta_t + Phi_t s_{t-1}:  solved by a Kogge-Stone scan
    //    over lanes with the prefix products P^(l)_t = Phi_t ... Phi_{t-2^l+1} precomputed at every factorisation
    //    (backward: X_t = gamma_t + Phi_t' X_{t+1}, whose span products are the transposes of the same P^(l)).
    // =====================================================================================================
    // transitions / stages of the own chunk that exist (the chunk that holds the final stage is partial), and of the own share of it
    __device__ __forceinline__ int nq_chunk() const { const int r = N - 1 - CH * clane(); return r < 0 ? 0 : (r > CH ? CH : r); }
    __device__ __forceinline__ int nst_chunk() const { const int r = N - CH * clane(); return r < 0 ? 0 : (r > CH ? CH : r); }
    // (counts of own stages that exist; the role-split mapping of an odd keep has SPL - 1 slots in use on role B, starting at slot 1)
    __device__ __forceinline__ int first_stage() const { return clane() * CH + wrole() * SPL; }
    __device__ __forceinline__ int nq_own() const { const int r = N - 1 - first_stage(), m_ = SPL - qoff(); return r < 0 ? 0 : (r > m_ ? m_ : r); }
    __device__ __forceinline__ int nst_own() const { const int r = N - first_stage(), m_ = SPL - qoff(); return r < 0 ? 0 : (r > m_ ? m_ : r); }
    // 9-element records (Ginv 0..5 | w 6..8, or a 3x3 matrix) are stored per lane as four 16-byte pairs + one single so
    // that the hot readers use ds_read_b128: element i of lane t of record `base`.
    __device__ __forceinline__ int idx9(int base, int t, int i) const { return i < 8 ? base + (((i >> 1) * L.TP + t) << 1) + (i & 1) : base + 8 * L.TP + t; }
    // The pairs are READ as 16-byte vectors and WRITTEN as scalars (FA(), PL()): the vector type carries may_alias.  With HIP's double2 (a struct, distinct
    // from `double` for type-based alias analysis) the compiler was free to move a pair load above an earlier scalar store to the same words — which it
    // did, depending on how a given instantiation inlined: the "miscompiled chunk recursion" of keep 3 (round 2: +10 .. 20 refinement iterations, 1e-2 off
    // on every path of one chunk shape, only in some builds) was this; -fno-strict-aliasing (csrc/Makefile) is the second line of defence.
    typedef double pair_t __attribute__((ext_vector_type(2), may_alias, aligned(16)));
    __device__ __forceinline__ void load9(int base, int t, double o[9]) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) { const pair_t v = *reinterpret_cast<const pair_t *>(S + base + ((k * L.TP + t) << 1)); o[2 * k] = v.x; o[2 * k + 1] = v.y; }
        o[8] = S[base + 8 * L.TP + t];
    }
    // the same record written as four 16-byte pairs + one single (round 5: a scalar 8-byte access of this layout has a lane stride of 16 bytes, a two-way bank conflict; the
    // factorisation — once per Newton step — used to write and re-read its records element by element: 14.7 % of the Newton kernel's busy cycles were LDS bank conflicts)
    __device__ __forceinline__ void store9(int base, int t, const double v[9]) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) { pair_t p_; p_.x = v[2 * k]; p_.y = v[2 * k + 1]; *reinterpret_cast<pair_t *>(S + base + ((k * L.TP + t) << 1)) = p_; }
        S[base + 8 * L.TP + t] = v[8];
    }
    __device__ __forceinline__ double &FA(int q, int i) const { return S[idx9(L.fac + cs(q) * 9 * L.TP, clane(), i)]; }  // own stage q
    __device__ __forceinline__ double &FAt(int t, int q, int i) const { return S[idx9(L.fac + q * 9 * L.TP, t, i)]; }
    __device__ __forceinline__ double &FU(int i) const { return S[L.facu + i * L.TP + clane()]; }                      // own control (one group per lane)
    __device__ __forceinline__ double &FUg(int g, int i) const { return S[L.facu + (g * 4 + i) * L.TP + clane()]; }    // control of own group g
    __device__ __forceinline__ double &FUc(int c, int i) const { return S[L.facu + ((c % NG) * 4 + i) * L.TP + c / NG]; }  // control c of the path
    __device__ __forceinline__ double &PL(int lvl, int t, int i) const { return S[idx9(L.phi + lvl * 9 * L.TP, t, i)]; }

    // DPP lane moves of a double (two 32-bit halves).  Lanes without a source keep `keep`.
    template <int CTRL> static __device__ __forceinline__ double dpp_mov(double v, double keep) {
        const int lo = __builtin_amdgcn_update_dpp(__double2loint(keep), __double2loint(v), CTRL, 0xf, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(__double2hiint(keep), __double2hiint(v), CTRL, 0xf, 0xf, false);
        return __hiloint2double(hi, lo);
    }
    // same, lanes without a source read 0 (bound_ctrl): no `old` operand to initialise
    template <int CTRL> static __device__ __forceinline__ double dpp_mov0(double v) {
        const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
        const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
        return __hiloint2double(hi, lo);
    }
    static constexpr int kDppRowShl = 0x100, kDppRowShr = 0x110, kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138;
    // neighbour exchange: out = v of lane tid + delta (own value at the ends).  One wave and |delta| == 1: a DPP wave shift (VALU latency);
    // one wave otherwise: LDS crossbar permute; several waves: the wave shift, and the lane at a wave boundary through mailbox `buf` (0 / 1) of L.ex with ONE barrier —
    // callers alternate buf, so that a call never overwrites what a slower wave still reads from the call before.
    template <int CNT> __device__ __forceinline__ void xchg(const double *v, int delta, double *out, int buf) const {
        if constexpr (NT == 64) {
            if (__builtin_constant_p(delta) && (delta == 1 || delta == -1)) {
#pragma unroll
                for (int k = 0; k < CNT; ++k) out[k] = delta == 1 ? dpp_mov<kDppWaveShl1>(v[k], v[k]) : dpp_mov<kDppWaveShr1>(v[k], v[k]);
                return;
            }
        }
        if constexpr (NT == 64) {  // one wave: LDS crossbar permute, no memory traffic, no barrier
            const int p = tid + delta;
            const int src = (p >= 0 && p < 64 ? p : tid) << 2;
#pragma unroll
            for (int k = 0; k < CNT; ++k) {
                const int lo = __builtin_amdgcn_ds_bpermute(src, __double2loint(v[k]));
                const int hi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(v[k]));
                out[k] = __hiloint2double(hi, lo);
            }
            return;
        }
        // several waves (|delta| == 1 always): DPP wave shift inside each wave, the lane at the wave boundary through a mailbox (one barrier)
        constexpr int NWV = NT / 64;
        double *e = S + L.ex + buf * 4 * NWV;
        const int wv = tid >> 6, lw_ = tid & 63;
        if (lw_ == (delta < 0 ? 63 : 0)) {
#pragma unroll
            for (int k = 0; k < CNT; ++k) e[k * NWV + wv] = v[k];
        }
        __syncthreads();
        const bool edge = delta < 0 ? (lw_ == 0 && wv > 0) : (lw_ == 63 && wv + 1 < NWV);
        const int src = delta < 0 ? (wv > 0 ? wv - 1 : 0) : (wv + 1 < NWV ? wv + 1 : wv);
#pragma unroll
        for (int k = 0; k < CNT; ++k) {
            const double m_ = e[k * NWV + src];
            const double d_ = delta < 0 ? dpp_mov<kDppWaveShr1>(v[k], v[k]) : dpp_mov<kDppWaveShl1>(v[k], v[k]);
            out[k] = edge ? m_ : d_;
        }
    }

    // value(s) held by lane `src` (0..63) of the caller's own wave
    template <int CNT> __device__ __forceinline__ void wshfl(const double *v, int src, double *out) const {
        const int a = (src & 63) << 2;
#pragma unroll
        for (int k = 0; k < CNT; ++k) {
            const int lo = __builtin_amdgcn_ds_bpermute(a, __double2loint(v[k]));
            const int hi = __builtin_amdgcn_ds_bpermute(a, __double2hiint(v[k]));
            out[k] = __hiloint2double(hi, lo);
        }
    }
    static constexpr bool SEG = TWO && NT > 64 && NW == 1;  // segmented scan (multi-wave blocks): one barrier per scan instead of one per level
    __device__ __forceinline__ double &RS(int lvl, int g, int i) const { return S[L.rseg + (lvl * L.nsm + g) * 9 + i]; }

    // y += / = E_q z  helpers on the regenerated coupling block of the transition out of own stage q
    __device__ __forceinline__ void apply_E(const Dyn<F> &d, const double re[T::NDYN], bool has_rc, const double z[3], double out[3]) const {
        // out = -E z  (so that y_next = b + out):  (E z)[tau_r] = -re_r f_r.z
        out[0] = out[1] = out[2] = 0;
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) out[dyn_tau<F>(r)] += re[r] * (d.f[r][0] * z[0] + d.f[r][1] * z[1] + d.f[r][2] * z[2]);
        if constexpr (F == F_K) { if (has_rc) out[2] += P.w_cr * z[2]; }
    }
    __device__ __forceinline__ void apply_Et(const Dyn<F> &d, const double re[T::NDYN], bool has_rc, const double x[3], double out[3]) const {
        // out = E' x :  (E'x)[c] = -sum_r re_r f_r[c] x[tau_r]
        out[0] = out[1] = out[2] = 0;
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) {
            const double s = -re[r] * x[dyn_tau<F>(r)];
            out[0] += s * d.f[r][0]; out[1] += s * d.f[r][1]; out[2] += s * d.f[r][2];
        }
        if constexpr (F == F_K) { if (has_rc) out[2] -= P.w_cr * x[2]; }
    }
    __device__ __forceinline__ void mul_Gr(const double g[9], const double y[3], double z[3]) const {  // z = Ginv y
        z[0] = g[0] * y[0] + g[1] * y[1] + g[2] * y[2];
        z[1] = g[1] * y[0] + g[3] * y[1] + g[4] * y[2];
        z[2] = g[2] * y[0] + g[4] * y[1] + g[5] * y[2];
    }
    __device__ __forceinline__ void mul_G(int q, const double y[3], double z[3]) const {  // own stage q
        double g[9];
        load9(L.fac + cs(q) * 9 * L.TP, clane(), g);
        mul_Gr(g, y, z);
    }

// ==================== [two_factor] ====================
// members of Fast, part 3: factorisation step A of the two-level mapping, and the coupling block of one transition.  TWO only, every NWX.
//   factor_blocks_two<UNI, POL>   every lane condenses the rows of its own stages (slacks eliminated) into (H_q | ws_q) and its controls' pivots: what the pivot
//                                 chain ([two_pivot_scan], [two_factor_chain]) starts from.  POL: the rows of the polish's active set (PolWrap)
//   transition (Tr)               E and the control column of the transition out of own stage q, regenerated from the lane's (k, ds, trig): used by both pivot scans
//   LDS     writes fac (one 9-record per own stage), facu element 0 (the pivot before elimination), rrb (lane 0: the uniform row steps of this factorisation; UNI: the
//           slack-elimination data too); role-split: the other role's share of the pivot goes through hx1 (= ex), one barrier
//   lanes   reads the inputs, cls / clse / clsc (general variant) or pat_* (UNI), pc* (POL); writes hi, hv (general variant only), hiu, hus
//   called  admm_loop and refine_phase_newton ([loops]) and polish_kernel, always followed by factor_chain_two
    template <bool UNI = false, bool POL = false> __device__ __forceinline__ void factor_blocks_two(LS &st, double rho) const {
        const double rho_eq = eq_step(rho);
        double huu_dyn[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) huu_dyn[g] = 0;
        double re[T::NDYN];
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) re[r] = eq_row_step(rho_eq, r);
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            HessFn h(rho, rho_eq, Wloc(j), Eloc(j), cls_of<UNI>(st, q));
            if constexpr (POL) { PolWrap<HessFn> w{h, st.pc[q]}; local_rows<F>(si, P, w); } else local_rows<F>(si, P, h);
            if (T::NEND && si.last) {
                h.W = Wend(); h.E = Eend(); h.cls = st.clse;
                if constexpr (POL) { PolWrap<HessFn> w{h, st.pce}; end_rows<F>(si, P, w); } else end_rows<F>(si, P, h);
            }
            h.H[HessFn::idx(0, 0)] += sig(0, j) + p_diag_node<F>(0, j, N, P);
            h.H[HessFn::idx(1, 1)] += sig(1, j) + p_diag_node<F>(1, j, N, P);
            h.H[HessFn::idx(2, 2)] += sig(2, j) + p_diag_node<F>(2, j, N, P);
            h.H[HessFn::idx(3, 3)] += sig(3, j) + P.w_s1;
            h.H[HessFn::idx(4, 4)] += sig(4, j) + P.w_s2;
            double G[6] = {h.H[HessFn::idx(0, 0)], h.H[HessFn::idx(0, 1)], h.H[HessFn::idx(0, 2)],
                           h.H[HessFn::idx(1, 1)], h.H[HessFn::idx(1, 2)], h.H[HessFn::idx(2, 2)]};
#pragma unroll
            for (int s = 0; s < T::NS; ++s) {
                const double hi = 1.0 / h.H[HessFn::idx(3 + s, 3 + s)];
                const double hv[3] = {h.H[HessFn::idx(0, 3 + s)], h.H[HessFn::idx(1, 3 + s)], h.H[HessFn::idx(2, 3 + s)]};
                if constexpr (UNI) {
                    if (q == 0 && tid == 0) {
                        S[L.rrb + 16 + s] = hi; S[L.rrb + 18 + 3 * s] = hv[0]; S[L.rrb + 18 + 3 * s + 1] = hv[1]; S[L.rrb + 18 + 3 * s + 2] = hv[2];
                        if constexpr (F == F_KPC) {
                            if (s == 1) {  // both copies of 1 / H_ss of the curvature slack: Sk box row as an inequality [17] / as an equality [25]
                                const double hss = h.H[HessFn::idx(3 + s, 3 + s)], w3 = Wloc()[3];
                                const bool eq0 = kpc_c3(st, q) != 0u;
                                const double h_in = eq0 ? hss - w3 * rho_eq + w3 * rho : hss, h_eq = eq0 ? hss : hss - w3 * rho + w3 * rho_eq;
                                S[L.rrb + 17] = 1.0 / h_in; S[L.rrb + 25] = 1.0 / h_eq;
                            }
                        }
                    }
                } else { st.hi[q][s] = hi; st.hv[q][s][0] = hv[0]; st.hv[q][s][1] = hv[1]; st.hv[q][s][2] = hv[2]; }
                G[0] -= hv[0] * hv[0] * hi; G[1] -= hv[0] * hv[1] * hi; G[2] -= hv[0] * hv[2] * hi;
                G[3] -= hv[1] * hv[1] * hi; G[4] -= hv[1] * hv[2] * hi; G[5] -= hv[2] * hv[2] * hi;
            }
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) {
                const int t = dyn_tau<F>(r);
                G[t == 0 ? 0 : (t == 1 ? 3 : 5)] += re[r];
            }
            double ws[3] = {0, 0, 0};
            if (j < N - 1) {
                const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    G[0] += re[r] * d.f[r][0] * d.f[r][0]; G[1] += re[r] * d.f[r][0] * d.f[r][1]; G[2] += re[r] * d.f[r][0] * d.f[r][2];
                    G[3] += re[r] * d.f[r][1] * d.f[r][1]; G[4] += re[r] * d.f[r][1] * d.f[r][2]; G[5] += re[r] * d.f[r][2] * d.f[r][2];
#pragma unroll
                    for (int c = 0; c < 3; ++c) ws[c] += re[r] * d.beta[r] * d.f[r][c];
                    huu_dyn[gOut(q)] += re[r] * d.beta[r] * d.beta[r];
                }
            }
            { const double rec[9] = {G[0], G[1], G[2], G[3], G[4], G[5], ws[0], ws[1], ws[2]}; store9(L.fac + cs(q) * 9 * L.TP, clane(), rec); }
        }
        if constexpr (NW == 2) {  // the control's pivot sums the beta^2 terms of all transitions of the group: the other role's go through LDS
            if (wrole() != own_role() && clane() < L.TP) S[L.hx1 + clane()] = huu_dyn[0];
            __syncthreads();
            if (wrole() == own_role() && clane() < L.TP) huu_dyn[0] += S[L.hx1 + clane()];
        }
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (has_ctl(g)) {
                    HessFn h(rho, rho_eq, Wctl(), Ectl(), st.clsc);
                    if constexpr (POL) { PolWrap<HessFn> w{h, st.pcc}; ctl_rows<F>(st.mkp, w); } else ctl_rows<F>(st.mkp, h);
                    double huu = h.H[HessFn::idx(2, 2)] + sig(5) + P.w_u;
                    if constexpr (T::HAS_SU) {
                        const double hi = 1.0 / (h.H[HessFn::idx(3, 3)] + sig(6) + P.w_su);
                        st.hiu = hi; st.hus = h.H[HessFn::idx(2, 3)];
                        huu -= st.hus * st.hus * hi;
                    }
                    FUg(g, 0) = huu + huu_dyn[g];
                }
            }
        }
        if (tid == 0) {  // uniform per-row steps for the specialised hot passes (valid when classify() found uniform classes)
#pragma unroll
            for (int r = 0; r < T::NLOC; ++r) S[L.rrb + r] = class_rho(pat_loc, r, Wloc()[r], rho, rho_eq);
#pragma unroll
            for (int r = 0; r < T::NCTL; ++r) S[L.rrb + 9 + r] = class_rho(pat_ctl, r, Wctl()[r], rho, rho_eq);
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) S[L.rrb + 12 + r] = rho_eq * Wdyn()[r];
            if constexpr (F == F_KPC) S[L.rrb + 15] = Wloc()[3] * rho_eq;               // Sk box row where it is an equality (S[rrb + 3]: where it is not)
            if constexpr (F == F_K) {
                S[L.rrb + 15] = class_rho(pat_loc, 2, Wloc(0)[2], rho, rho_eq);       // steering box row of the stages 0 and N-2 (own Ruiz factor)
                S[L.rrb + 24] = class_rho(pat_last, 0, Wloc()[0], rho, rho_eq);       // e_phi row of the final stage (end-heading window)
            }
        }
        __syncthreads();
    }
    struct Tr { double E[9], wn0[3]; };  // transition j -> j + 1:  E = M[x_{j+1}, x_j],  wn0 = M[x_{j+1}, u] (the part this transition contributes)
    __device__ __forceinline__ Tr transition(const LS &st, int q, const double re[T::NDYN]) const {
        const int qn = q + 1 < SPL ? q + 1 : q;
        const double kq = q + 1 < SPL ? st.kin[qn] : st.kout, dsq = q + 1 < SPL ? st.dsin[qn] : st.dsout;
        const double trq[2] = {q + 1 < SPL ? st.trin[F == F_K ? qn : 0][0] : st.trout[0], q + 1 < SPL ? st.trin[F == F_K ? qn : 0][1] : st.trout[1]};
        const Dyn<F> d = make_dyn_tr<F>(kq, dsq, trq, P);
        Tr tr;
#pragma unroll
        for (int i = 0; i < 9; ++i) tr.E[i] = 0;
        tr.wn0[0] = tr.wn0[1] = tr.wn0[2] = 0;
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) {
            const int tt = dyn_tau<F>(r);
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) tr.E[tt * 3 + cc] += -re[r] * d.f[r][cc];
            tr.wn0[tt] += -re[r] * d.beta[r];
        }
        if constexpr (F == F_K) { if (stage(q) + 1 <= N - 2) tr.E[8] += -P.w_cr; }
        return tr;
    }

// ==================== [two_pivot_scan] ====================
// members of Fast, part 4: factorisation step B of the two-level mapping as a scan over chunks.  TWO only.  3 x 3 helpers (sym_full, mul33,
// mul33t, sym_sub_abt), the chunk element and its composition (ChunkEl, combine_el), and the two scans: factor_pivots_scan (NW 1: NWX 1, 4, 5) and
// factor_pivots_scan2 (NW 2: NWX 2, 3; ChunkRun is its hand-over between the roles).  TWINS: the two functions are the same four steps written twice — scan2 splits
// steps (1) and (3) over the two roles of a chunk; a change to the arithmetic of one belongs in the other.
//   LDS     reads fac / facu as factor_blocks_two left them; double-buffers the scan elements (2 x 21 x TP doubles; scan2: its hand-over in the second buffer) in phi,
//           whose tables are dead here and rebuilt by factor_chain_two right after; commits fac / facu (Ginv | w, 1 / p_u | l_x) only when the cross-check passed;
//           the vote goes through block_any (ex, NT > 64)
//   lanes   reads the transition inputs (kin, dsin, kout, dsout, trin, trout) through transition(); writes nothing
//   called  factor_chain_two ([two_factor_chain]) only; false sends it down the sequential recursion
    // ---------------------------------------------------------------------------------------------------------------------------------
    // The pivot chain of the block LDL' as a SCAN over chunks (one lane per chunk, NW == 1).
    //
    // The sequential recursion  G_{j+1} = H_{j+1} - E_j G_j^-1 E_j' (- the rank-one term of the group's control)  walks N - 1 dependent 3 x 3 steps
    // (215 k cycles at N = 200: 14 iterations' worth, paid at every refactorisation).  It is a linear-fractional map of the pivot, and such maps
    // compose: for chunk t, eliminating its interior stages and its control from the chunk's own terms, with its first stage x_a and the first stage of
    // the next chunk x_b RETAINED, leaves a quadratic [[A, B], [B', D]] on (x_a, x_b); the correction the chunk passes on is
    //       Delta_{t+1} = D - B' (A + Delta_t)^-1 B                       (G of chunk t's first stage = H + Delta_t),
    // and two consecutive chunks combine by eliminating the shared stage:  K = (A2 + D1)^-1 (an SPD pivot: a Schur complement of a principal
    // submatrix),  A12 = A1 - B1 K B1',  B12 = -B1 K B2,  D12 = D2 - B2' K B2.  So: (1) every lane reduces its own chunk (SPL - 1 eliminations + the
    // control), (2) Kogge-Stone over the chunks (log2 levels, 21 doubles per element, through LDS), (3) every lane runs the ordinary recursion over its
    // own SPL stages from G = H + Delta_t and stores exactly what the sequential loop stored (Ginv_j | w_j per stage, 1 / p_u | l_x per control).
    // Same factorisation in a different elimination order.  MEASURED (config 3): 31 k cycles instead of 215 k.  What the scan hands chunk t and what chunk
    // t - 1's own recursion passes on are the same quantity computed two ways; they agree to rounding (2e-15 relative), i.e. the stored factors are those of M
    // plus a symmetric block-diagonal perturbation of that size, which moves the QP's solution by ~3 x as much — harmless.  Step (4) checks exactly that
    // agreement at every factorisation and falls back to the sequential recursion when it fails (never observed to trigger: tools/scan_fallbacks.py).  The check
    // is not decoration: while this function was developed, two builds of it (3-stage chunks, then 5-stage chunks after a restructuring) produced factors that
    // cost the refinement 10 - 20 extra iterations per path and moved its result by 1e-2, on every path of the shape and only in builds that did not consume
    // the chunk's outgoing correction — a code-generation problem, not rounding (the same source with the value consumed matches the oracle to 1e-11, and
    // so does every variant since the check consumes it).  tests/test_refine.py::test_device_refine_every_keep_value_matches_oracle pins every chunk shape.
    // ---------------------------------------------------------------------------------------------------------------------------------
    static __device__ __forceinline__ void sym_full(const double s[6], double f[9]) {
        f[0] = s[0]; f[1] = s[1]; f[2] = s[2]; f[3] = s[1]; f[4] = s[3]; f[5] = s[4]; f[6] = s[2]; f[7] = s[4]; f[8] = s[5];
    }
    static __device__ __forceinline__ void mul33(const double a[9], const double b[9], double c[9]) {  // c = a b
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[3 * r + k] = a[3 * r] * b[k] + a[3 * r + 1] * b[3 + k] + a[3 * r + 2] * b[6 + k];
    }
    static __device__ __forceinline__ void mul33t(const double a[9], const double b[9], double c[9]) {  // c = a b'
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[3 * r + k] = a[3 * r] * b[3 * k] + a[3 * r + 1] * b[3 * k + 1] + a[3 * r + 2] * b[3 * k + 2];
    }
    // s -= a b' (the product is symmetric by construction; packed [00 01 02 11 12 22])
    static __device__ __forceinline__ void sym_sub_abt(double s[6], const double a[9], const double b[9]) {
        s[0] -= a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
        s[1] -= a[0] * b[3] + a[1] * b[4] + a[2] * b[5];
        s[2] -= a[0] * b[6] + a[1] * b[7] + a[2] * b[8];
        s[3] -= a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
        s[4] -= a[3] * b[6] + a[4] * b[7] + a[5] * b[8];
        s[5] -= a[6] * b[6] + a[7] * b[7] + a[8] * b[8];
    }
    struct ChunkEl { double A[6], B[9], D[6]; };
    // first o second (first = the chunks before): eliminates the stage they share
    static __device__ __forceinline__ ChunkEl combine_el(const ChunkEl &a, const ChunkEl &b) {
        double ks[6], Ki[6], K[9], X[9], Y[9];
#pragma unroll
        for (int i = 0; i < 6; ++i) ks[i] = b.A[i] + a.D[i];
        inv3_sym(ks, Ki);
        sym_full(Ki, K);
        ChunkEl o;
        mul33(a.B, K, X);  // B1 K
        mul33(K, b.B, Y);  // K B2
#pragma unroll
        for (int i = 0; i < 6; ++i) { o.A[i] = a.A[i]; o.D[i] = b.D[i]; }
        sym_sub_abt(o.A, X, a.B);  // A1 - B1 K B1'
        double bt[9] = {b.B[0], b.B[3], b.B[6], b.B[1], b.B[4], b.B[7], b.B[2], b.B[5], b.B[8]}, yt[9] = {Y[0], Y[3], Y[6], Y[1], Y[4], Y[7], Y[2], Y[5], Y[8]};
        sym_sub_abt(o.D, bt, yt);  // D2 - B2' K B2
        mul33(a.B, Y, o.B);
#pragma unroll
        for (int i = 0; i < 9; ++i) o.B[i] = -o.B[i];
        return o;
    }
    static constexpr double kScanTol = 1e-11;  // step (4): largest relative disagreement between the scan's and the recursion's correction that still commits the scan
    __device__ __forceinline__ bool factor_pivots_scan(LS &st, const double re[T::NDYN]) const {
        static_assert(NW == 1, "one lane per chunk");
        const int nst = nst_own(), nq = nq_own();  // own stages / own outgoing transitions
        const bool full = nq == SPL;               // the chunk has a successor: its element is part of somebody's prefix
        // (round 5) the blocks factor_blocks_two left (H_q, ws_q) are NOT held in registers across the scan: every use reads them from LDS, and the results of step (3) stay in
        // registers until the cross-check of step (4) has passed — so a failed check leaves LDS exactly as it was (no restore) and the scan's peak register demand drops
        // by 36 doubles (the Newton kernels refactorise at every step: this is where they spilled)
        auto ldrec = [&](int q, double r_[9]) {  // (H_q | ws_q) of own stage q as one 16-byte-pair record read; a stage that does not exist: identity / zero
            load9(L.fac + cs(q) * 9 * L.TP, clane(), r_);
            if (!(q < nst)) { r_[0] = r_[3] = r_[5] = 1.0; r_[1] = r_[2] = r_[4] = r_[6] = r_[7] = r_[8] = 0.0; }
        };
        double pu0[NG];  // the controls' pivots as factor_blocks_two left them (multi-group mapping: G controls per lane, each eliminated after its group's last transition)
#pragma unroll
        for (int g = 0; g < NG; ++g) pu0[g] = T::HAS_U ? (has_ctl(g) ? FUg(g, 0) : 1.0) : 1.0;
        // ---- (1) the chunk's element: x_0 retained, stages 1 .. SPL-1 and the control(s) eliminated ----
        ChunkEl el;
#pragma unroll
        for (int i = 0; i < 6; ++i) { el.A[i] = (i == 0 || i == 3 || i == 5) ? 1.0 : 0.0; el.D[i] = 0.0; }
#pragma unroll
        for (int i = 0; i < 9; ++i) el.B[i] = 0.0;
        if (full) {
            double A[6], Bf[9], bu[3], G[6], w[3], pu = pu0[0];
            // elimination of the current control from the retained pair (x_0, the stage the run has reached): its couplings b_u, w and its pivot p_u
            auto ctl_elim = [&]() {
                const double pi = 1.0 / pu;
                const double lb[3] = {bu[0] * pi, bu[1] * pi, bu[2] * pi};
                A[0] -= lb[0] * bu[0]; A[1] -= lb[0] * bu[1]; A[2] -= lb[0] * bu[2]; A[3] -= lb[1] * bu[1]; A[4] -= lb[1] * bu[2]; A[5] -= lb[2] * bu[2];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) Bf[3 * r + k] -= lb[r] * w[k];
                const double lw[3] = {w[0] * pi, w[1] * pi, w[2] * pi};
                G[0] -= lw[0] * w[0]; G[1] -= lw[0] * w[1]; G[2] -= lw[0] * w[2]; G[3] -= lw[1] * w[1]; G[4] -= lw[1] * w[2]; G[5] -= lw[2] * w[2];
            };
            {
                double r0[9], r1[9];
                ldrec(0, r0);
                ldrec(SPL > 1 ? 1 : 0, r1);
#pragma unroll
                for (int i = 0; i < 6; ++i) A[i] = r0[i];
                const Tr t0 = transition(st, 0, re);
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) Bf[3 * r + k] = t0.E[3 * k + r];  // M[x_0, x_1] = E_0'
#pragma unroll
                for (int i = 0; i < 3; ++i) { bu[i] = r0[6 + i]; w[i] = t0.wn0[i] + ((SPL > 1 && gOut(1) == 0) ? r1[6 + i] : 0.0); }
#pragma unroll
                for (int i = 0; i < 6; ++i) G[i] = SPL > 1 ? r1[i] : 0.0;
                if constexpr (NG > 1) {
                    if (gOut(1) != 0) {  // (groups of one stage) the first group ends with transition 0: its control goes now, stage 1 starts the next one
                        ctl_elim();
#pragma unroll
                        for (int i = 0; i < 3; ++i) { bu[i] = 0.0; w[i] = r1[6 + i]; }
                        pu = pu0[gOut(1) < NG ? gOut(1) : 0];
                    }
                }
            }
#pragma unroll
            for (int q = 1; q < SPL; ++q) {  // eliminate x_q
                const Tr tq = transition(st, q, re);
                double Gi[6], Gf[9], Tm[9], Ln[9], Bn[9];
                inv3_sym(G, Gi);
                sym_full(Gi, Gf);
                mul33(Bf, Gf, Tm);          // T = B_f G^-1
                sym_sub_abt(A, Tm, Bf);     // A -= T B_f'
                mul33t(Tm, tq.E, Bn);       // T E'
                mul33(tq.E, Gf, Ln);        // L = E G^-1
                double Gn[6], rn_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                if (q + 1 < SPL) ldrec(q + 1 < SPL ? q + 1 : q, rn_);
#pragma unroll
                for (int i = 0; i < 6; ++i) Gn[i] = rn_[i];
                sym_sub_abt(Gn, Ln, tq.E);  // H_next - L E'
                if constexpr (T::HAS_U) {
                    const double lu[3] = {Gf[0] * w[0] + Gf[1] * w[1] + Gf[2] * w[2], Gf[3] * w[0] + Gf[4] * w[1] + Gf[5] * w[2], Gf[6] * w[0] + Gf[7] * w[1] + Gf[8] * w[2]};
#pragma unroll
                    for (int r = 0; r < 3; ++r) bu[r] -= Bf[3 * r] * lu[0] + Bf[3 * r + 1] * lu[1] + Bf[3 * r + 2] * lu[2];  // T w = B_f (G^-1 w)
                    pu -= lu[0] * w[0] + lu[1] * w[1] + lu[2] * w[2];
// the next stage's own coupling belongs to the current control only while it is in the same group
                    const bool same_grp = q + 1 < SPL && gOut(q + 1 < SPL ? q + 1 : q) == gOut(q);
#pragma unroll
                    for (int r = 0; r < 3; ++r)
                        w[r] = tq.wn0[r] - (tq.E[3 * r] * lu[0] + tq.E[3 * r + 1] * lu[1] + tq.E[3 * r + 2] * lu[2]) + (same_grp ? rn_[6 + r] : 0.0);
                }
#pragma unroll
                for (int i = 0; i < 9; ++i) Bf[i] = -Bn[i];
#pragma unroll
                for (int i = 0; i < 6; ++i) G[i] = Gn[i];
                if constexpr (NG > 1) {
                    if (q + 1 < SPL && gOut(q + 1 < SPL ? q + 1 : q) != gOut(q)) {  // group boundary inside the lane: this control goes, the next stage starts the next one
                        ctl_elim();
#pragma unroll
                        for (int i = 0; i < 3; ++i) { bu[i] = 0.0; w[i] = rn_[6 + i]; }
                        pu = pu0[gOut(q + 1 < SPL ? q + 1 : q)];
                    }
                }
            }
            if constexpr (T::HAS_U) ctl_elim();  // the (last) control
#pragma unroll
            for (int i = 0; i < 6; ++i) { el.A[i] = A[i]; el.D[i] = G[i]; }
#pragma unroll
            for (int i = 0; i < 9; ++i) el.B[i] = Bf[i];
        }
        // ---- (2) inclusive Kogge-Stone over the chunks, double-buffered in the (idle) prefix-table region ----
        double *sb = S + L.phi;
        const int TPs = L.TP, t = clane() + (NT > 64 ? 0 : 0);
        const int tl = tid;  // NW == 1: chunk index == thread index
        (void)t;
        int cur = 0;
        auto put = [&](int buf, const ChunkEl &e) {
            if (tl < TPs) {
#pragma unroll
                for (int i = 0; i < 6; ++i) { sb[(buf * 21 + i) * TPs + tl] = e.A[i]; sb[(buf * 21 + 15 + i) * TPs + tl] = e.D[i]; }
#pragma unroll
                for (int i = 0; i < 9; ++i) sb[(buf * 21 + 6 + i) * TPs + tl] = e.B[i];
            }
        };
        auto get = [&](int buf, int lane) {
            ChunkEl e;
#pragma unroll
            for (int i = 0; i < 6; ++i) { e.A[i] = sb[(buf * 21 + i) * TPs + lane]; e.D[i] = sb[(buf * 21 + 15 + i) * TPs + lane]; }
#pragma unroll
            for (int i = 0; i < 9; ++i) e.B[i] = sb[(buf * 21 + 6 + i) * TPs + lane];
            return e;
        };
        __syncthreads();  // (the region held the previous factorisation's tables: every reader is done)
        put(cur, el);
        __syncthreads();
        const int nch = (N + SPL - 1) / SPL;  // chunks that own a stage
        for (int d = 1; d < nch; d <<= 1) {
            if (tl >= d && tl < TPs) { const ChunkEl p = get(cur, tl - d); el = combine_el(p, el); }
            put(cur ^ 1, el);
            __syncthreads();
            cur ^= 1;
        }
        // ---- (3) own stages from G = H + Delta_t: the ordinary recursion, lane-parallel ----
        double Rq[SPL][9], ru[NG][4];  // step (3)'s results: (Ginv | w) per own stage, (1 / p_u | l_x) per control — committed to LDS after the cross-check
        bool ctl_done[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) { ru[g][0] = ru[g][1] = ru[g][2] = ru[g][3] = 0; ctl_done[g] = false; }
        auto local_pass = [&](const double din[6], double gout[6]) {
            double G[6], w[3], pu = pu0[0];
            {
                double r0[9];
                ldrec(0, r0);
#pragma unroll
                for (int i = 0; i < 6; ++i) G[i] = r0[i] + din[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) w[i] = r0[6 + i];
            }
#pragma unroll
            for (int q = 0; q < SPL; ++q) {
                if (q < nst) {
                    double Gi[6];
                    inv3_sym(G, Gi);
#pragma unroll
                    for (int i = 0; i < 6; ++i) Rq[q][i] = Gi[i];
                    Rq[q][6] = Rq[q][7] = Rq[q][8] = 0;
                    if (q < nq) {  // the transition out of own stage q (the final stage of the path has none: its pivot inverse only)
                        Rq[q][6] = w[0]; Rq[q][7] = w[1]; Rq[q][8] = w[2];
                        const Tr tq = transition(st, q, re);
                        double Gf[9], Ln[9];
                        sym_full(Gi, Gf);
                        mul33(tq.E, Gf, Ln);
                        double Gn[6], rn_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                        if (q + 1 < SPL) ldrec(q + 1 < SPL ? q + 1 : q, rn_);
#pragma unroll
                        for (int i = 0; i < 6; ++i) Gn[i] = rn_[i];
                        sym_sub_abt(Gn, Ln, tq.E);
                        if constexpr (T::HAS_U) {
                            const double lu[3] = {Gf[0] * w[0] + Gf[1] * w[1] + Gf[2] * w[2], Gf[3] * w[0] + Gf[4] * w[1] + Gf[5] * w[2], Gf[6] * w[0] + Gf[7] * w[1] + Gf[8] * w[2]};
                            double wn[3];
#pragma unroll
                            for (int r = 0; r < 3; ++r) wn[r] = tq.wn0[r] - (tq.E[3 * r] * lu[0] + tq.E[3 * r + 1] * lu[1] + tq.E[3 * r + 2] * lu[2]);
                            pu -= lu[0] * w[0] + lu[1] * w[1] + lu[2] * w[2];
                            if (grp_end(q, nq)) {  // last transition of the group: the control
                                const double pi = 1.0 / pu;
                                const double lx[3] = {wn[0] * pi, wn[1] * pi, wn[2] * pi};
                                Gn[0] -= lx[0] * wn[0]; Gn[1] -= lx[0] * wn[1]; Gn[2] -= lx[0] * wn[2]; Gn[3] -= lx[1] * wn[1]; Gn[4] -= lx[1] * wn[2]; Gn[5] -= lx[2] * wn[2];
                                ru[gOut(q)][0] = pi; ru[gOut(q)][1] = lx[0]; ru[gOut(q)][2] = lx[1]; ru[gOut(q)][3] = lx[2]; ctl_done[gOut(q)] = true;
                                if constexpr (NG > 1) {  // the next stage (on this lane) starts the next group
#pragma unroll
                                    for (int r = 0; r < 3; ++r) w[r] = rn_[6 + r];
                                    pu = pu0[q + 1 < SPL ? gOut(q + 1 < SPL ? q + 1 : q) : 0];
                                }
                            } else {
#pragma unroll
                                for (int r = 0; r < 3; ++r) w[r] = wn[r] + rn_[6 + r];
                            }
                        }
#pragma unroll
                        for (int i = 0; i < 6; ++i) G[i] = Gn[i];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) gout[i] = G[i];  // a full chunk: the correction its OWN recursion passes on (cross-checked below against the scan's)
        };
        double din[6] = {0, 0, 0, 0, 0, 0}, gout[6] = {0, 0, 0, 0, 0, 0};
        if (nst > 0) {
            if (tl > 0) {
                const ChunkEl p = get(cur, tl - 1);  // the chunks before this one
                double Ai[6], Af[9], X[9];
                inv3_sym(p.A, Ai);
                sym_full(Ai, Af);
                const double bt[9] = {p.B[0], p.B[3], p.B[6], p.B[1], p.B[4], p.B[7], p.B[2], p.B[5], p.B[8]};
                mul33(bt, Af, X);  // B' A^-1
#pragma unroll
                for (int i = 0; i < 6; ++i) din[i] = p.D[i];
                sym_sub_abt(din, X, bt);  // D - B' A^-1 B
            }
            local_pass(din, gout);
        }
        // ---- (4) cross-check.  What chunk t took from the scan and what chunk t - 1's own recursion passes on are the same quantity computed in two
        //      elimination orders: they must agree to rounding (measured 2e-15 relative).  The stored factors are then those of M plus a symmetric
        //      block-diagonal perturbation of that size — harmless (the QP's solution moves by ~3 x the perturbation).  Anything larger means this
        //      factorisation cannot be trusted (an ill-conditioned interface block, or a code-generation problem: one build of this very function for
        //      3-stage chunks produced factors that cost the refinement 10 - 20 extra iterations): the sequential recursion then redoes it from the
        //      restored blocks.  Returns false in that case. ----
        __syncthreads();
        if (tl < TPs) {
#pragma unroll
            for (int i = 0; i < 6; ++i) sb[i * TPs + tl] = gout[i];
        }
        __syncthreads();
        bool bad = false;
        if (nst > 0 && tl > 0) {
            double wd = 0, wr = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) { wd = fmax(wd, fabs(sb[i * TPs + tl - 1] - din[i])); wr = fmax(wr, fabs(din[i])); }
            bad = !(wd <= kScanTol * wr) || nonfinite_bits(wd) != 0;
            if (in.dbg_cycles != nullptr && wr > 0) atomicMax(reinterpret_cast<unsigned long long *>(in.dbg_cycles + (size_t)b * 16 + 15), (unsigned long long)__double_as_longlong(wd / wr));  // dev: worst relative disagreement seen
        }
        const bool any_bad = block_any(bad);
        if (in.dbg_cycles != nullptr && tid == 0) { long long *d = in.dbg_cycles + (size_t)b * 16; d[13] += 1; d[14] += any_bad ? 1 : 0; }  // dev: factorisations / fallbacks of this path
        if (!any_bad) {  // commit (a failed check leaves the blocks of factor_blocks_two in LDS untouched: the sequential recursion starts from them)
#pragma unroll
            for (int q = 0; q < SPL; ++q) {
                if (q < nst) store9(L.fac + cs(q) * 9 * L.TP, clane(), Rq[q]);  // (a stage without an outgoing transition: its w slots are zero, as factor_blocks_two left them)
            }
            if constexpr (T::HAS_U) {
#pragma unroll
                for (int g = 0; g < NG; ++g)
                    if (ctl_done[g]) { FUg(g, 0) = ru[g][0]; FUg(g, 1) = ru[g][1]; FUg(g, 2) = ru[g][2]; FUg(g, 3) = ru[g][3]; }
            }
        }
        __syncthreads();
        return !any_bad;
    }

    // ---------------------------------------------------------------------------------------------------------------------------------
    // The same scan for the ROLE-SPLIT mapping (NW == 2): a chunk's interior elimination and its own recursion run on role A, then on role B, with what the
    // recursion carries handed over through LDS (step 1: A, B_f, b_u, G, w, p_u = 28 numbers; step 3: G, w, p_u = 10); the Kogge-Stone scan over the chunk
    // elements runs on the role-B lanes.  Same arithmetic per stage as factor_pivots_scan, same cross-check, same fall-back.
    // ---------------------------------------------------------------------------------------------------------------------------------
    struct ChunkRun { double A[6], Bf[9], bu[3], G[6], w[3], pu; };
    __device__ __forceinline__ bool factor_pivots_scan2(LS &st, const double re[T::NDYN]) const {
        static_assert(NW == 2 || NW == 1, "role-split mapping");
        const int role = wrole(), tl = clane(), TPs = L.TP, off = qoff();
        const int nqc = nq_chunk(), nstc = nst_chunk();
        const bool fullc = nqc == CH;  // the chunk has a successor: its element is part of somebody's prefix
        const int c0 = role * SPL - off;  // chunk index of own slot q: c0 + q
        // (the blocks factor_blocks_two left are read from LDS where they are used, and step (3)'s results are committed after the cross-check: see factor_pivots_scan)
        auto ldrec = [&](int q, double r_[9]) {  // (H | ws) of own slot q as one record read; a slot without a stage: identity / zero
            const bool ex = q >= off && c0 + q < nstc;
            load9(L.fac + (ex ? c0 + q : 0) * 9 * TPs, tl < TPs ? tl : 0, r_);
            if (!ex) { r_[0] = r_[3] = r_[5] = 1.0; r_[1] = r_[2] = r_[4] = r_[6] = r_[7] = r_[8] = 0.0; }
        };
        const double pu0 = tl < C ? FU(0) : 1.0;
        double *sb = S + L.phi;
        // eliminate the stage whose pivot block / control coupling the run carries (own slot q: its outgoing transition); the next stage's own terms are added when it is
        // on this lane, else by the receiver of the run
        auto elim = [&](ChunkRun &r_, int q) {
            const Tr tq = transition(st, q, re);
            double Gi[6], Gf[9], Tm[9], Ln[9], Bn[9];
            inv3_sym(r_.G, Gi);
            sym_full(Gi, Gf);
            mul33(r_.Bf, Gf, Tm);          // T = B_f G^-1
            sym_sub_abt(r_.A, Tm, r_.Bf);  // A -= T B_f'
            mul33t(Tm, tq.E, Bn);          // T E'
            mul33(tq.E, Gf, Ln);           // L = E G^-1
            double Gn[6], rx_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (q + 1 < SPL) ldrec(q + 1 < SPL ? q + 1 : q, rx_);
#pragma unroll
            for (int i = 0; i < 6; ++i) Gn[i] = rx_[i];
            sym_sub_abt(Gn, Ln, tq.E);     // H_next - L E'
            const double lu[3] = {Gf[0] * r_.w[0] + Gf[1] * r_.w[1] + Gf[2] * r_.w[2], Gf[3] * r_.w[0] + Gf[4] * r_.w[1] + Gf[5] * r_.w[2], Gf[6] * r_.w[0] + Gf[7] * r_.w[1] + Gf[8] * r_.w[2]};
#pragma unroll
            for (int r = 0; r < 3; ++r) r_.bu[r] -= r_.Bf[3 * r] * lu[0] + r_.Bf[3 * r + 1] * lu[1] + r_.Bf[3 * r + 2] * lu[2];
            r_.pu -= lu[0] * r_.w[0] + lu[1] * r_.w[1] + lu[2] * r_.w[2];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                r_.w[r] = tq.wn0[r] - (tq.E[3 * r] * lu[0] + tq.E[3 * r + 1] * lu[1] + tq.E[3 * r + 2] * lu[2]) + rx_[6 + r];
#pragma unroll
            for (int i = 0; i < 9; ++i) r_.Bf[i] = -Bn[i];
#pragma unroll
            for (int i = 0; i < 6; ++i) r_.G[i] = Gn[i];
        };
        // ---- (1) the chunk's element: x_0 retained, chunk stages 1 .. CH-1 and the control eliminated — role A's stages, then role B's ----
        ChunkEl el;
#pragma unroll
        for (int i = 0; i < 6; ++i) { el.A[i] = (i == 0 || i == 3 || i == 5) ? 1.0 : 0.0; el.D[i] = 0.0; }
#pragma unroll
        for (int i = 0; i < 9; ++i) el.B[i] = 0.0;
        double *hb = sb + 21 * TPs;  // hand-off [28][TP] in the second buffer of the scan (the first put() goes to buffer 0)
        __syncthreads();  // (the region held the previous factorisation's tables: every reader is done)
        {
            ChunkRun rn;
            if (role == 0 && fullc) {
                double r0[9], r1[9];
                ldrec(0, r0);
                ldrec(1, r1);
#pragma unroll
                for (int i = 0; i < 6; ++i) rn.A[i] = r0[i];
                const Tr t0 = transition(st, 0, re);
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) rn.Bf[3 * r + k] = t0.E[3 * k + r];  // M[x_0, x_1] = E_0'
#pragma unroll
                for (int i = 0; i < 3; ++i) { rn.bu[i] = r0[6 + i]; rn.w[i] = t0.wn0[i] + r1[6 + i]; }
#pragma unroll
                for (int i = 0; i < 6; ++i) rn.G[i] = r1[i];
                rn.pu = pu0;
#pragma unroll
                for (int q = 1; q < SPL; ++q) elim(rn, q);
                int k = 0;
                auto putv = [&](double v) { sb[21 * TPs + k * TPs + tl] = v; ++k; };
#pragma unroll
                for (int i = 0; i < 6; ++i) putv(rn.A[i]);
#pragma unroll
                for (int i = 0; i < 9; ++i) putv(rn.Bf[i]);
#pragma unroll
                for (int i = 0; i < 3; ++i) putv(rn.bu[i]);
#pragma unroll
                for (int i = 0; i < 6; ++i) putv(rn.G[i]);
#pragma unroll
                for (int i = 0; i < 3; ++i) putv(rn.w[i]);
                putv(rn.pu);
            }
            __syncthreads();
            if (role == 1 && fullc) {
                int k = 0;
                auto getv = [&]() { const double v = hb[k * TPs + tl]; ++k; return v; };
#pragma unroll
                for (int i = 0; i < 6; ++i) rn.A[i] = getv();
#pragma unroll
                for (int i = 0; i < 9; ++i) rn.Bf[i] = getv();
#pragma unroll
                for (int i = 0; i < 3; ++i) rn.bu[i] = getv();
#pragma unroll
                for (int i = 0; i < 6; ++i) rn.G[i] = getv();
#pragma unroll
                for (int i = 0; i < 3; ++i) rn.w[i] = getv();
                rn.pu = getv();
                // role B's first stage: its own block / control coupling
#pragma unroll
                for (int q = 0; q < SPL; ++q)
                    if (q == off) {
                        double rb_[9];
                        ldrec(q, rb_);
#pragma unroll
                        for (int i = 0; i < 6; ++i) rn.G[i] += rb_[i];
#pragma unroll
                        for (int i = 0; i < 3; ++i) rn.w[i] += rb_[6 + i];
                    }
#pragma unroll
                for (int q = 0; q < SPL; ++q) if (q >= off) elim(rn, q);
                // the control
                const double pi = 1.0 / rn.pu;
                const double lb[3] = {rn.bu[0] * pi, rn.bu[1] * pi, rn.bu[2] * pi};
                rn.A[0] -= lb[0] * rn.bu[0]; rn.A[1] -= lb[0] * rn.bu[1]; rn.A[2] -= lb[0] * rn.bu[2]; rn.A[3] -= lb[1] * rn.bu[1]; rn.A[4] -= lb[1] * rn.bu[2]; rn.A[5] -= lb[2] * rn.bu[2];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k2 = 0; k2 < 3; ++k2) rn.Bf[3 * r + k2] -= lb[r] * rn.w[k2];
                const double lw[3] = {rn.w[0] * pi, rn.w[1] * pi, rn.w[2] * pi};
                rn.G[0] -= lw[0] * rn.w[0]; rn.G[1] -= lw[0] * rn.w[1]; rn.G[2] -= lw[0] * rn.w[2]; rn.G[3] -= lw[1] * rn.w[1]; rn.G[4] -= lw[1] * rn.w[2]; rn.G[5] -= lw[2] * rn.w[2];
#pragma unroll
                for (int i = 0; i < 6; ++i) { el.A[i] = rn.A[i]; el.D[i] = rn.G[i]; }
#pragma unroll
                for (int i = 0; i < 9; ++i) el.B[i] = rn.Bf[i];
            }
        }
        // ---- (2) inclusive Kogge-Stone over the chunks on the role-B lanes, double-buffered ----
        int cur = 0;
        const bool scl = role == 1 && tl < TPs;
        auto put = [&](int buf, const ChunkEl &e) {
            if (scl) {
#pragma unroll
                for (int i = 0; i < 6; ++i) { sb[(buf * 21 + i) * TPs + tl] = e.A[i]; sb[(buf * 21 + 15 + i) * TPs + tl] = e.D[i]; }
#pragma unroll
                for (int i = 0; i < 9; ++i) sb[(buf * 21 + 6 + i) * TPs + tl] = e.B[i];
            }
        };
        auto get = [&](int buf, int lane) {
            ChunkEl e;
#pragma unroll
            for (int i = 0; i < 6; ++i) { e.A[i] = sb[(buf * 21 + i) * TPs + lane]; e.D[i] = sb[(buf * 21 + 15 + i) * TPs + lane]; }
#pragma unroll
            for (int i = 0; i < 9; ++i) e.B[i] = sb[(buf * 21 + 6 + i) * TPs + lane];
            return e;
        };
        put(cur, el);
        __syncthreads();
        const int nch = (N + CH - 1) / CH;  // chunks that own a stage
        for (int d = 1; d < nch; d <<= 1) {
            if (scl && tl >= d) { const ChunkEl p = get(cur, tl - d); el = combine_el(p, el); }
            put(cur ^ 1, el);
            __syncthreads();
            cur ^= 1;
        }
        // ---- (3) own stages from G = H + Delta_t: the ordinary recursion, role A then role B ----
        double din[6] = {0, 0, 0, 0, 0, 0}, gout[6] = {0, 0, 0, 0, 0, 0};
        if (role == 0 && nstc > 0 && tl > 0) {
            const ChunkEl p = get(cur, tl - 1);  // the chunks before this one
            double Ai[6], Af[9], X[9];
            inv3_sym(p.A, Ai);
            sym_full(Ai, Af);
            const double bt[9] = {p.B[0], p.B[3], p.B[6], p.B[1], p.B[4], p.B[7], p.B[2], p.B[5], p.B[8]};
            mul33(bt, Af, X);  // B' A^-1
#pragma unroll
            for (int i = 0; i < 6; ++i) din[i] = p.D[i];
            sym_sub_abt(din, X, bt);  // D - B' A^-1 B
        }
        __syncthreads();  // every reader of the scan's result is done: the other buffer carries the hand-off (G 6, w 3, p_u 1)
        double *h2 = sb + (cur ^ 1) * 21 * TPs;
        double cG[6], cw[3], cpu = pu0;
        double Rq[SPL][9], ru[4] = {0, 0, 0, 0};  // step (3)'s results, committed after the cross-check
        bool ctl_done = false;
#pragma unroll
        for (int q = 0; q < SPL; ++q)
#pragma unroll
            for (int i = 0; i < 9; ++i) Rq[q][i] = 0;
#pragma unroll 1
        for (int r = 0; r < 2; ++r) {
            if (r == 1) {
                __syncthreads();
                if (role == 1) {
#pragma unroll
                    for (int i = 0; i < 6; ++i) cG[i] = h2[i * TPs + tl];
#pragma unroll
                    for (int i = 0; i < 3; ++i) cw[i] = h2[(6 + i) * TPs + tl];
                    cpu = h2[9 * TPs + tl];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 6; ++i) cG[i] = din[i];
                cw[0] = cw[1] = cw[2] = 0;
            }
            if (role == r && nstc > 0) {
                bool first = true;
#pragma unroll
                for (int q = 0; q < SPL; ++q) {
                    if (q < off) continue;
                    const int cq = c0 + q;
                    if (first) {  // the first own stage's own block / control coupling on top of what the recursion carries in
                        double rb_[9];
                        ldrec(q, rb_);
#pragma unroll
                        for (int i = 0; i < 6; ++i) cG[i] += rb_[i];
#pragma unroll
                        for (int i = 0; i < 3; ++i) cw[i] += rb_[6 + i];
                        first = false;
                    }
                    if (cq < nstc) {
                        double Gi[6];
                        inv3_sym(cG, Gi);
#pragma unroll
                        for (int i = 0; i < 6; ++i) Rq[q][i] = Gi[i];
                        if (cq < nqc) {  // the transition out of this stage (the final stage of the path has none: its pivot inverse only)
#pragma unroll
                            for (int i = 0; i < 3; ++i) Rq[q][6 + i] = cw[i];
                            const Tr tq = transition(st, q, re);
                            double Gf[9], Ln[9];
                            sym_full(Gi, Gf);
                            mul33(tq.E, Gf, Ln);
                            double Gn[6], rx_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                            if (q + 1 < SPL) ldrec(q + 1 < SPL ? q + 1 : q, rx_);
#pragma unroll
                            for (int i = 0; i < 6; ++i) Gn[i] = rx_[i];
                            sym_sub_abt(Gn, Ln, tq.E);
                            const double lu[3] = {Gf[0] * cw[0] + Gf[1] * cw[1] + Gf[2] * cw[2], Gf[3] * cw[0] + Gf[4] * cw[1] + Gf[5] * cw[2], Gf[6] * cw[0] + Gf[7] * cw[1] + Gf[8] * cw[2]};
                            double wn[3];
#pragma unroll
                            for (int k = 0; k < 3; ++k) wn[k] = tq.wn0[k] - (tq.E[3 * k] * lu[0] + tq.E[3 * k + 1] * lu[1] + tq.E[3 * k + 2] * lu[2]);
                            cpu -= lu[0] * cw[0] + lu[1] * cw[1] + lu[2] * cw[2];
                            if (cq + 1 == nqc) {  // last transition of the group: the control
                                const double pi = 1.0 / cpu;
                                const double lx[3] = {wn[0] * pi, wn[1] * pi, wn[2] * pi};
                                Gn[0] -= lx[0] * wn[0]; Gn[1] -= lx[0] * wn[1]; Gn[2] -= lx[0] * wn[2]; Gn[3] -= lx[1] * wn[1]; Gn[4] -= lx[1] * wn[2]; Gn[5] -= lx[2] * wn[2];
                                ru[0] = pi; ru[1] = lx[0]; ru[2] = lx[1]; ru[3] = lx[2]; ctl_done = true;
                                cw[0] = cw[1] = cw[2] = 0;
                            } else {
#pragma unroll
                                for (int k = 0; k < 3; ++k) cw[k] = wn[k] + rx_[6 + k];
                            }
#pragma unroll
                            for (int i = 0; i < 6; ++i) cG[i] = Gn[i];
                        }
                    }
                }
                if (r == 0) {
#pragma unroll
                    for (int i = 0; i < 6; ++i) h2[i * TPs + tl] = cG[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) h2[(6 + i) * TPs + tl] = cw[i];
                    h2[9 * TPs + tl] = cpu;
                } else {
#pragma unroll
                    for (int i = 0; i < 6; ++i) gout[i] = cG[i];  // a full chunk: the correction its OWN recursion passes on (cross-checked below against the scan's)
                }
            }
        }
        // ---- (4) cross-check (see factor_pivots_scan) ----
        __syncthreads();
        if (scl) {
#pragma unroll
            for (int i = 0; i < 6; ++i) sb[i * TPs + tl] = gout[i];
        }
        __syncthreads();
        bool bad = false;
        if (role == 0 && nstc > 0 && tl > 0) {
            double wd = 0, wr = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) { wd = fmax(wd, fabs(sb[i * TPs + tl - 1] - din[i])); wr = fmax(wr, fabs(din[i])); }
            bad = !(wd <= kScanTol * wr) || nonfinite_bits(wd) != 0;
            if (in.dbg_cycles != nullptr && wr > 0) atomicMax(reinterpret_cast<unsigned long long *>(in.dbg_cycles + (size_t)b * 16 + 15), (unsigned long long)__double_as_longlong(wd / wr));  // dev: worst relative disagreement seen
        }
        const bool any_bad = block_any(bad);
        if (in.dbg_cycles != nullptr && tid == 0) { long long *d = in.dbg_cycles + (size_t)b * 16; d[13] += 1; d[14] += any_bad ? 1 : 0; }  // dev: factorisations / fallbacks of this path
        if (!any_bad) {  // commit (a failed check leaves the blocks of factor_blocks_two in LDS untouched: the sequential recursion starts from them)
#pragma unroll
            for (int q = 0; q < SPL; ++q) {
                if (q >= off && c0 + q < nstc && tl < TPs) store9(L.fac + (c0 + q) * 9 * TPs, tl, Rq[q]);
            }
            if (ctl_done) { FU(0) = ru[0]; FU(1) = ru[1]; FU(2) = ru[2]; FU(3) = ru[3]; }
        }
        __syncthreads();
        return !any_bad;
    }

// ==================== [two_factor_chain] ====================
// members of Fast, part 5: factor_chain_two, factorisation step B of the two-level mapping and the tables of its solve.  TWO only, every NWX.
// Three parts (the PO_FC_TICK buckets of a PO_NW_TRACE build): (0) the pivot chain as a scan ([two_pivot_scan]); when its cross-check fails, the sequential block
// LDL' over all stages, every lane running the same recursion on broadcast reads; (1) Phi_t of every full chunk, column by column through the homogeneous forward sweep
// (sweep_forward<2> / split_forward<2>, [two_sweeps]); (2) the prefix tables of the boundary scans: one wave — in-row levels 0..3, Q^incl (4), Q^suf (5) of the
// 16-lane DPP rows; SEG (NT > 64, one lane per chunk) — levels 0..2 inside 8-lane segments, Q^incl (3), Q^suf (4) and the segment products R^(l) in rseg.
//   LDS     reads fac / facu as factor_blocks_two left them and replaces them by the factor (Ginv | w, 1 / p_u | l_x); the fall-back's (k, ds, trig) table [N][4] lies
//           on phi (LayoutF's wt alias), which is rebuilt right after; writes phi (every level) and rseg; role-split: the Phi columns cross the roles through hx0 / hx1
//   lanes   reads the transition inputs; writes nothing (the homogeneous sweeps take no right-hand side and store nothing)
//   called  after every factor_blocks_two: admm_loop, refine_phase_newton ([loops]), polish_kernel
    // sequential block LDL' (every lane of every wave runs the same scalar recursion on broadcast reads — no
    // cross-wave hand-off needed; thread 0 stores).  The coupling blocks are regenerated from the owner's registers.
    __device__ __forceinline__ void factor_chain_two(LS &st, double rho) const {
        const double rho_eq = eq_step(rho);
        double re[T::NDYN];
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) re[r] = eq_row_step(rho_eq, r);
        bool scanned = false;
#ifdef PO_NW_TRACE
        long long tf_ = __builtin_readcyclecounter();
#endif
        // the pivot chain as a scan over chunks ([two_pivot_scan]); false: its cross-check failed, the sequential recursion below runs instead
        if constexpr (NW == 1) scanned = factor_pivots_scan(st, re); else scanned = factor_pivots_scan2(st, re);
        PO_FC_TICK(0)
        if (!scanned) {
            // publish per-stage (k, ds) of the outgoing transitions so that every lane can rebuild E_j
            double *kd = S + L.phi;  // scratch [N][4]: k, ds (+ K's cached trig) of the transition out of stage j (phi is rebuilt below)
    #pragma unroll
            for (int q = 0; q < SPL; ++q) {
                const int j = stage(q);
                if (j < N) {
                    kd[4 * j] = q + 1 < SPL ? st.kin[q + 1 < SPL ? q + 1 : q] : st.kout;
                    kd[4 * j + 1] = q + 1 < SPL ? st.dsin[q + 1 < SPL ? q + 1 : q] : st.dsout;
                    if constexpr (F == F_K) {
                        kd[4 * j + 2] = q + 1 < SPL ? st.trin[q + 1 < SPL ? q + 1 : q][0] : st.trout[0];
                        kd[4 * j + 3] = q + 1 < SPL ? st.trin[q + 1 < SPL ? q + 1 : q][1] : st.trout[1];
                    }
                }
            }
            __syncthreads();
            {
                double G[6], w[3] = {0, 0, 0}, pu = 0;
    #pragma unroll
                for (int i = 0; i < 6; ++i) G[i] = FAt(0, 0, i);
                if constexpr (T::HAS_U) { w[0] = FAt(0, 0, 6); w[1] = FAt(0, 0, 7); w[2] = FAt(0, 0, 8); pu = FUc(0, 0); }
                int c = 0, gcnt = 0;
                for (int j = 0; j < N - 1; ++j) {
                    const int t = j / CH, q = j % CH;
                    // what this step needs from LDS does not depend on the pivot chain: requested first, the 3 x 3 inverse (a division) runs meanwhile
                    const int tn = (j + 1) / CH, qn = (j + 1) % CH;
                    const double trj[2] = {kd[4 * j + 2], kd[4 * j + 3]};
                    const double kj_ = kd[4 * j], dsj_ = kd[4 * j + 1];
                    double Gn[6], wsn[3];
    #pragma unroll
                    for (int i = 0; i < 6; ++i) Gn[i] = FAt(tn, qn, i);
    #pragma unroll
                    for (int i = 0; i < 3; ++i) wsn[i] = FAt(tn, qn, 6 + i);
                    double Gi[6];
                    inv3_sym(G, Gi);
                    const Dyn<F> d = make_dyn_tr<F>(kj_, dsj_, trj, P);
                    double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, wn[3] = {0, 0, 0};
    #pragma unroll
                    for (int r = 0; r < T::NDYN; ++r) {
                        const int tt = dyn_tau<F>(r);
    #pragma unroll
                        for (int cc = 0; cc < 3; ++cc) E[tt * 3 + cc] += -re[r] * d.f[r][cc];
                        wn[tt] += -re[r] * d.beta[r];
                    }
                    if constexpr (F == F_K) { if (j + 1 <= N - 2) E[8] += -P.w_cr; }
                    const double Gf[9] = {Gi[0], Gi[1], Gi[2], Gi[1], Gi[3], Gi[4], Gi[2], Gi[4], Gi[5]};
                    double Ln[9];
    #pragma unroll
                    for (int r = 0; r < 3; ++r)
    #pragma unroll
                        for (int k = 0; k < 3; ++k) Ln[r * 3 + k] = E[r * 3 + 0] * Gf[k] + E[r * 3 + 1] * Gf[3 + k] + E[r * 3 + 2] * Gf[6 + k];
                    Gn[0] -= Ln[0] * E[0] + Ln[1] * E[1] + Ln[2] * E[2];
                    Gn[1] -= Ln[0] * E[3] + Ln[1] * E[4] + Ln[2] * E[5];
                    Gn[2] -= Ln[0] * E[6] + Ln[1] * E[7] + Ln[2] * E[8];
                    Gn[3] -= Ln[3] * E[3] + Ln[4] * E[4] + Ln[5] * E[5];
                    Gn[4] -= Ln[3] * E[6] + Ln[4] * E[7] + Ln[5] * E[8];
                    Gn[5] -= Ln[6] * E[6] + Ln[7] * E[7] + Ln[8] * E[8];
                    const double wcur[3] = {w[0], w[1], w[2]};
                    if constexpr (T::HAS_U) {
                        const double lu[3] = {Gf[0] * w[0] + Gf[1] * w[1] + Gf[2] * w[2], Gf[3] * w[0] + Gf[4] * w[1] + Gf[5] * w[2],
                                              Gf[6] * w[0] + Gf[7] * w[1] + Gf[8] * w[2]};
    #pragma unroll
                        for (int r = 0; r < 3; ++r) wn[r] -= E[r * 3 + 0] * lu[0] + E[r * 3 + 1] * lu[1] + E[r * 3 + 2] * lu[2];
                        pu -= lu[0] * w[0] + lu[1] * w[1] + lu[2] * w[2];
                        ++gcnt;
                        if (gcnt == GK || j == N - 2) {
                            gcnt = 0;
                            const double pi = 1.0 / pu;
                            const double lx[3] = {wn[0] * pi, wn[1] * pi, wn[2] * pi};
                            Gn[0] -= lx[0] * wn[0]; Gn[1] -= lx[0] * wn[1]; Gn[2] -= lx[0] * wn[2];
                            Gn[3] -= lx[1] * wn[1]; Gn[4] -= lx[1] * wn[2]; Gn[5] -= lx[2] * wn[2];
                            if (tid == 0) { FUc(c, 0) = pi; FUc(c, 1) = lx[0]; FUc(c, 2) = lx[1]; FUc(c, 3) = lx[2]; }
                            ++c;
                            if (j + 1 <= N - 2) { w[0] = wsn[0]; w[1] = wsn[1]; w[2] = wsn[2]; pu = FUc(c, 0); }
                        } else {
                            w[0] = wn[0] + wsn[0]; w[1] = wn[1] + wsn[1]; w[2] = wn[2] + wsn[2];
                        }
                    }
                    __syncthreads();  // everybody has read stage j / j+1 before thread 0 overwrites stage j
                    if (tid == 0) {
    #pragma unroll
                        for (int i = 0; i < 6; ++i) FAt(t, q, i) = Gi[i];
                        FAt(t, q, 6) = wcur[0]; FAt(t, q, 7) = wcur[1]; FAt(t, q, 8) = wcur[2];
                    }
    #pragma unroll
                    for (int i = 0; i < 6; ++i) G[i] = Gn[i];
                }
                {   // final stage: its pivot inverse only
                    double Gi[6];
                    inv3_sym(G, Gi);
                    if (tid == 0) {
    #pragma unroll
                        for (int i = 0; i < 6; ++i) FAt((N - 1) / CH, (N - 1) % CH, i) = Gi[i];
                    }
                }
            }
            __syncthreads();
        }
        // ---- chunk transfer matrices Phi_t and their Kogge-Stone prefix products ----
        double ph[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const bool tw = wrole() == NW - 1 && clane() < L.TP;  // the lanes that write the chunk tables (NW == 2: the wave the chunk's outflow ends up in)
        if constexpr (NW == 1) {
            double fu[NG][4];
#pragma unroll
            for (int g = 0; g < NG; ++g) { fu[g][0] = fu[g][1] = fu[g][2] = fu[g][3] = 0; if constexpr (T::HAS_U) { fu[g][0] = FUg(g, 0); fu[g][1] = FUg(g, 1); fu[g][2] = FUg(g, 2); fu[g][3] = FUg(g, 3); } }
            if (nq_own() == SPL) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double y[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0}, acc[NG];
#pragma unroll
                    for (int g = 0; g < NG; ++g) acc[g] = 0;
                    sweep_forward<2>(st, y, SPL, acc, re, fu);
#pragma unroll
                    for (int r = 0; r < 3; ++r) ph[3 * r + k] = y[r];
                }
            }
        } else {
            double fu[4];
            load_fu(fu);
            const bool fullc = nq_chunk() == CH;
#pragma unroll 1
            for (int k = 0; k < 3; ++k) {
                const double yin[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
                double out[3], yu;
                split_forward<2>(st, yin, out, yu, re, fu);
                __syncthreads();  // (slot 0 is rewritten by the next column's sweep)
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double v_ = fullc ? out[r] : 0.0;
                    ph[3 * r + 0] = k == 0 ? v_ : ph[3 * r + 0]; ph[3 * r + 1] = k == 1 ? v_ : ph[3 * r + 1]; ph[3 * r + 2] = k == 2 ? v_ : ph[3 * r + 2];
                }
            }
        }
        if (tw) store9(L.phi, clane(), ph);
        __syncthreads();
        PO_FC_TICK(1)
        if constexpr (SEG) {
            // ---- segmented tables: Q^(l)_t = Phi_t..Phi_{t-2^l+1} inside 8-lane segments (levels 0..2), Q^incl (level 3),
            //      Q^suf_t = Phi_{segment end}..Phi_t (level 4), and the Kogge-Stone products R^(l)_g of the segment maps ----
            for (int lvl = 0; lvl < 3; ++lvl) {
                const int dd = 1 << lvl;
                double pn[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) pn[i] = ph[i];
                if ((tid & 7) >= dd && tid < L.TP) {
                    double pb[9];
#pragma unroll
                    for (int i = 0; i < 9; ++i) pb[i] = PL(lvl, tid - dd, i);
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int k = 0; k < 3; ++k) pn[3 * r + k] = ph[3 * r] * pb[k] + ph[3 * r + 1] * pb[3 + k] + ph[3 * r + 2] * pb[6 + k];
                }
#pragma unroll
                for (int i = 0; i < 9; ++i) { ph[i] = pn[i]; if (tid < L.TP) PL(lvl + 1, tid, i) = pn[i]; }
                __syncthreads();
            }
            // suffix products, built in place in level 4 (starts as Phi_t = level 0)
            double qs[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) { qs[i] = tid < L.TP ? PL(0, tid, i) : 0.0; if (tid < L.TP) PL(4, tid, i) = qs[i]; }
            __syncthreads();
            for (int lvl = 0; lvl < 3; ++lvl) {
                const int dd = 1 << lvl;
                double pn[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) pn[i] = qs[i];
                if ((tid & 7) + dd <= 7 && tid + dd < L.TP) {
                    double pa[9];  // product over the lanes above: Q^suf(lvl)_{t+dd}
#pragma unroll
                    for (int i = 0; i < 9; ++i) pa[i] = PL(4, tid + dd, i);
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int k = 0; k < 3; ++k) pn[3 * r + k] = pa[3 * r] * qs[k] + pa[3 * r + 1] * qs[3 + k] + pa[3 * r + 2] * qs[6 + k];
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 9; ++i) { qs[i] = pn[i]; if (tid < L.TP) PL(4, tid, i) = pn[i]; }
                __syncthreads();
            }
            // segment maps R_g = Q^incl at the segment's last lane; their prefix products by lanes 0..15
            const int nsg = (L.TP + 7) >> 3;
            double rr_[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) rr_[i] = 0.0;
            if (tid < nsg) {
                const int tl = tid * 8 + 7;
#pragma unroll
                for (int i = 0; i < 9; ++i) { rr_[i] = tl < L.TP ? PL(3, tl, i) : 0.0; RS(0, tid, i) = rr_[i]; }
            }
            __syncthreads();
            for (int lvl = 0; lvl < 4; ++lvl) {
                const int dd = 1 << lvl;
                double pn[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) pn[i] = rr_[i];
                if (tid < nsg && tid >= dd) {
                    double pb[9];
#pragma unroll
                    for (int i = 0; i < 9; ++i) pb[i] = RS(lvl, tid - dd, i);
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int k = 0; k < 3; ++k) pn[3 * r + k] = rr_[3 * r] * pb[k] + rr_[3 * r + 1] * pb[3 + k] + rr_[3 * r + 2] * pb[6 + k];
                }
                if (tid < nsg) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) { rr_[i] = pn[i]; RS(lvl + 1, tid, i) = pn[i]; }
                }
                __syncthreads();
            }
        } else {
            // ---- one wave: row-segmented tables (rows of 16 lanes = the reach of a DPP row shift).  Levels 0..3: Q^(l)_t = Phi_t..Phi_{t-2^l+1}
            //      inside the row; level 4: Q^incl_t = Phi_t..Phi_{row start}; level 5: Q^suf_t = Phi_{row end}..Phi_t.  Chunks that are not full
            //      have Phi = 0, so every product that reaches them is zero and the scans need no predicates. ----
            for (int lvl = 0; lvl < 4; ++lvl) {
                const int dd = 1 << lvl;
                double pn[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) pn[i] = ph[i];
                if ((clane() & 15) >= dd && clane() < L.TP) {
                    double pb[9];
                    load9(L.phi + lvl * 9 * L.TP, clane() - dd, pb);
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int k = 0; k < 3; ++k) pn[3 * r + k] = ph[3 * r] * pb[k] + ph[3 * r + 1] * pb[3 + k] + ph[3 * r + 2] * pb[6 + k];
                }
#pragma unroll
                for (int i = 0; i < 9; ++i) ph[i] = pn[i];
                if (tw) store9(L.phi + (lvl + 1) * 9 * L.TP, clane(), pn);
                __syncthreads();
            }
            double qs[9];
            load9(L.phi, clane() < L.TP ? clane() : 0, qs);
#pragma unroll
            for (int i = 0; i < 9; ++i) qs[i] = clane() < L.TP ? qs[i] : 0.0;
            if (tw) store9(L.phi + 5 * 9 * L.TP, clane(), qs);
            __syncthreads();
            for (int lvl = 0; lvl < 4; ++lvl) {
                const int dd = 1 << lvl;
                double pn[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) pn[i] = qs[i];
                if ((clane() & 15) + dd <= 15 && clane() + dd < L.TP) {
                    double pa[9];  // product over the lanes above: Q^suf(lvl)_{t+dd}
                    load9(L.phi + 5 * 9 * L.TP, clane() + dd, pa);
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int k = 0; k < 3; ++k) pn[3 * r + k] = pa[3 * r] * qs[k] + pa[3 * r + 1] * qs[3 + k] + pa[3 * r + 2] * qs[6 + k];
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 9; ++i) qs[i] = pn[i];
                if (tw) store9(L.phi + 5 * 9 * L.TP, clane(), pn);
                __syncthreads();
            }
        }
        PO_FC_TICK(2)
    }

// ==================== [two_sweeps] ====================
// members of Fast, part 6: the chunk-local substitution sweeps of the two-level solve, and the whole solve of the role-split mapping.  TWO only.
//   sweep_forward<MODE> / sweep_backward<STORE>     NW 1 (NWX 1, 4, 5): the own chunk on the own lane — called by solve_two ([two_solve]) and, MODE 2, by factor_chain_two
//   hx_put / hx_get, load_fu, split_forward<MODE> / split_backward<STORE>, scan_forward_wave / scan_backward_wave, solve_split
//                                                   NW 2 (NWX 2, 3): a chunk across its two lanes — solve_split is called by admm_loop and refine_phase_newton in
//                                                   solve_two's place, split_forward<2> by factor_chain_two
//   LDS     reads fac (one 9-record per stage, requested a stage ahead), facu (once per solve, by the caller), phi (the scans); role-split: the 3-vector (+ control
//           accumulator) that crosses the role boundary goes through hx0 (A -> B forward, B -> next chunk's A backward, role A's scan result)
//           and hx1 (B -> A backward, role B's scan result), one barrier each; hx1 is also ex — no block reduction may run between these barriers
//   lanes   in: st.bx, st.bxu (right-hand side, rhs_pass_two), st.bnext (NW 1: the next chunk's first right-hand side); out: st.bx, st.bxu (solution), st.bnext / st.bprev
//           (the neighbouring chunks' boundary values, for update_pass_two)
// TWINS: scan_forward_wave / scan_backward_wave are the one-wave PO_FWD_LEVEL / PO_BWD_LEVEL scans of solve_two ([two_solve]) with the lane taken from clane() and
// the row totals read at lane_base; a change to one belongs in the other.
    // Local forward sweep over the first nq transitions of the own chunk.
    //   MODE 0: rhs from st.bx, nothing stored (zero-inflow pass); MODE 1: as 0 but stores z_q = Ginv_q y_q into st.bx;
    //   MODE 2: homogeneous (rhs = 0), used to build Phi.
    // y: inflow at own stage 0, on return the value at the stage after the last transition (the control's column
    // already applied).  acc: running control rhs in, y_u out.
    // Multi-group mapping: acc / fu are per group of the lane, and a control's column is applied after the last transition of ITS group (grp_end).
    template <int MODE> __device__ __forceinline__ void sweep_forward(LS &st, double y[3], int nq, double acc[NG], const double re[T::NDYN], const double fu[NG][4]) const {
        // fu = (pu_inv, lx[3]) of the own control, read ONCE per solve by the caller (a ds_read + wait per use inside the stage loop costs a
        // full LDS round trip on the dependent chain); the factor of stage q+1 is requested before stage q is computed.
        double g[9];
        load9(L.fac, tid, g);
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            double gn[9];
            if (q + 1 < SPL) load9(L.fac + (q + 1 < SPL ? q + 1 : q) * 9 * L.TP, tid, gn);
            if (q < nq) {
                const int j = stage(q);
                double z[3], ez[3];
                mul_Gr(g, y, z);
                if (MODE == 1) { st.bx[q][0] = z[0]; st.bx[q][1] = z[1]; st.bx[q][2] = z[2]; }
                if constexpr (T::HAS_U) acc[gOut(q)] -= g[6] * z[0] + g[7] * z[1] + g[8] * z[2];
                const Dyn<F> d = dyn_out(st, q);
                apply_E(d, re, j + 1 <= N - 2, z, ez);
                double b[3] = {0, 0, 0};
                if (MODE != 2) {
                    if (q + 1 < SPL) { b[0] = st.bx[q + 1 < SPL ? q + 1 : q][0]; b[1] = st.bx[q + 1 < SPL ? q + 1 : q][1]; b[2] = st.bx[q + 1 < SPL ? q + 1 : q][2]; }
                    else { b[0] = st.bnext[0]; b[1] = st.bnext[1]; b[2] = st.bnext[2]; }
                }
                y[0] = b[0] + ez[0]; y[1] = b[1] + ez[1]; y[2] = b[2] + ez[2];
                if (grp_end(q, nq)) {
                    if constexpr (T::HAS_U) { y[0] -= fu[gOut(q)][1] * acc[gOut(q)]; y[1] -= fu[gOut(q)][2] * acc[gOut(q)]; y[2] -= fu[gOut(q)][3] * acc[gOut(q)]; }
                }
            }
            if (q + 1 < SPL) {
#pragma unroll
                for (int i = 0; i < 9; ++i) g[i] = gn[i];
            }
        }
    }
    // Local backward sweep: x enters as the solution at the stage after the last own transition, leaves as the
    // solution at own stage 0.  st.bx holds z_q.  STORE: write the solution into st.bx / st.bxu[0].
    template <bool STORE> __device__ __forceinline__ void sweep_backward(LS &st, double x[3], int nq, const double re[T::NDYN], const double fu[NG][4]) const {
        double xu = 0;
        double gr[9];
        load9(L.fac + (SPL - 1) * 9 * L.TP, tid, gr);
        if constexpr (T::HAS_U && NG == 1) {
            if (nq > 0) xu = st.bxu[0] - (fu[0][1] * x[0] + fu[0][2] * x[1] + fu[0][3] * x[2]);
            if (STORE) st.bxu[0] = xu;
        }
        if constexpr (NG > 1 && STORE) {  // (groups of the lane without a transition: their control does not exist)
#pragma unroll
            for (int g = 0; g < NG; ++g) if (!(g * GK < nq)) st.bxu[g] = 0.0;
        }
#pragma unroll
        for (int q = SPL - 1; q >= 0; --q) {
            double gn[9];
            if (q > 0) load9(L.fac + (q > 0 ? q - 1 : 0) * 9 * L.TP, tid, gn);  // next stage's factor in flight while this one is applied
            if (q < nq) {
                const int j = stage(q);
                const Dyn<F> d = dyn_out(st, q);
                double t[3], g[3];
                if constexpr (NG > 1) {  // the control of this transition's group: solved from the stage after the group's last transition (x holds it right now)
                    if (grp_end(q, nq)) { xu = st.bxu[gOut(q)] - (fu[gOut(q)][1] * x[0] + fu[gOut(q)][2] * x[1] + fu[gOut(q)][3] * x[2]); if (STORE) st.bxu[gOut(q)] = xu; }
                }
                apply_Et(d, re, j + 1 <= N - 2, x, t);
                if constexpr (T::HAS_U) { t[0] += gr[6] * xu; t[1] += gr[7] * xu; t[2] += gr[8] * xu; }
                mul_Gr(gr, t, g);
                x[0] = st.bx[q][0] - g[0]; x[1] = st.bx[q][1] - g[1]; x[2] = st.bx[q][2] - g[2];
                if (STORE) { st.bx[q][0] = x[0]; st.bx[q][1] = x[1]; st.bx[q][2] = x[2]; }
            }
            if (q > 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) gr[i] = gn[i];
            }
        }
    }

    // =====================================================================================================
    // ROLE-SPLIT MAPPING (NW == 2): the sweeps of a chunk run on role A (chunk stages 0 .. SPL-1), then role B (the rest; the control where its elimination falls); what
    // crosses the role boundary is a 3-vector (+ the running control accumulator) through one of two LDS slots and one barrier (NT = 64: both roles are lanes of ONE wave,
    // the barrier is free; NT = 128: one wave per role).  The chunk-boundary scans are the one-wave DPP scans, forward on the role-B lanes (where the chunk outflows are),
    // backward on the role-A lanes (where the chunk-entry solutions are).
    // Convention: the inflow `yin` of a chunk EXCLUDES the rhs of its first stage (the receiver adds its own rhs), so no rhs travels between lanes.
    // =====================================================================================================
    __device__ __forceinline__ void hx_put(int slot, const double v[4]) const {
        if (clane() < L.TP) {
#pragma unroll
            for (int k = 0; k < 4; ++k) S[slot + k * L.TP + clane()] = v[k];
        }
    }
    __device__ __forceinline__ void hx_get(int slot, int lane, double v[4]) const {  // lane out of range: zeros
        const bool ok = lane >= 0 && lane < L.TP;
        const int l_ = ok ? lane : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const double t_ = S[slot + k * L.TP + l_]; v[k] = ok ? t_ : 0.0; }
    }
    // own control's factor entries (pu_inv, lx[3]): read once per solve by BOTH roles (the elimination falls in role A in a final chunk with < SPL transitions)
    __device__ __forceinline__ void load_fu(double fu[4]) const {
        fu[0] = fu[1] = fu[2] = fu[3] = 0;
        if constexpr (T::HAS_U) { if (clane() < L.TP) { fu[0] = FU(0); fu[1] = FU(1); fu[2] = FU(2); fu[3] = FU(3); } }
    }
    // Forward sweep of the own chunk across both roles.  MODE 0: nothing stored; MODE 1: z_q = Ginv_q y_q stored in st.bx; MODE 2: homogeneous (rhs = 0).
    // In: st.bx = rhs of the own stages, st.bxu[0] = this lane's share of the control's rhs (rhs_pass_two).  Out (role B): out = outflow of a full chunk (after the
    // control's column); yu (the role that eliminated the control) = the control's forward-substituted rhs.  One barrier.
    template <int MODE> __device__ __forceinline__ void split_forward(LS &st, const double yin[3], double out[3], double &yu, const double re[T::NDYN], const double fu[4]) const {
        const int nqc = nq_chunk(), nstc = nst_chunk();
        out[0] = out[1] = out[2] = 0; yu = 0;
        double msg[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int r = 0; r < 2; ++r) {
            if (r == 1) { __syncthreads(); if (wrole() == 1) hx_get(L.hx0, clane(), msg); }
            if (wrole() == r) {
                const int off = qoff(), c0 = r * SPL - off;  // chunk index of own slot q: c0 + q
                double acc = (MODE != 2 ? st.bxu[0] : 0.0) + msg[3];
                double y[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) y[k] = (r == 0 ? yin[k] : msg[k]);
                // the control's column at the role boundary (the group's last transition was role A's last: both shares of the accumulator are here now)
                if (r == 1 && nqc == SPL) { y[0] -= fu[1] * acc; y[1] -= fu[2] * acc; y[2] -= fu[3] * acc; yu = acc; }
                bool first = true;
#pragma unroll
                for (int q = 0; q < SPL; ++q) {
                    if (q < off) continue;
                    const int cq = c0 + q;
                    if (MODE != 2 && first) { y[0] += st.bx[q][0]; y[1] += st.bx[q][1]; y[2] += st.bx[q][2]; }
                    first = false;
                    double g[9], z[3];
                    load9(L.fac + cq * 9 * L.TP, clane(), g);
                    mul_Gr(g, y, z);
                    if (MODE == 1 && cq < nstc) { st.bx[q][0] = z[0]; st.bx[q][1] = z[1]; st.bx[q][2] = z[2]; }
                    if (cq < nqc) {
                        double ez[3];
                        acc -= g[6] * z[0] + g[7] * z[1] + g[8] * z[2];
                        apply_E(dyn_out(st, q), re, false, z, ez);
#pragma unroll
                        for (int k = 0; k < 3; ++k) y[k] = ez[k] + ((MODE != 2 && q + 1 < SPL) ? st.bx[q + 1 < SPL ? q + 1 : q][k] : 0.0);
                        // last transition of the group: the control's column (deferred to role B's entry when it is role A's last transition, see above)
                        if (cq + 1 == nqc && !(r == 0 && q == SPL - 1)) { y[0] -= fu[1] * acc; y[1] -= fu[2] * acc; y[2] -= fu[3] * acc; yu = acc; }
                    }
                }
                if (r == 0) { msg[0] = y[0]; msg[1] = y[1]; msg[2] = y[2]; msg[3] = acc; hx_put(L.hx0, msg); }
                else if (nqc == CH) { out[0] = y[0]; out[1] = y[1]; out[2] = y[2]; }
            }
        }
    }
    // Backward sweep of the own chunk across both roles (B then A).  Role B: xin = solution at the next chunk's first stage (full chunks); the chunk that holds the final
    // stage starts from that stage's own z.  st.bx holds z_q, st.bxu[0] (control owner) the control's D^-1 y.  STORE: solutions into st.bx / st.bxu[0] (both roles end up with the
    // chunk's control in st.bxu[0]).  Role A returns x0 = the solution at chunk stage 0 and xnext = the solution at chunk stage SPL.  One barrier (slot 1); with STORE role B
    // also posts (its last stage, the control) into slot 0 for role A of the NEXT chunk.
    template <bool STORE> __device__ __forceinline__ void split_backward(LS &st, const double xin[3], double x0[3], double xnext[3], const double re[T::NDYN], const double fu[4]) const {
        const int nqc = nq_chunk();
        x0[0] = x0[1] = x0[2] = 0; xnext[0] = xnext[1] = xnext[2] = 0;
        double msg[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int r = 1; r >= 0; --r) {
            if (r == 0) { __syncthreads(); if (wrole() == 0) hx_get(L.hx1, clane(), msg); }
            if (wrole() == r) {
                const int off = qoff(), c0 = r * SPL - off;
                // entry: the solution at the stage after this role's last transition, and the control
                double x[3] = {0, 0, 0}, xu = 0;
                const int kf = nqc - c0;  // own slot of the path's final stage when it lies in this role's part of the (final) chunk
                if (r == 1) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) x[k] = nqc == CH ? xin[k] : 0.0;
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k) { x[k] = msg[k]; xnext[k] = msg[k]; }
                    xu = msg[3];
                }
                if (nqc < CH) {  // the chunk that holds the final stage: its z is its solution
#pragma unroll
                    for (int q = 0; q < SPL; ++q) if (q == kf && q >= off) { x[0] = st.bx[q][0]; x[1] = st.bx[q][1]; x[2] = st.bx[q][2]; }
                }
                if (T::HAS_U && r == own_role() && nqc > 0) xu = st.bxu[0] - (fu[1] * x[0] + fu[2] * x[1] + fu[3] * x[2]);
#pragma unroll
                for (int q = SPL - 1; q >= 0; --q) {
                    if (q < off) continue;
                    const int cq = c0 + q;
                    if (cq < nqc) {
                        double g[9], t[3], gt[3];
                        load9(L.fac + cq * 9 * L.TP, clane(), g);
                        apply_Et(dyn_out(st, q), re, false, x, t);
                        t[0] += g[6] * xu; t[1] += g[7] * xu; t[2] += g[8] * xu;
                        mul_Gr(g, t, gt);
                        x[0] = st.bx[q][0] - gt[0]; x[1] = st.bx[q][1] - gt[1]; x[2] = st.bx[q][2] - gt[2];
                        if (STORE) { st.bx[q][0] = x[0]; st.bx[q][1] = x[1]; st.bx[q][2] = x[2]; }
                    }
                }
                if (STORE) st.bxu[0] = xu;
                if (r == 1) {
                    if (STORE) { const double nb[4] = {st.bx[SPL - 1][0], st.bx[SPL - 1][1], st.bx[SPL - 1][2], xu}; hx_put(L.hx0, nb); }  // last stage + control, for role A of the next chunk
                    msg[0] = x[0]; msg[1] = x[1]; msg[2] = x[2]; msg[3] = xu;
                    hx_put(L.hx1, msg);
                } else { x0[0] = x[0]; x0[1] = x[1]; x0[2] = x[2]; }
            }
        }
    }
    // one-wave boundary scans on the chunk lanes of the calling role (the DPP row scans of solve_two; tables of chunks that are not full are zero).  NT = 64: the role's lanes
    // are one half of the wave (two DPP rows); the row totals are read with v_readlane at the role's lane offset.
    // (twin: the one-wave branches of solve_two's F2 / B2, [two_solve] — calling these from there changes solve_two's device code, so the text stands twice)
    __device__ __forceinline__ void scan_forward_wave(double s[3], int lane_base) const {
        const int tfull = (N - 1) / CH;
        const int tp_ = clane() < L.TP ? clane() : tfull;
        double pa[9], pb[9];
        load9(L.phi, tp_, pa);
#define PO_FWD_LEVEL(LVL, PC, PN) \
        { \
            load9(L.phi + (LVL + 1) * 9 * L.TP, tp_, PN); \
            const double o0 = dpp_mov0<kDppRowShr + (1 << LVL)>(s[0]), o1 = dpp_mov0<kDppRowShr + (1 << LVL)>(s[1]), o2 = dpp_mov0<kDppRowShr + (1 << LVL)>(s[2]); \
            s[0] += PC[0] * o0 + PC[1] * o1 + PC[2] * o2; \
            s[1] += PC[3] * o0 + PC[4] * o1 + PC[5] * o2; \
            s[2] += PC[6] * o0 + PC[7] * o1 + PC[8] * o2; \
        }
        PO_FWD_LEVEL(0, pa, pb) PO_FWD_LEVEL(1, pb, pa) PO_FWD_LEVEL(2, pa, pb) PO_FWD_LEVEL(3, pb, pa)
#undef PO_FWD_LEVEL
        const int nrow = (L.TP + 15) >> 4;
        const int row = clane() >> 4;
        for (int r = 1; r < nrow; ++r) {
            const bool sel = row == r;
            const double c0 = bcast(s[0], lane_base + 16 * r - 1), c1 = bcast(s[1], lane_base + 16 * r - 1), c2 = bcast(s[2], lane_base + 16 * r - 1);
            const double a0 = pa[0] * c0 + pa[1] * c1 + pa[2] * c2;
            const double a1 = pa[3] * c0 + pa[4] * c1 + pa[5] * c2;
            const double a2 = pa[6] * c0 + pa[7] * c1 + pa[8] * c2;
            s[0] += sel ? a0 : 0.0; s[1] += sel ? a1 : 0.0; s[2] += sel ? a2 : 0.0;
        }
    }
    __device__ __forceinline__ void scan_backward_wave(double r[3], int lane_base) const {
        const int tfull = (N - 1) / CH;
        double pa[9], pb[9];
        load9(L.phi, clane() < L.TP ? clane() : tfull, pa);
#define PO_BWD_LEVEL(LVL, PC, PN) \
        { \
            const int e_ = LVL < 3 ? clane() + (2 << LVL) - 1 : clane(); \
            load9(L.phi + (LVL < 3 ? LVL + 1 : 5) * 9 * L.TP, e_ < L.TP ? e_ : tfull, PN); \
            const double o0 = dpp_mov0<kDppRowShl + (1 << LVL)>(r[0]), o1 = dpp_mov0<kDppRowShl + (1 << LVL)>(r[1]), o2 = dpp_mov0<kDppRowShl + (1 << LVL)>(r[2]); \
            r[0] += PC[0] * o0 + PC[3] * o1 + PC[6] * o2; \
            r[1] += PC[1] * o0 + PC[4] * o1 + PC[7] * o2; \
            r[2] += PC[2] * o0 + PC[5] * o1 + PC[8] * o2; \
        }
        PO_BWD_LEVEL(0, pa, pb) PO_BWD_LEVEL(1, pb, pa) PO_BWD_LEVEL(2, pa, pb) PO_BWD_LEVEL(3, pb, pa)
#undef PO_BWD_LEVEL
        const int rlast = tfull >> 4;
        const int row = clane() >> 4;
        for (int rr = rlast - 1; rr >= 0; --rr) {
            const bool sel = row == rr;
            const double c0 = bcast(r[0], lane_base + 16 * (rr + 1)), c1 = bcast(r[1], lane_base + 16 * (rr + 1)), c2 = bcast(r[2], lane_base + 16 * (rr + 1));
            const double a0 = pa[0] * c0 + pa[3] * c1 + pa[6] * c2;
            const double a1 = pa[1] * c0 + pa[4] * c1 + pa[7] * c2;
            const double a2 = pa[2] * c0 + pa[5] * c1 + pa[8] * c2;
            r[0] += sel ? a0 : 0.0; r[1] += sel ? a1 : 0.0; r[2] += sel ? a2 : 0.0;
        }
    }
    static constexpr int kLaneB = (NW == 2 && NT == 64) ? 32 : 0;  // wave lane of role B's chunk 0 (NT = 128: role B is a wave of its own)
    // The linear solve of one iteration, role-split mapping.  In: st.bx = rhs of the own stages, st.bxu[0] = this lane's share of the control's rhs (the owner's includes the
    // control's own rows).  Out: st.bx = solution at the own stages, st.bxu[0] = the own chunk's control (both roles), st.bnext = solution at the next stage,
    // st.bprev = (solution at the previous stage, control of the transition into the own first stage).
    __device__ __forceinline__ void solve_split(LS &st, double rho) const {
        const double rho_eq = eq_step(rho);
        double re[T::NDYN];
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) re[r] = eq_row_step(rho_eq, r);
        const int tfull = (N - 1) / CH;
        const bool fullc = nq_chunk() == CH;
        const double zero3[3] = {0, 0, 0};
        double fu[4];
        load_fu(fu);
        double s[3], yu, t4[4];
        // F1: outflow of every full chunk with zero inflow; F2: forward scan of the chunk outflows on the role-B lanes, handed to role A of the next chunk
        split_forward<0>(st, zero3, s, yu, re, fu);
        if (wrole() == 1) {
            if (!fullc) s[0] = s[1] = s[2] = 0.0;
            scan_forward_wave(s, kLaneB);
            t4[0] = s[0]; t4[1] = s[1]; t4[2] = s[2]; t4[3] = 0;
            hx_put(L.hx1, t4);
        }
        __syncthreads();
        double yin[3] = {0, 0, 0};
        if (wrole() == 0) { hx_get(L.hx1, clane() - 1, t4); yin[0] = t4[0]; yin[1] = t4[1]; yin[2] = t4[2]; }
        // F3: true forward (stores z = D^-1 L^-1 rhs)
        split_forward<1>(st, yin, s, yu, re, fu);
        if (wrole() == own_role()) st.bxu[0] = nq_chunk() > 0 ? yu * fu[0] : 0.0;
        // B1: backward with zero inflow (the chunk that holds the final stage: its true solution); B2: suffix scan on the role-A lanes, handed to role B
        double r[3], xn[3];
        split_backward<false>(st, zero3, r, xn, re, fu);
        if (wrole() == 0) {
            if (clane() > tfull) r[0] = r[1] = r[2] = 0.0;
            scan_backward_wave(r, 0);
            t4[0] = r[0]; t4[1] = r[1]; t4[2] = r[2]; t4[3] = 0;
            hx_put(L.hx0, t4);
        }
        __syncthreads();
        double xin[3] = {0, 0, 0};
        if (wrole() == 1) { hx_get(L.hx0, clane() + 1, t4); xin[0] = t4[0]; xin[1] = t4[1]; xin[2] = t4[2]; st.bnext[0] = xin[0]; st.bnext[1] = xin[1]; st.bnext[2] = xin[2]; }
        // (slot 0 is rewritten by role B inside the next sweep: by the lanes that have just read it, in program order)
        // B3: true backward; role B posts (its last stage, control) for role A of the next chunk on the way
        split_backward<true>(st, xin, r, xn, re, fu);
        if (wrole() == 0) {
            st.bnext[0] = xn[0]; st.bnext[1] = xn[1]; st.bnext[2] = xn[2];
            hx_get(L.hx0, clane() - 1, st.bprev);                         // previous chunk's last stage + its control
            const double mine[4] = {st.bx[SPL - 1][0], st.bx[SPL - 1][1], st.bx[SPL - 1][2], 0.0};
            hx_put(L.hx1, mine);                                     // own last stage, for role B of the same chunk
        }
        __syncthreads();
        if (wrole() == 1) { hx_get(L.hx1, clane(), st.bprev); st.bprev[3] = st.bxu[0]; }
    }

// ==================== [two_rhs] ====================
// members of Fast, part 7: the right-hand side pass of the two-level mapping, and the vote on uniform row classes.  TWO only, every NWX.
//   rhs_pass_two<UNI, FIRST, POL, NWT>   the first of an iteration's three passes: sigma x + A' rho (2 clip(v) - v) per own stage and control, slacks eliminated (gs / gsu
//                                        keep the slacks' part for update_pass_two).  POL: rows of the polish's active set; NWT: minus the gradient (Newton direction)
//   classify                             are the row classes of the bounds one pattern on every lane?  Sets pat_loc / pat_ctl / pat_last (the only non-const member)
//   LDS     rhs_pass_two reads rrb (UNI: row steps, uhi / uhv) and uses the xchg mailboxes at ex (NT > 64); classify votes through the first words at S (NT > 64), which
//           the kernel zeroes afterwards
//   lanes   reads x, u, su, every v, cls* (general variant), pc* (POL), hi / hv / hiu / hus (general variant); writes bx, bxu, gs, gsu and, NW 1, bnext (the next chunk's
//           first right-hand side; role-split: the receiver adds its own, and the other role's share of the control's rhs rides in bxu[0])
//   called  rhs_pass_two by admm_loop (every iteration), refine_phase_newton (<.., NWT>, every step) and polish_kernel (<.., POL>); classify once, by solve_body right
//           after load(), to choose between the UNI kernel and deferring the path to the general one
    // UNI: all lanes share the row-class patterns (pat_loc / pat_ctl, set by classify()); FIRST: cold-start iteration.
    // NWT (Newton refinement, refine = 2; general variant only): the right-hand side is MINUS THE GRADIENT of the augmented Lagrangian at (x, v = a.x + y / rho),
    //   -g = -(P x + A' rho (v - clip(v))),   so that the solve returns the Newton direction: "2 clip(v) - v" -> "clip(v) - v", "sigma x" -> "-P x".
    template <bool UNI, bool FIRST, bool POL = false, bool NWT = false> __device__ __forceinline__ void rhs_pass_two(LS &st, double rho) const {
        static_assert(!NWT || (!UNI && !FIRST && !POL), "Newton right-hand side: general variant");
        const double rho_eq = eq_step(rho);
        double tku[NG];  // the dynamics rows' part of the controls' right-hand sides, per group of the lane
#pragma unroll
        for (int g = 0; g < NG; ++g) tku[g] = 0;
        double re[T::NDYN];
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) re[r] = eq_row_step(rho_eq, r);
        const double tgt = NWT ? 1.0 : 2.0;  // target of an equality row: 2 b - v (ADMM) / b - v (Newton)
        double nwp[2] = {0, 0}, nwn = 0;     // K, Newton: steering of the neighbouring stages (tridiagonal R block of P)
        if constexpr (NWT && F == F_K) {
            double xl[4] = {0, 0, 0, 0}, pl[4], xf[3] = {st.x[0][0], st.x[0][1], st.x[0][2]}, nf[3];
            const int nst_ = nst_own();
#pragma unroll
            for (int q = 0; q < SPL; ++q) if (q == nst_ - 1) { xl[0] = st.x[q][0]; xl[1] = st.x[q][1]; xl[2] = st.x[q][2]; }
            xchg<4>(xl, -1, pl, 0);
            xchg<3>(xf, +1, nf, 1);
            nwp[0] = pl[2]; nwn = nf[2];
        }
        RhsFnX<UNI, FIRST, T::NLOC, NWT> fn0;
        fn0.rho = rho; fn0.rho_eq = rho_eq; fn0.W = Wloc(); fn0.cls = 0; fn0.stride = 1; fn0.v = nullptr;
        if constexpr (UNI) {
#pragma unroll
            for (int r = 0; r < T::NLOC; ++r) fn0.rr[r] = S[L.rrb + r];
        }
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            RhsFnX<UNI, FIRST, T::NLOC, NWT> fn = fn0;
            fn.cls = UNI ? 0u : st.cls[q];
            if constexpr (F == F_K) {
                fn.W = Wloc(j);
                if constexpr (UNI) { if (k_end(j)) fn.rr[2] = k_rr2_end(); if (si.last) fn.rr[0] = k_rr0_last(); }
            }
            if constexpr (F == F_KPC && UNI) { if (kpc_c3(st, q)) fn.rr[3] = S[L.rrb + 15]; }
            if constexpr (NWT) {
                fn.g[0] = -(p_diag_node<F>(0, j, N, P) * st.x[q][0]); fn.g[1] = 0.0; fn.g[2] = -(p_diag_node<F>(2, j, N, P) * st.x[q][2]);
                fn.g[3] = T::NS > 0 ? -(P.w_s1 * st.x[q][3 < 3 + T::NS ? 3 : 0]) : 0.0;
                fn.g[4] = T::NS > 1 ? -(P.w_s2 * st.x[q][4 < 3 + T::NS ? 4 : 0]) : 0.0;
                if constexpr (F == F_K) {
                    if (j <= N - 2) {
                        if (j >= 1) fn.g[2] += P.w_cr * (q > 0 ? st.x[q > 0 ? q - 1 : 0][2] : nwp[0]);
                        if (j + 1 <= N - 2) fn.g[2] += P.w_cr * (q + 1 < SPL ? st.x[q + 1 < SPL ? q + 1 : q][2] : nwn);
                    }
                }
            } else {
#pragma unroll
                for (int a = 0; a < 5; ++a) fn.g[a] = a < 3 + T::NS ? sig(a, j) * st.x[q][a] : 0.0;
            }
            fn.v = st.vl[q]; fn.stride = 1;
            if constexpr (POL) { PolWrap<RhsFnX<UNI, FIRST, T::NLOC>> w{fn, st.pc[q]}; local_rows<F>(si, P, w); } else local_rows<F>(si, P, fn);
            if (T::NEND && si.last) {
                RhsFnX<false, FIRST, 1, NWT> fe;
                fe.rho = rho; fe.rho_eq = rho_eq; fe.W = Wend(); fe.cls = st.clse; fe.v = st.vend; fe.stride = 1;
#pragma unroll
                for (int a = 0; a < 5; ++a) fe.g[a] = fn.g[a];
                if constexpr (POL) { PolWrap<RhsFnX<false, FIRST, 1>> w{fe, st.pce}; end_rows<F>(si, P, w); } else end_rows<F>(si, P, fe);
#pragma unroll
                for (int a = 0; a < 5; ++a) fn.g[a] = fe.g[a];
            }
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) { const double t = FIRST ? 0.0 : re[r] * (tgt * st.bin0[r] - st.vd[q][r]); fn.g[dyn_tau<F>(r)] -= t; }
            } else {
                const Dyn<F> d = dyn_in(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double t = FIRST ? 0.0 : re[r] * (tgt * d.b[r] - st.vd[q][r]);
                    fn.g[dyn_tau<F>(r)] -= t;
                    if (in_own_group(q)) tku[gIn(q)] += t * d.beta[r];
                }
            }
            if (j < N - 1) {
                const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double vv = q + 1 < SPL ? st.vd[q + 1 < SPL ? q + 1 : q][r] : st.vdo[r];
                    const double t = FIRST ? 0.0 : re[r] * (tgt * d.b[r] - vv);
                    fn.g[0] += t * d.f[r][0]; fn.g[1] += t * d.f[r][1]; fn.g[2] += t * d.f[r][2];
                    if (q == SPL - 1 && out_own_group(q)) tku[NG - 1] += t * d.beta[r];
                }
            }
#pragma unroll
            for (int s = 0; s < T::NS; ++s) {
                const double hi_ = UNI ? uhi_at(s, st, q) : st.hi[q][s];
                const double w = fn.g[3 + s] * hi_;
                fn.g[0] -= (UNI ? uhv(s, 0) : st.hv[q][s][0]) * w; fn.g[1] -= (UNI ? uhv(s, 1) : st.hv[q][s][1]) * w; fn.g[2] -= (UNI ? uhv(s, 2) : st.hv[q][s][2]) * w;
                st.gs[q][s] = fn.g[3 + s];
            }
            st.bx[q][0] = fn.g[0]; st.bx[q][1] = fn.g[1]; st.bx[q][2] = fn.g[2];
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) st.bxu[g] = 0;
        if constexpr (NW == 2) { if (!has_ctl()) st.bxu[0] = tku[0]; }  // the other role's share of the control's rhs travels with the forward hand-off (split_forward)
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (has_ctl(g)) {
                    RhsFnX<UNI, FIRST, T::NCTL, NWT> fn;
                    fn.rho = rho; fn.rho_eq = rho_eq; fn.W = Wctl(); fn.cls = st.clsc;
                    if constexpr (UNI) {
#pragma unroll
                        for (int r = 0; r < T::NCTL; ++r) fn.rr[r] = S[L.rrb + 9 + r];
                    }
                    fn.g[0] = fn.g[1] = fn.g[4] = 0;
                    fn.g[2] = (NWT ? -(P.w_u * st.u[g]) : sig(5) * st.u[g]) + tku[g];
                    fn.g[3] = T::HAS_SU ? (NWT ? -(P.w_su * st.su) : sig(6) * st.su) : 0.0;
                    fn.v = st.vc[g]; fn.stride = 1;
                    if constexpr (POL) { PolWrap<RhsFnX<UNI, FIRST, T::NCTL>> w{fn, st.pcc}; ctl_rows<F>(st.mkp, w); } else ctl_rows<F>(st.mkp, fn);
                    if constexpr (T::HAS_SU) { fn.g[2] -= st.hus * fn.g[3] * st.hiu; st.gsu = fn.g[3]; }
                    st.bxu[g] = fn.g[2];
                }
            }
        }
        // rhs of the next chunk's first stage (needed by the last own transition); the stage-split mapping lets the receiver add its own rhs
        if constexpr (NW == 1) xchg<3>(st.bx[0], +1, st.bnext, 0);
    }

    // Are the row-class patterns (fixed for the whole solve) the same on every lane that owns rows?
    __device__ __forceinline__ bool classify(const LS &st) {
        if constexpr (F == F_K) {
            // K: every stage but the last shares a pattern (the last one has the end-heading window on its e_phi row and no steering row); the end
            // stages' own Ruiz factors (k_end) change row steps, not classes.  One-wave blocks only (the last stage's pattern is read across lanes).
            if constexpr (NT != 64) return false;
            const unsigned p0k = (unsigned)__builtin_amdgcn_readfirstlane((int)st.cls[0]);
            bool samek = true;
            unsigned pl = 0;
#pragma unroll
            for (int q = 0; q < SPL; ++q) {
                if (stage(q) < N - 1 && st.cls[q] != p0k) samek = false;
                if (stage(q) == N - 1) pl = st.cls[q];
            }
            pat_loc = p0k; pat_ctl = 0;
            pat_last = (unsigned)__builtin_amdgcn_readlane((int)pl, (N - 1) / SPL);
            return __all(samek ? 1 : 0) != 0;
        }
        unsigned p0 = 0, pc = 0;
        bool same = true;
        p0 = (unsigned)__builtin_amdgcn_readfirstlane((int)st.cls[0]);
        pc = (unsigned)__builtin_amdgcn_readfirstlane((int)st.clsc);
        const unsigned keep_ = F == F_KPC ? ~kKpcRow3 : ~0u;  // KPC: row 3 may differ from stage to stage (cls_of)
        p0 &= keep_;
#pragma unroll
        for (int q = 0; q < SPL; ++q) if (stage(q) < N && (st.cls[q] & keep_) != p0) same = false;
        if (T::HAS_U && (NW == 1 ? cidx(0) < C : has_ctl()) && st.clsc != pc) same = false;
        pat_loc = p0; pat_ctl = pc;
        if constexpr (NT > 64) {
            // block-wide AND through the (still unused) dynamic LDS: __syncthreads_and() would add 256 B of STATIC LDS to the kernel, which is what
            // separates 2 x 81.7 KB (KPC, N = 400) from the 160 KB of a CU
            const bool wave_ok = __all(same ? 1 : 0) != 0;
            if ((tid & 63) == 0) { S[tid >> 6] = wave_ok ? 1.0 : 0.0; if constexpr (NW == 2) { S[4 + (tid >> 6)] = (double)p0; S[6 + (tid >> 6)] = (double)pc; } }
            __syncthreads();
            bool all_ok = true;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) all_ok = all_ok && S[w] != 0.0;
            if constexpr (NW == 2) {  // both waves must have found the same stage pattern; the control pattern is the owner wave's
                all_ok = all_ok && S[4] == S[5];
                pat_ctl = (unsigned)S[7];
            }
            __syncthreads();  // before anybody zeroes the block's LDS
            return all_ok;
        } else return __all(same ? 1 : 0) != 0;
    }

// ==================== [two_solve] ====================
// members of Fast, part 8: solve_two, the linear solve of one iteration on the two-level mapping with ONE LANE PER CHUNK (NW 1: NWX 1, 4, 5; the
// role-split mapping runs solve_split, [two_sweeps]).  TWO only.  Five phases, the PO_TICK buckets and PO_MARK labels: F1 every chunk's outflow with zero inflow
// (sweep_forward<0>), F2 forward scan of the chunk boundaries s_t = beta_t + Phi_t s_{t-1}, F3 the true forward sweep and B1 the backward sweep with zero inflow, B2
// the suffix scan X_t = gamma_t + Phi_t' X_{t+1}, B3 the true backward sweep.  The scans: one wave — DPP row shifts inside rows of 16 lanes, row totals through
// v_readlane, no barrier; SEG (NT > 64) — 8-lane segments on DPP, segment totals through LDS with the scan's one barrier, carried back through in-wave permutes.
//   LDS     reads fac, facu, phi (levels 0..5 / SEG 0..4), rseg; writes mail (SEG: segment totals, forward [0], backward [1]) and, NT > 64, the xchg mailboxes at ex
//   lanes   in: st.bx, st.bxu, st.bnext (rhs_pass_two); out: st.bx, st.bxu = the solution at the own stages / controls, st.bnext = the next chunk's first stage,
//           st.bprev = the previous chunk's last stage and its last control
//   called  once per iteration by admm_loop, once per Newton step by refine_phase_newton ([loops]), and by polish_kernel; ph_: cycles per phase (dev) or nullptr
// PO_TICK is local to solve_two and #undef'd at its end.
    __device__ __forceinline__ void solve_two(LS &st, double rho, long long *ph_) const {
        const bool prof = ph_ != nullptr;
        long long tt = prof ? __builtin_readcyclecounter() : 0;
#define PO_TICK(i) if (prof) { const long long n_ = __builtin_readcyclecounter(); ph_[i] += n_ - tt; tt = n_; }
        const double rho_eq = eq_step(rho);
        double re[T::NDYN];
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) re[r] = eq_row_step(rho_eq, r);
        const int nq = nq_own(), nst = nst_own();
        const bool full = (nq == SPL);
        double fu[NG][4];  // own controls' factor entries, one read per solve
#pragma unroll
        for (int g = 0; g < NG; ++g) { fu[g][0] = fu[g][1] = fu[g][2] = fu[g][3] = 0; if constexpr (T::HAS_U) { fu[g][0] = FUg(g, 0); fu[g][1] = FUg(g, 1); fu[g][2] = FUg(g, 2); fu[g][3] = FUg(g, 3); } }
        const int tfull = (N - 1) / SPL;  // chunks 0..tfull-1 are full, chunk tfull holds the final stage
        // ---- F1: outflow of every full chunk with zero inflow (chunk 0: its true inflow b_0) ----
        double s[3] = {0, 0, 0};
        {   // every lane runs the sweep (no divergence); only full chunks' results are used
            if (tid == 0) { s[0] = st.bx[0][0]; s[1] = st.bx[0][1]; s[2] = st.bx[0][2]; }
            double acc[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = st.bxu[g];
            sweep_forward<0>(st, s, nq, acc, re, fu);
        }
        PO_TICK(0) PO_MARK("F2");
        // ---- F2: scan of the chunk boundaries  s_t = beta_t + Phi_t s_{t-1} ----
        int buf = 1;
        double yin[3];
        if constexpr (SEG) {
            const int lw = tid & 63, sl = tid & 7, nsg = (L.TP + 7) >> 3;
            const int tp_ = tid < L.TP ? tid : 0;
            // (a) inside 8-lane segments: Kogge-Stone on in-wave permutes, no barrier
            // (DPP row shifts: the 8-lane segments are halves of the 16-lane DPP rows; what crosses a segment boundary is masked by `on`)
#define PO_SEG_FWD(LVL) \
            { \
                double p[9]; \
                load9(L.phi + LVL * 9 * L.TP, tp_, p); \
                const double o0 = dpp_mov0<kDppRowShr + (1 << LVL)>(s[0]), o1 = dpp_mov0<kDppRowShr + (1 << LVL)>(s[1]), o2 = dpp_mov0<kDppRowShr + (1 << LVL)>(s[2]); \
                const bool on = sl >= (1 << LVL) && tid < tfull; \
                const double a0 = p[0] * o0 + p[1] * o1 + p[2] * o2; \
                const double a1 = p[3] * o0 + p[4] * o1 + p[5] * o2; \
                const double a2 = p[6] * o0 + p[7] * o1 + p[8] * o2; \
                s[0] += on ? a0 : 0.0; s[1] += on ? a1 : 0.0; s[2] += on ? a2 : 0.0; \
            }
            PO_SEG_FWD(0) PO_SEG_FWD(1) PO_SEG_FWD(2)
#undef PO_SEG_FWD
            // (b) segment totals through LDS (the only barrier), scanned redundantly by lanes 0..15 of every wave
            double *mb = S + L.mail;
            if (sl == 7 && tid < L.TP) { const bool v = tid < tfull; mb[(tid >> 3) * 3] = v ? s[0] : 0.0; mb[(tid >> 3) * 3 + 1] = v ? s[1] : 0.0; mb[(tid >> 3) * 3 + 2] = v ? s[2] : 0.0; }
            __syncthreads();
            double sg[3] = {0, 0, 0};
            if (lw < nsg && lw * 8 + 7 < L.TP) { sg[0] = mb[lw * 3]; sg[1] = mb[lw * 3 + 1]; sg[2] = mb[lw * 3 + 2]; }
            const int nl2 = nsg > 16 ? 5 : (nsg > 8 ? 4 : (nsg > 4 ? 3 : (nsg > 2 ? 2 : (nsg > 1 ? 1 : 0))));
            if constexpr (NT == 128) {  // <= 16 segment totals: one DPP row
#define PO_SEG_FWD2(LVL) \
                if (LVL < nl2) { \
                    double p[9]; \
                    const int g_ = lw < nsg ? lw : 0; \
                    _Pragma("unroll") for (int i = 0; i < 9; ++i) p[i] = RS(LVL, g_, i); \
                    const double o0 = dpp_mov0<kDppRowShr + (1 << LVL)>(sg[0]), o1 = dpp_mov0<kDppRowShr + (1 << LVL)>(sg[1]), o2 = dpp_mov0<kDppRowShr + (1 << LVL)>(sg[2]); \
                    const bool on = lw >= (1 << LVL) && lw < nsg && lw * 8 + 7 < tfull; \
                    const double a0 = p[0] * o0 + p[1] * o1 + p[2] * o2; \
                    const double a1 = p[3] * o0 + p[4] * o1 + p[5] * o2; \
                    const double a2 = p[6] * o0 + p[7] * o1 + p[8] * o2; \
                    sg[0] += on ? a0 : 0.0; sg[1] += on ? a1 : 0.0; sg[2] += on ? a2 : 0.0; \
                }
                PO_SEG_FWD2(0) PO_SEG_FWD2(1) PO_SEG_FWD2(2) PO_SEG_FWD2(3)
#undef PO_SEG_FWD2
            } else {
            for (int lvl = 0; lvl < nl2; ++lvl) {
                const int dd = 1 << lvl;
                double o[3], p[9];
                const int g_ = lw < nsg ? lw : 0;
#pragma unroll
                for (int i = 0; i < 9; ++i) p[i] = RS(lvl, g_, i);
                wshfl<3>(sg, lw - dd, o);
                const bool on = lw >= dd && lw < nsg && lw * 8 + 7 < tfull;
                const double a0 = p[0] * o[0] + p[1] * o[1] + p[2] * o[2];
                const double a1 = p[3] * o[0] + p[4] * o[1] + p[5] * o[2];
                const double a2 = p[6] * o[0] + p[7] * o[1] + p[8] * o[2];
                sg[0] += on ? a0 : 0.0; sg[1] += on ? a1 : 0.0; sg[2] += on ? a2 : 0.0;
            }
            }
            // (c) carry of the previous segment into every lane: s_t += Q^incl_t S_{g-1}
            {
                const int g = tid >> 3;
                double c[3], p[9];
                wshfl<3>(sg, g > 0 ? g - 1 : 0, c);
                load9(L.phi + 3 * 9 * L.TP, tp_, p);
                const bool on = g > 0 && tid < tfull;
                const double a0 = p[0] * c[0] + p[1] * c[1] + p[2] * c[2];
                const double a1 = p[3] * c[0] + p[4] * c[1] + p[5] * c[2];
                const double a2 = p[6] * c[0] + p[7] * c[1] + p[8] * c[2];
                s[0] += on ? a0 : 0.0; s[1] += on ? a1 : 0.0; s[2] += on ? a2 : 0.0;
            }
            // inflow of chunk t = outflow of chunk t - 1: a DPP wave shift inside the wave; lane 0 of wave w > 0 takes the inclusive total of
            // segment 8 w - 1, which every wave holds in its own copy of the segment scan (no LDS round trip, no barrier)
            {
                const int wv = __builtin_amdgcn_readfirstlane(tid) >> 6;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double c = bcast(sg[k], wv > 0 ? 8 * wv - 1 : 0);
                    yin[k] = dpp_mov<kDppWaveShr1>(s[k], s[k]);
                    if (lw == 0 && wv > 0) yin[k] = c;
                }
            }
        } else {
            // one wave: Kogge-Stone inside rows of 16 lanes on DPP row shifts (VALU latency instead of an LDS round trip per level), then the
            // row totals carried from row to row through readlane broadcasts.  No predicates: lanes without a source get o = 0, entries of
            // chunks that are not full are zero (entry tfull always is), see factor_chain_two.  (twin: scan_forward_wave, [two_sweeps])
            const int tp_ = tid < L.TP ? tid : tfull;
            // straight-line code, the table of level l + 1 requested before level l is computed (its load does not depend on s)
            double pa[9], pb[9];
            load9(L.phi, tp_, pa);
#define PO_FWD_LEVEL(LVL, PC, PN) \
            { \
                load9(L.phi + (LVL + 1) * 9 * L.TP, tp_, PN); \
                const double o0 = dpp_mov0<kDppRowShr + (1 << LVL)>(s[0]), o1 = dpp_mov0<kDppRowShr + (1 << LVL)>(s[1]), o2 = dpp_mov0<kDppRowShr + (1 << LVL)>(s[2]); \
                s[0] += PC[0] * o0 + PC[1] * o1 + PC[2] * o2; \
                s[1] += PC[3] * o0 + PC[4] * o1 + PC[5] * o2; \
                s[2] += PC[6] * o0 + PC[7] * o1 + PC[8] * o2; \
            }
            PO_FWD_LEVEL(0, pa, pb) PO_FWD_LEVEL(1, pb, pa) PO_FWD_LEVEL(2, pa, pb) PO_FWD_LEVEL(3, pb, pa)  // pa ends up holding level 4 = Q^incl
#undef PO_FWD_LEVEL
            const int nrow = (L.TP + 15) >> 4;
            if (nrow > 1) {
                const double *p = pa;
                const int row = tid >> 4;
                for (int r = 1; r < nrow; ++r) {  // s_t += Q^incl_t s_{16 r - 1} for the lanes of row r (row r - 1 is final by now)
                    const bool sel = row == r;
                    const double c0 = bcast(s[0], 16 * r - 1), c1 = bcast(s[1], 16 * r - 1), c2 = bcast(s[2], 16 * r - 1);
                    const double a0 = p[0] * c0 + p[1] * c1 + p[2] * c2;
                    const double a1 = p[3] * c0 + p[4] * c1 + p[5] * c2;
                    const double a2 = p[6] * c0 + p[7] * c1 + p[8] * c2;
                    s[0] += sel ? a0 : 0.0; s[1] += sel ? a1 : 0.0; s[2] += sel ? a2 : 0.0;
                }
            }
        }
        if constexpr (!SEG) xchg<3>(s, -1, yin, buf);  // inflow of chunk t = outflow of chunk t-1
        buf ^= 1;
        if (tid == 0) { yin[0] = st.bx[0][0]; yin[1] = st.bx[0][1]; yin[2] = st.bx[0][2]; }
        PO_TICK(1) PO_MARK("F3B1");
        // ---- F3: true local forward (stores z = D^-1 y), then B1: backward with zero inflow ----
        double r[3] = {0, 0, 0}, zlast[3] = {0, 0, 0};
        {
            double acc[NG], y[3] = {yin[0], yin[1], yin[2]};
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = st.bxu[g];
            sweep_forward<1>(st, y, nq, acc, re, fu);
            // the own stage after the last transition (only in the chunk holding the final stage): z = Ginv y
#pragma unroll
            for (int q = 0; q < SPL; ++q)
                if (q == nq && q < nst) { mul_G(q, y, zlast); st.bx[q][0] = zlast[0]; st.bx[q][1] = zlast[1]; st.bx[q][2] = zlast[2]; }
            if constexpr (T::HAS_U) {
#pragma unroll
                for (int g = 0; g < NG; ++g) st.bxu[g] = g * GK < nq ? acc[g] * fu[g][0] : 0.0;  // (a group of the lane without a transition has no control)
            }
            // B1 on every lane without storing: full chunks get gamma_t (zero inflow), the final chunk its true X
            r[0] = zlast[0]; r[1] = zlast[1]; r[2] = zlast[2];  // zero for full chunks
            sweep_backward<false>(st, r, nq, re, fu);
        }
        PO_TICK(2) PO_MARK("B2");
        // ---- B2: suffix scan of the chunk boundaries  X_t = gamma_t + Phi_t' X_{t+1} ----
        if constexpr (SEG) {
            const int lw = tid & 63, sl = tid & 7, nsg = (L.TP + 7) >> 3;
            const int glast = tfull >> 3;  // segment of the chunk that holds the final stage (its true X)
#define PO_SEG_BWD(LVL) \
            { \
                double p[9]; \
                const bool on = sl + (1 << LVL) <= 7 && tid + (1 << LVL) <= tfull; \
                const int tp_ = on ? tid + (1 << LVL) - 1 : 0; \
                load9(L.phi + LVL * 9 * L.TP, tp_, p); \
                const double o0 = dpp_mov0<kDppRowShl + (1 << LVL)>(r[0]), o1 = dpp_mov0<kDppRowShl + (1 << LVL)>(r[1]), o2 = dpp_mov0<kDppRowShl + (1 << LVL)>(r[2]); \
                const double a0 = p[0] * o0 + p[3] * o1 + p[6] * o2; \
                const double a1 = p[1] * o0 + p[4] * o1 + p[7] * o2; \
                const double a2 = p[2] * o0 + p[5] * o1 + p[8] * o2; \
                r[0] += on ? a0 : 0.0; r[1] += on ? a1 : 0.0; r[2] += on ? a2 : 0.0; \
            }
            PO_SEG_BWD(0) PO_SEG_BWD(1) PO_SEG_BWD(2)
#undef PO_SEG_BWD
            double *mb = S + L.mail + 3 * L.nsm;
            if (sl == 0 && tid < L.TP) { const bool v = tid <= tfull; mb[(tid >> 3) * 3] = v ? r[0] : 0.0; mb[(tid >> 3) * 3 + 1] = v ? r[1] : 0.0; mb[(tid >> 3) * 3 + 2] = v ? r[2] : 0.0; }
            __syncthreads();
            double sg[3] = {0, 0, 0};
            if (lw < nsg) { sg[0] = mb[lw * 3]; sg[1] = mb[lw * 3 + 1]; sg[2] = mb[lw * 3 + 2]; }
            const int nl2 = nsg > 16 ? 5 : (nsg > 8 ? 4 : (nsg > 4 ? 3 : (nsg > 2 ? 2 : (nsg > 1 ? 1 : 0))));
            if constexpr (NT == 128) {  // X_{8g} = A_g + R_g' X_{8(g+1)}; <= 16 segments: one DPP row
#define PO_SEG_BWD2(LVL) \
                if (LVL < nl2) { \
                    double p[9]; \
                    const bool on = lw + (1 << LVL) <= glast; \
                    const int g_ = on ? lw + (1 << LVL) - 1 : 0; \
                    _Pragma("unroll") for (int i = 0; i < 9; ++i) p[i] = RS(LVL, g_, i); \
                    const double o0 = dpp_mov0<kDppRowShl + (1 << LVL)>(sg[0]), o1 = dpp_mov0<kDppRowShl + (1 << LVL)>(sg[1]), o2 = dpp_mov0<kDppRowShl + (1 << LVL)>(sg[2]); \
                    const double a0 = p[0] * o0 + p[3] * o1 + p[6] * o2; \
                    const double a1 = p[1] * o0 + p[4] * o1 + p[7] * o2; \
                    const double a2 = p[2] * o0 + p[5] * o1 + p[8] * o2; \
                    sg[0] += on ? a0 : 0.0; sg[1] += on ? a1 : 0.0; sg[2] += on ? a2 : 0.0; \
                }
                PO_SEG_BWD2(0) PO_SEG_BWD2(1) PO_SEG_BWD2(2) PO_SEG_BWD2(3)
#undef PO_SEG_BWD2
            } else {
            for (int lvl = 0; lvl < nl2; ++lvl) {  // X_{8g} = A_g + R_g' X_{8(g+1)}
                const int dd = 1 << lvl;
                double o[3], p[9];
                const bool on = lw + dd <= glast;
                const int g_ = on ? lw + dd - 1 : 0;
#pragma unroll
                for (int i = 0; i < 9; ++i) p[i] = RS(lvl, g_, i);
                wshfl<3>(sg, lw + dd, o);
                const double a0 = p[0] * o[0] + p[3] * o[1] + p[6] * o[2];
                const double a1 = p[1] * o[0] + p[4] * o[1] + p[7] * o[2];
                const double a2 = p[2] * o[0] + p[5] * o[1] + p[8] * o[2];
                sg[0] += on ? a0 : 0.0; sg[1] += on ? a1 : 0.0; sg[2] += on ? a2 : 0.0;
            }
            }
            {   // carry of the next segment into every lane: X_t += (Q^suf_t)' X_{8(g+1)}
                const int g = tid >> 3;
                double c[3], p[9];
                wshfl<3>(sg, g + 1 < 64 ? g + 1 : 0, c);
                const bool on = g < glast && tid < L.TP;
                load9(L.phi + 4 * 9 * L.TP, on ? tid : 0, p);
                const double a0 = p[0] * c[0] + p[3] * c[1] + p[6] * c[2];
                const double a1 = p[1] * c[0] + p[4] * c[1] + p[7] * c[2];
                const double a2 = p[2] * c[0] + p[5] * c[1] + p[8] * c[2];
                r[0] += on ? a0 : 0.0; r[1] += on ? a1 : 0.0; r[2] += on ? a2 : 0.0;
            }
            // X_{t+1} for every lane: wave shift; lane 63 of wave w takes X at the first lane of segment 8 (w + 1) from the segment scan
            {
                const int wv = __builtin_amdgcn_readfirstlane(tid) >> 6;
                const bool more = 64 * (wv + 1) < L.TP;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double c = bcast(sg[k], more ? 8 * (wv + 1) : 0);
                    st.bnext[k] = dpp_mov<kDppWaveShl1>(r[k], r[k]);
                    if (lw == 63 && more) st.bnext[k] = c;
                }
            }
        } else {
            // suffix scan, same structure: DPP row shifts to the left inside the rows, then the first lane of row r + 1 carried into row r  (twin: scan_backward_wave)
            double pa[9], pb[9];
            load9(L.phi, tid < L.TP ? tid : tfull, pa);
#define PO_BWD_LEVEL(LVL, PC, PN) \
            { \
                const int e_ = LVL < 3 ? tid + (2 << LVL) - 1 : tid;  /* next level's entry; after level 3: Q^suf of the own lane */ \
                load9(L.phi + (LVL < 3 ? LVL + 1 : 5) * 9 * L.TP, e_ < L.TP ? e_ : tfull, PN); \
                const double o0 = dpp_mov0<kDppRowShl + (1 << LVL)>(r[0]), o1 = dpp_mov0<kDppRowShl + (1 << LVL)>(r[1]), o2 = dpp_mov0<kDppRowShl + (1 << LVL)>(r[2]); \
                r[0] += PC[0] * o0 + PC[3] * o1 + PC[6] * o2; \
                r[1] += PC[1] * o0 + PC[4] * o1 + PC[7] * o2; \
                r[2] += PC[2] * o0 + PC[5] * o1 + PC[8] * o2; \
            }
            PO_BWD_LEVEL(0, pa, pb) PO_BWD_LEVEL(1, pb, pa) PO_BWD_LEVEL(2, pa, pb) PO_BWD_LEVEL(3, pb, pa)  // pa ends up holding Q^suf
#undef PO_BWD_LEVEL
            const int rlast = tfull >> 4;  // row of the chunk that holds the final stage (its true X)
            if (rlast > 0) {
                const double *p = pa;
                const int row = tid >> 4;
                for (int rr = rlast - 1; rr >= 0; --rr) {  // X_t += (Q^suf_t)' X_{16 (rr + 1)} for the lanes of row rr
                    const bool sel = row == rr;
                    const double c0 = bcast(r[0], 16 * (rr + 1)), c1 = bcast(r[1], 16 * (rr + 1)), c2 = bcast(r[2], 16 * (rr + 1));
                    const double a0 = p[0] * c0 + p[3] * c1 + p[6] * c2;
                    const double a1 = p[1] * c0 + p[4] * c1 + p[7] * c2;
                    const double a2 = p[2] * c0 + p[5] * c1 + p[8] * c2;
                    r[0] += sel ? a0 : 0.0; r[1] += sel ? a1 : 0.0; r[2] += sel ? a2 : 0.0;
                }
            }
        }
        if constexpr (!SEG) xchg<3>(r, +1, st.bnext, buf);  // X_{t+1}: inflow of the backward sweep, and the next chunk's first stage for the update
        buf ^= 1;
        PO_TICK(3) PO_MARK("B3");
        // ---- B3: true local backward on every lane (the final chunk re-runs from its own last stage) ----
        {
            double x[3] = {full ? st.bnext[0] : zlast[0], full ? st.bnext[1] : zlast[1], full ? st.bnext[2] : zlast[2]};
            sweep_backward<true>(st, x, nq, re, fu);
        }
        // previous chunk's last stage (+ its control) for the update of the rows into own stage 0
        double xl[4] = {0, 0, 0, st.bxu[NG - 1]};  // (the transition into the next lane's first stage belongs to this lane's last group)
#pragma unroll
        for (int q = 0; q < SPL; ++q) if (q == nst - 1) { xl[0] = st.bx[q][0]; xl[1] = st.bx[q][1]; xl[2] = st.bx[q][2]; }
        xchg<4>(xl, -1, st.bprev, buf);
        PO_TICK(4)
#undef PO_TICK
    }

// ==================== [two_update] ====================
// members of Fast, part 9: the row passes that FOLLOW a solve on the two-level mapping.  TWO only, every NWX.
//   update_pass_two<CERT, FIRST, UNI, POL>   the last of an iteration's three passes: slacks back-substituted from gs / gsu, then x, u, su and every v relaxed towards the
//                                            solve's result (alpha); CERT: also the ingredients of OSQP's infeasibility certificate (Cert, [single_level])
//   nbr_x<NEXT>                              x of the stages next to the own ones and the own chunk's control, for passes that run on the ITERATE (no solve just before)
//   residual_pass_two<UNI>                   primal / dual residuals and their norms, scaled and unscaled, objective, non-finite flag (Resid)
//   LDS     no table is read: what a pass needs from other lanes arrives in st.bnext / st.bprev (update) or through nbr_x — xchg (NW 1; mailboxes at ex when NT > 64) or
//           the hand-off slots hx0 / hx1 (role-split, two or four barriers); UNI reads rrb; the cross-wave reductions (NT > 64) go through ex
//   lanes   update_pass_two reads bx, bxu, bnext, bprev, gs, gsu, hi / hv (general variant) and writes x, u, su, vl, vd, vdo, vend, vc; residual_pass_two writes nothing
//   called  update_pass_two by admm_loop (every iteration) and polish_kernel (<.., POL>); residual_pass_two by admm_loop at the checks and by refine_phase_newton at every
//           step; nbr_x by residual_pass_two and nw_reexpress_pass ([newton_passes])
    // CERT: also evaluate the ingredients of OSQP's primal infeasibility certificate on this iteration's delta_y.
    // FIRST is the compile-time cold-start flag of the plain variant; the CERT variant (rare) takes it at run time.
    template <bool CERT, bool FIRST, bool UNI = false, bool POL = false> __device__ __forceinline__ Cert update_pass_two(LS &st, double rho, bool first_rt) const {
        static_assert(!(CERT && POL), "the polish never evaluates the infeasibility certificate");
        using UFn = typename std::conditional<CERT, UpdCertFn, UpdFnX<FIRST>>::type;
        const bool first = CERT ? first_rt : FIRST;
        const double al = P.alpha;
        const double rho_eq = eq_step(rho);
        Cert ct = {0, 0, 0};
        double re[T::NDYN], dy_next[T::NDYN], dytk[NG];  // dy of the rows into the stage processed just before (q+1); A' dy on the controls, per group of the lane
#pragma unroll
        for (int g = 0; g < NG; ++g) dytk[g] = 0;
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) { re[r] = eq_row_step(rho_eq, r); dy_next[r] = 0; }
#pragma unroll
        for (int q = SPL - 1; q >= 0; --q) {  // descending: the rows OUT of stage q are the rows INTO q+1, handled one step earlier
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            typename std::conditional<CERT, UpdCertFn, UpdFnX<FIRST>>::type fn;
            fn.alpha = al;
            if constexpr (CERT) fn.first = first;
            if constexpr (CERT) {
                fn.rho = rho; fn.rho_eq = rho_eq; fn.W = Wloc(j); fn.E = Eloc(j); fn.cls = cls_of<UNI>(st, q); fn.ndy = 0; fn.sup = 0;
#pragma unroll
                for (int a = 0; a < 5; ++a) fn.ady[a] = 0;
            }
            fn.xt[0] = st.bx[q][0]; fn.xt[1] = st.bx[q][1]; fn.xt[2] = st.bx[q][2];
            fn.xt[3] = fn.xt[4] = 0;
#pragma unroll
            for (int s = 0; s < T::NS; ++s)
                fn.xt[3 + s] = (st.gs[q][s] - ((UNI ? uhv(s, 0) : st.hv[q][s][0]) * fn.xt[0] + (UNI ? uhv(s, 1) : st.hv[q][s][1]) * fn.xt[1] + (UNI ? uhv(s, 2) : st.hv[q][s][2]) * fn.xt[2])) * (UNI ? uhi_at(s, st, q) : st.hi[q][s]);
            fn.v = st.vl[q]; fn.stride = 1;
            if constexpr (POL) { PolWrap<UFn> w{fn, st.pc[q]}; local_rows<F>(si, P, w); } else local_rows<F>(si, P, fn);
            if (T::NEND && si.last) {
                fn.v = st.vend;
                if constexpr (CERT) { fn.W = Wend(); fn.E = Eend(); fn.cls = st.clse; }
                if constexpr (POL) { PolWrap<UFn> w{fn, st.pce}; end_rows<F>(si, P, w); } else end_rows<F>(si, P, fn);
            }
            double dy_out[T::NDYN];  // rows out of stage q
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) dy_out[r] = dy_next[r];
            if (q == SPL - 1 && j < N - 1) {  // identical update of the copy of the next chunk's incoming rows
                const Dyn<F> d = dyn_out(st, q);
                const double ut = T::HAS_U ? st.bxu[NG - 1] : 0.0;
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double zt = d.f[r][0] * fn.xt[0] + d.f[r][1] * fn.xt[1] + d.f[r][2] * fn.xt[2] + d.beta[r] * ut - st.bnext[dyn_tau<F>(r)];
                    const double dv = al * (zt - (first ? 0.0 : d.b[r]));
                    st.vdo[r] += dv;
                    if (CERT) { dy_out[r] = re[r] * dv; if (out_own_group(q)) dytk[NG - 1] += dy_out[r] * d.beta[r]; }
                }
            }
            double dy_in[T::NDYN], bsum = 0;
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double dv = al * (-fn.xt[dyn_tau<F>(r)] - (first ? 0.0 : st.bin0[r]));
                    st.vd[q][r] += dv;
                    dy_in[r] = re[r] * dv; bsum += st.bin0[r] * dy_in[r];
                }
            } else {
                const Dyn<F> d = dyn_in(st, q);
                const double p0 = psel(q, st.bx[q > 0 ? q - 1 : 0][0], st.bprev[0]), p1 = psel(q, st.bx[q > 0 ? q - 1 : 0][1], st.bprev[1]), p2 = psel(q, st.bx[q > 0 ? q - 1 : 0][2], st.bprev[2]);
                const double ut = T::HAS_U ? psel(q, st.bxu[gIn(q)], st.bprev[3]) : 0.0;
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double zt = d.f[r][0] * p0 + d.f[r][1] * p1 + d.f[r][2] * p2 + d.beta[r] * ut - fn.xt[dyn_tau<F>(r)];
                    const double dv = al * (zt - (first ? 0.0 : d.b[r]));
                    st.vd[q][r] += dv;
                    dy_in[r] = re[r] * dv; bsum += d.b[r] * dy_in[r];
                    if (CERT && in_own_group(q)) dytk[gIn(q)] += dy_in[r] * d.beta[r];
                }
            }
            if constexpr (CERT) {
                // equality rows: dy unrestricted, u.dy+ + l.dy- = b.dy ; A'dy on this stage's variables
                double ad[5];
#pragma unroll
                for (int a = 0; a < 5; ++a) ad[a] = fn.ady[a];
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) { ad[dyn_tau<F>(r)] -= dy_in[r]; fn.ndy = fmax(fn.ndy, fabs(dy_in[r])); }
                if (j < N - 1) {
                    const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                    for (int r = 0; r < T::NDYN; ++r) { ad[0] += dy_out[r] * d.f[r][0]; ad[1] += dy_out[r] * d.f[r][1]; ad[2] += dy_out[r] * d.f[r][2]; }
                }
#pragma unroll
                for (int a = 0; a < 3 + T::NS; ++a) ct.natdy = fmax(ct.natdy, fabs(ad[a]));
                ct.ndy = fmax(ct.ndy, fn.ndy);
                ct.sup += fn.sup + bsum;
            }
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) dy_next[r] = dy_in[r];
#pragma unroll
            for (int a = 0; a < 3 + T::NS; ++a) st.x[q][a] += al * (fn.xt[a] - st.x[q][a]);
        }
        if constexpr (CERT && NW == 2) {  // A' dy on the control sums over the group's transitions: the other role's go through LDS
            if (wrole() != own_role() && clane() < L.TP) S[L.hx1 + clane()] = dytk[0];
            __syncthreads();
            if (wrole() == own_role() && clane() < L.TP) dytk[0] += S[L.hx1 + clane()];
            __syncthreads();
        }
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (has_ctl(g)) {
                    typename std::conditional<CERT, UpdCertFn, UpdFnX<FIRST>>::type fn;
                    fn.alpha = al;
                    if constexpr (CERT) fn.first = first;
                    if constexpr (CERT) {
                        fn.rho = rho; fn.rho_eq = rho_eq; fn.W = Wctl(); fn.E = Ectl(); fn.cls = st.clsc; fn.ndy = 0; fn.sup = 0;
#pragma unroll
                        for (int a = 0; a < 5; ++a) fn.ady[a] = 0;
                    }
                    fn.xt[0] = fn.xt[1] = fn.xt[4] = 0;
                    fn.xt[2] = st.bxu[g];
                    fn.xt[3] = T::HAS_SU ? (st.gsu - st.hus * fn.xt[2]) * st.hiu : 0.0;
                    fn.v = st.vc[g]; fn.stride = 1;
                    if constexpr (POL) { PolWrap<UFn> w{fn, st.pcc}; ctl_rows<F>(st.mkp, w); } else ctl_rows<F>(st.mkp, fn);
                    st.u[g] += al * (fn.xt[2] - st.u[g]);
                    if constexpr (T::HAS_SU) st.su += al * (fn.xt[3] - st.su);
                    if constexpr (CERT) {
                        ct.natdy = fmax(ct.natdy, fabs(fn.ady[2] + dytk[g]));
                        if constexpr (T::HAS_SU) ct.natdy = fmax(ct.natdy, fabs(fn.ady[3]));
                        ct.ndy = fmax(ct.ndy, fn.ndy);
                        ct.sup += fn.sup;
                    }
                }
            }
        }
        if constexpr (CERT) {
            ct.ndy = wave_max(ct.ndy); ct.natdy = wave_max(ct.natdy); ct.sup = wave_sum(ct.sup);
            if constexpr (NT > 64) {
                __syncthreads();
                double *red = S + L.ex;
                const int w = tid >> 6;
                if ((tid & 63) == 0) { red[w * 3] = ct.ndy; red[w * 3 + 1] = ct.natdy; red[w * 3 + 2] = ct.sup; }
                __syncthreads();
                ct.ndy = 0; ct.natdy = 0; ct.sup = 0;
                for (int k = 0; k < NT / 64; ++k) { ct.ndy = fmax(ct.ndy, red[k * 3]); ct.natdy = fmax(ct.natdy, red[k * 3 + 1]); ct.sup += red[k * 3 + 2]; }
                __syncthreads();
            }
        }
        return ct;
    }

    // x of the neighbouring stages for the row passes: pl = (x of the stage before the own first stage, control of the transition into the own first stage), nf = x of
    // the stage after the own last stage (NEXT: only where it is needed), uown = the own chunk's control (role-split mapping: the role that does not hold it gets it here)
    template <bool NEXT> __device__ __forceinline__ void nbr_x(const LS &st, double pl[4], double nf[3], double &uown) const {
        double xl[4] = {0, 0, 0, st.u[NG - 1]}, xf[4] = {0, 0, 0, 0};  // (the transition into the next lane's first stage belongs to this lane's last group)
        bool got = false;
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            if (stage(q) < N) {
                xl[0] = st.x[q][0]; xl[1] = st.x[q][1]; xl[2] = st.x[q][2];  // ends up as the last own stage
                if (!got) { xf[0] = st.x[q][0]; xf[1] = st.x[q][1]; xf[2] = st.x[q][2]; got = true; }
            }
        }
        if constexpr (NW == 1) { xf[0] = st.x[0][0]; xf[1] = st.x[0][1]; xf[2] = st.x[0][2]; }
        uown = st.u[0];
        nf[0] = nf[1] = nf[2] = 0;
        if constexpr (NW == 1) {
            xchg<4>(xl, -1, pl, 0);
            if constexpr (NEXT) xchg<3>(xf, +1, nf, 1);
        } else {
            // previous stage's owner: role B -> role A of the next chunk (with its control), role A -> role B of the same chunk; the role without the control gets it from the other
            hx_put(wrole() == 1 ? L.hx0 : L.hx1, xl);
            __syncthreads();
            double t_[4];
            if (wrole() == 0) { hx_get(L.hx0, clane() - 1, pl); hx_get(L.hx0, clane(), t_); }
            else { hx_get(L.hx1, clane(), pl); hx_get(L.hx1, clane(), t_); pl[3] = 0; }
            if (!has_ctl()) uown = t_[3];
            if (wrole() == 1) pl[3] = uown;  // the transition into role B's first stage belongs to the own group
            __syncthreads();
            if constexpr (NEXT) {  // next stage's owner: role A -> role B of the previous chunk, role B -> role A of the same chunk
                hx_put(wrole() == 0 ? L.hx0 : L.hx1, xf);
                __syncthreads();
                if (wrole() == 0) hx_get(L.hx1, clane(), t_); else hx_get(L.hx0, clane() + 1, t_);
                nf[0] = t_[0]; nf[1] = t_[1]; nf[2] = t_[2];
                __syncthreads();
            }
        }
    }
    template <bool UNI = false> __device__ __forceinline__ Resid residual_pass_two(const LS &st, double rho) const {
        const double rho_eq = eq_step(rho);
        double pl[4], nf[3] = {0, 0, 0};
        double uown;  // control of the own chunk
        nbr_x<F == F_K>(st, pl, nf, uown);
        const double nf2 = nf[2];
        double m[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        double re[T::NDYN], ed[T::NDYN], ytku[NG], ob = 0;  // ytku: the dynamics rows' part of A'y on the controls, per group of the lane
#pragma unroll
        for (int g = 0; g < NG; ++g) ytku[g] = 0;
        int bad = 0;
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) { re[r] = eq_row_step(rho_eq, r); ed[r] = eq_row_scale(r); }
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            ResFn fn;
            fn.rho = rho; fn.rho_eq = rho_eq; fn.W = Wloc(j); fn.E = Eloc(j); fn.cls = cls_of<UNI>(st, q);
            fn.rp = fn.nAx = fn.nz = fn.rps = fn.nAxs = fn.nzs = 0;
#pragma unroll
            for (int a = 0; a < 5; ++a) { fn.x[a] = a < 3 + T::NS ? st.x[q][a] : 0.0; fn.aty[a] = 0; }
            fn.v = st.vl[q]; fn.stride = 1;
            local_rows<F>(si, P, fn);
            if (T::NEND && si.last) { fn.v = st.vend; fn.W = Wend(); fn.E = Eend(); fn.cls = st.clse; end_rows<F>(si, P, fn); }
            double bin[3] = {0, 0, 0}, ax[3] = {0, 0, 0};
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) { bin[r] = st.bin0[r]; ax[r] = -fn.x[dyn_tau<F>(r)]; }
            } else {
                const Dyn<F> d = dyn_in(st, q);
                const double p0 = psel(q, st.x[q > 0 ? q - 1 : 0][0], pl[0]), p1 = psel(q, st.x[q > 0 ? q - 1 : 0][1], pl[1]), p2 = psel(q, st.x[q > 0 ? q - 1 : 0][2], pl[2]);
                const double uu = T::HAS_U ? psel(q, NW == 1 ? st.u[gIn(q)] : uown, pl[3]) : 0.0;
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    bin[r] = d.b[r];
                    ax[r] = d.f[r][0] * p0 + d.f[r][1] * p1 + d.f[r][2] * p2 + d.beta[r] * uu - fn.x[dyn_tau<F>(r)];
                    if (in_own_group(q)) ytku[gIn(q)] += re[r] * (st.vd[q][r] - d.b[r]) * d.beta[r];
                }
            }
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) {
                const double y = re[r] * (st.vd[q][r] - bin[r]);
                const double a0 = fabs(ax[r] - bin[r]), a1 = fabs(ax[r]), a2 = fabs(bin[r]);
                fn.rp = fmax(fn.rp, a0); fn.nAx = fmax(fn.nAx, a1); fn.nz = fmax(fn.nz, a2);
                fn.rps = fmax(fn.rps, ed[r] * a0); fn.nAxs = fmax(fn.nAxs, ed[r] * a1); fn.nzs = fmax(fn.nzs, ed[r] * a2);
                fn.aty[dyn_tau<F>(r)] -= y;
            }
            if (j < N - 1) {
                const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double vv = q + 1 < SPL ? st.vd[q + 1 < SPL ? q + 1 : q][r] : st.vdo[r];
                    const double y = re[r] * (vv - d.b[r]);
                    fn.aty[0] += y * d.f[r][0]; fn.aty[1] += y * d.f[r][1]; fn.aty[2] += y * d.f[r][2];
                    if (q == SPL - 1 && out_own_group(q)) ytku[NG - 1] += y * d.beta[r];
                }
            }
            double px[5];
            px[0] = p_diag_node<F>(0, j, N, P) * fn.x[0];
            px[1] = 0.0;
            px[2] = p_diag_node<F>(2, j, N, P) * fn.x[2];
            if constexpr (F == F_K) {
                if (j <= N - 2) {
                    if (j >= 1) px[2] -= P.w_cr * (q > 0 ? st.x[q > 0 ? q - 1 : 0][2] : pl[2]);
                    if (j + 1 <= N - 2) px[2] -= P.w_cr * (q + 1 < SPL ? st.x[q + 1 < SPL ? q + 1 : q][2] : nf2);
                }
            }
            px[3] = P.w_s1 * fn.x[3];
            px[4] = T::NS > 1 ? P.w_s2 * fn.x[4] : 0.0;
#pragma unroll
            for (int a = 0; a < 3 + T::NS; ++a) {
                ob += fn.x[a] * px[a];
                bad |= nonfinite_bits(fn.x[a]) | nonfinite_bits(px[a] + fn.aty[a]);
                const double g0 = fabs(px[a] + fn.aty[a]), g1 = fabs(px[a]), g2 = fabs(fn.aty[a]), cd = cD(a, j);
                m[1] = fmax(m[1], g0); m[4] = fmax(m[4], g1); m[5] = fmax(m[5], g2);
                m[7] = fmax(m[7], cd * g0); m[10] = fmax(m[10], cd * g1); m[11] = fmax(m[11], cd * g2);
            }
            m[0] = fmax(m[0], fn.rp); m[2] = fmax(m[2], fn.nAx); m[3] = fmax(m[3], fn.nz);
            m[6] = fmax(m[6], fn.rps); m[8] = fmax(m[8], fn.nAxs); m[9] = fmax(m[9], fn.nzs);
        }
        if constexpr (NW == 2) {  // the control's dual residual sums over the group's transitions: the other role's go through LDS
            if (wrole() != own_role() && clane() < L.TP) S[L.hx1 + clane()] = ytku[0];
            __syncthreads();
            if (wrole() == own_role() && clane() < L.TP) ytku[0] += S[L.hx1 + clane()];
            __syncthreads();
        }
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g)
            if (has_ctl(g)) {
                ResFn fn;
                fn.rho = rho; fn.rho_eq = rho_eq; fn.W = Wctl(); fn.E = Ectl(); fn.cls = st.clsc;
                fn.rp = fn.nAx = fn.nz = fn.rps = fn.nAxs = fn.nzs = 0;
                fn.x[0] = fn.x[1] = fn.x[4] = 0; fn.x[2] = st.u[g]; fn.x[3] = T::HAS_SU ? st.su : 0.0;
#pragma unroll
                for (int a = 0; a < 5; ++a) fn.aty[a] = 0;
                fn.v = st.vc[g]; fn.stride = 1;
                ctl_rows<F>(st.mkp, fn);
                fn.aty[2] += ytku[g];
                const double pxv[2] = {P.w_u * fn.x[2], T::HAS_SU ? P.w_su * fn.x[3] : 0.0};
#pragma unroll
                for (int a = 0; a < 1 + T::HAS_SU; ++a) {
                    ob += fn.x[2 + a] * pxv[a];
                    bad |= nonfinite_bits(fn.x[2 + a]) | nonfinite_bits(pxv[a] + fn.aty[2 + a]);
                    const double g0 = fabs(pxv[a] + fn.aty[2 + a]), g1 = fabs(pxv[a]), g2 = fabs(fn.aty[2 + a]), cd = cD(5 + a);
                    m[1] = fmax(m[1], g0); m[4] = fmax(m[4], g1); m[5] = fmax(m[5], g2);
                    m[7] = fmax(m[7], cd * g0); m[10] = fmax(m[10], cd * g1); m[11] = fmax(m[11], cd * g2);
                }
                m[0] = fmax(m[0], fn.rp); m[2] = fmax(m[2], fn.nAx); m[3] = fmax(m[3], fn.nz);
                m[6] = fmax(m[6], fn.rps); m[8] = fmax(m[8], fn.nAxs); m[9] = fmax(m[9], fn.nzs);
            }
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = wave_max(m[i]);
        ob = wave_sum(ob);
        bad = __any(bad) ? 1 : 0;
        if constexpr (NT > 64) {
            __syncthreads();
            double *red = S + L.ex;
            const int w = tid >> 6;
            if ((tid & 63) == 0) {
#pragma unroll
                for (int i = 0; i < 12; ++i) red[w * 14 + i] = m[i];
                red[w * 14 + 12] = ob; red[w * 14 + 13] = bad ? 1.0 : 0.0;
            }
            __syncthreads();
            ob = 0;
            for (int k = 0; k < NT / 64; ++k) {
#pragma unroll
                for (int i = 0; i < 12; ++i) m[i] = fmax(m[i], red[k * 14 + i]);
                ob += red[k * 14 + 12];
                bad |= red[k * 14 + 13] != 0.0;
            }
            __syncthreads();
        }
        Resid R = {m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11], 0.5 * ob, bad};
        return R;
    }

// ==================== [newton_passes] ====================
// members of Fast, part 10: what the phases AFTER the ADMM loop add to the two-level mapping.  TWO only, every NWX.
//   state_io / park_io <STORE>      the lane's ADMM state (x and every v; park_io: + the classes of the factorisation in use, kept in st.pc*) to / from a block in HBM,
//                                   [k][NT] so that a wave's access is coalesced: the hand-over between the solve, Newton, fallback and polish launches ([kernels])
//   block_any, block_sum2           block-wide OR / pair of sums: one wave — DPP / __any only; NT > 64 — through ex with three barriers (role-split: ex is hand-off slot 1)
//   reclass_pass                    row classes st.cls* from the rows' activity (ReclassFn, [row_fns]) and v re-expressed for the new steps
//   nw_reexpress_pass, nw_dir_of, nw_dir_pass<MODE>, nw_ls_eval01, nw_ls_eval      the Newton refinement's own passes (the banner below): w = a.x + y / rho from the
//                                   iterate; the direction's slope terms / the step applied; the merit function and its derivative along the direction (exact line search)
//   LDS     nothing but ex (NT > 64) and what nbr_x uses ([two_update])
//   lanes   reclass_pass writes cls*, vl, vd, vdo, vend, vc; nw_reexpress_pass every v; nw_dir_pass<1> x, u, su and every v; the direction is read where the solve left
//           it (bx, bxu, bnext, bprev; slacks from gs / gsu, hi, hv, hiu, hus); the others write nothing
//   called  the passes by refine_phase_newton ([loops]) only; block_any also by the pivot scans; state_io / park_io by the kernels
    static constexpr int kStateDoubles = SPL * (3 + T::NS) + SPL * T::NLOC + SPL * T::NDYN + T::NDYN + 2 + 1 + 4 * NG;  // x, vl, vd, vdo, vend, su, (u, vc) per control
    template <bool STORE> __device__ __forceinline__ void state_io(LS &st, double *base) const {  // [k][NT]: coalesced
        int k = 0;
        auto io = [&](double &v) { if constexpr (STORE) base[(size_t)k * NT + tid] = v; else v = base[(size_t)k * NT + tid]; ++k; };
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
#pragma unroll
            for (int a = 0; a < 3 + T::NS; ++a) io(st.x[q][a]);
#pragma unroll
            for (int r = 0; r < T::NLOC; ++r) io(st.vl[q][r]);
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) io(st.vd[q][r]);
        }
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) io(st.vdo[r]);
        io(st.vend[0]); io(st.vend[1]); io(st.su);
#pragma unroll
        for (int g = 0; g < NG; ++g) { io(st.u[g]); io(st.vc[g][0]); io(st.vc[g][1]); io(st.vc[g][2]); }
    }
    // a parked Newton path (sliced launches): the lane state, then the classes of the factorisation it was using (st.pc*: free outside the polish), [kParkDoubles][NT]
    static constexpr int kParkDoubles = kStateDoubles + SPL + 2;
    template <bool STORE> __device__ __forceinline__ void park_io(LS &st, double *base) const {
        state_io<STORE>(st, base);
        double *c = base + (size_t)kStateDoubles * NT;
#pragma unroll
        for (int q = 0; q < SPL; ++q) { if constexpr (STORE) c[(size_t)q * NT + tid] = (double)st.pc[q]; else st.pc[q] = (unsigned)c[(size_t)q * NT + tid]; }
        if constexpr (STORE) { c[(size_t)SPL * NT + tid] = (double)st.pce; c[(size_t)(SPL + 1) * NT + tid] = (double)st.pcc; }
        else { st.pce = (unsigned)c[(size_t)SPL * NT + tid]; st.pcc = (unsigned)c[(size_t)(SPL + 1) * NT + tid]; }
    }
    __device__ __forceinline__ bool block_any(bool f) const {
        bool a = __any(f) != 0;
        if constexpr (NT > 64) {
            __syncthreads();
            double *red = S + L.ex;
            if ((tid & 63) == 0) red[tid >> 6] = a ? 1.0 : 0.0;
            __syncthreads();
            a = false;
            for (int k = 0; k < NT / 64; ++k) a = a || red[k] != 0.0;
            __syncthreads();
        }
        return a;
    }
    // Refinement: row classes (st.cls*) from activity, v re-expressed for the change of step (rho_old -> rho_new included); true when a class changed
    // req_old / req_new: the equality rows' step before / after when it is not 1e3 x rho (leaving the Newton refinement)
    __device__ __forceinline__ bool reclass_pass(LS &st, const unsigned cls0[SPL], unsigned clse0, unsigned clsc0, double rho_old, double rho_new, int mode, double req_old = -1.0, double req_new = -1.0) const {
        ReclassFn fn;
        fn.rho_o = rho_old; fn.rho_n = rho_new;
        fn.req_o = req_old > 0.0 ? req_old : kRhoEqOverIneq * rho_old; fn.req_n = req_new > 0.0 ? req_new : kRhoEqOverIneq * rho_new;
        fn.mode = mode; fn.changes = 0;
        static_assert(T::NLOC <= 9 && T::NCTL <= 9, "ReclassFn::v");
        const double ratio = fn.req_o / fn.req_n;  // the dynamics rows are equalities
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
#pragma unroll
            for (int r = 0; r < T::NLOC; ++r) fn.v[r] = st.vl[q][r];
            fn.cls_type = cls0[q]; fn.cls_old = st.cls[q]; fn.cls_new = 0;
            local_rows<F>(si, P, fn);
#pragma unroll
            for (int r = 0; r < T::NLOC; ++r) st.vl[q][r] = fn.v[r];
            st.cls[q] = fn.cls_new;
            if (T::NEND && si.last) {
                fn.v[0] = st.vend[0]; fn.v[1] = st.vend[1];
                fn.cls_type = clse0; fn.cls_old = st.clse; fn.cls_new = 0;
                end_rows<F>(si, P, fn);
                st.vend[0] = fn.v[0]; st.vend[1] = fn.v[1];
                st.clse = fn.cls_new;
            }
            if (ratio != 1.0) {  // dynamics rows: equalities, step rho_eq
                if (j == 0) {
#pragma unroll
                    for (int r = 0; r < T::NDYN; ++r) st.vd[q][r] = st.bin0[r] + ratio * (st.vd[q][r] - st.bin0[r]);
                } else {
                    const Dyn<F> d = dyn_in(st, q);
#pragma unroll
                    for (int r = 0; r < T::NDYN; ++r) st.vd[q][r] = d.b[r] + ratio * (st.vd[q][r] - d.b[r]);
                }
                if (q == SPL - 1 && j < N - 1) {
                    const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                    for (int r = 0; r < T::NDYN; ++r) st.vdo[r] = d.b[r] + ratio * (st.vdo[r] - d.b[r]);
                }
            }
        }
        if constexpr (T::HAS_U) {
            const unsigned clsc_old = st.clsc;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (has_ctl(g)) {
#pragma unroll
                    for (int r = 0; r < 3; ++r) fn.v[r] = st.vc[g][r];
                    fn.cls_type = clsc0; fn.cls_old = clsc_old; fn.cls_new = 0;
                    ctl_rows<F>(st.mkp, fn);
#pragma unroll
                    for (int r = 0; r < 3; ++r) st.vc[g][r] = fn.v[r];
                    st.clsc = fn.cls_new;  // (several controls per lane: KP, whose one control row is free — the same class for every group)
                }
            }
        }
        return block_any(fn.changes != 0);
    }
    // =====================================================================================================
    // NEWTON REFINEMENT (po_params.refine = 2; two-level mapping, every lane layout): semismooth Newton on the augmented Lagrangian
    //     phi_y(x) = 1/2 x'Px + sum_i rho_i / 2 dist^2(a_i x + y_i / rho_i, [l_i, u_i])
    // with an exact line search (po_hip.h; oracle/po_oracle.c `refine == 2`).  The one-number-per-row state holds w_i = a_i x + y_i / rho_i, so that
    // z = clip(w), y = rho (w - z) and the gradient of phi is the dual residual of (x, y): residual_pass_two serves as it is.  The Newton matrix is the
    // ADMM matrix with the rows outside their bounds at rho_i and the others at RHO_MIN (row classes 0 / 1 / 2, reclass_pass mode 3), its right-hand side
    // minus the gradient (rhs_pass_two<.., NWT>), so factor_*_two and solve_two are used unchanged; what is new are the passes below.
    // =====================================================================================================
    __device__ __forceinline__ void block_sum2(double &a, double &b) const {
        a = wave_sum(a); b = wave_sum(b);
        if constexpr (NT > 64) {
            __syncthreads();
            double *red = S + L.ex;
            const int w = tid >> 6;
            if ((tid & 63) == 0) { red[2 * w] = a; red[2 * w + 1] = b; }
            __syncthreads();
            a = 0; b = 0;
            for (int k = 0; k < NT / 64; ++k) { a += red[2 * k]; b += red[2 * k + 1]; }
            __syncthreads();
        }
    }
    // v <- a.x + ratio (v - clip(v)) on every row (free rows: v - clip(v) = 0)
    __device__ __forceinline__ void nw_reexpress_pass(LS &st, double ratio, double ratio_eq, const unsigned cls0[SPL], unsigned clse0, unsigned clsc0) const {
        double pl[4], nf[3] = {0, 0, 0}, uown;
        nbr_x<true>(st, pl, nf, uown);
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            NwReexFn fn;
            fn.ratio = ratio; fn.ratio_eq = ratio_eq; fn.cls_type = cls0[q];
#pragma unroll
            for (int a = 0; a < 5; ++a) fn.x[a] = a < 3 + T::NS ? st.x[q][a] : 0.0;
            fn.v = st.vl[q];
            local_rows<F>(si, P, fn);
            if (T::NEND && si.last) { fn.v = st.vend; fn.cls_type = clse0; end_rows<F>(si, P, fn); }
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) st.vd[q][r] = -fn.x[dyn_tau<F>(r)] + ratio_eq * (st.vd[q][r] - st.bin0[r]);
            } else {
                const Dyn<F> d = dyn_in(st, q);
                const double p0 = psel(q, st.x[q > 0 ? q - 1 : 0][0], pl[0]), p1 = psel(q, st.x[q > 0 ? q - 1 : 0][1], pl[1]), p2 = psel(q, st.x[q > 0 ? q - 1 : 0][2], pl[2]);
                const double uu = T::HAS_U ? psel(q, NW == 1 ? st.u[gIn(q)] : uown, pl[3]) : 0.0;
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double ax = d.f[r][0] * p0 + d.f[r][1] * p1 + d.f[r][2] * p2 + d.beta[r] * uu - fn.x[dyn_tau<F>(r)];
                    st.vd[q][r] = ax + ratio_eq * (st.vd[q][r] - d.b[r]);
                }
            }
            if (q == SPL - 1 && j < N - 1) {  // the copy of the next chunk's incoming rows
                const Dyn<F> d = dyn_out(st, q);
                const double uu = T::HAS_U ? (NW == 1 ? st.u[NG - 1] : uown) : 0.0;
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double ax = d.f[r][0] * fn.x[0] + d.f[r][1] * fn.x[1] + d.f[r][2] * fn.x[2] + d.beta[r] * uu - nf[dyn_tau<F>(r)];
                    st.vdo[r] = ax + ratio_eq * (st.vdo[r] - d.b[r]);
                }
            }
        }
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (has_ctl(g)) {
                    NwReexFn fn;
                    fn.ratio = ratio; fn.ratio_eq = ratio_eq; fn.cls_type = clsc0;
                    fn.x[0] = fn.x[1] = fn.x[4] = 0; fn.x[2] = st.u[g]; fn.x[3] = T::HAS_SU ? st.su : 0.0;
                    fn.v = st.vc[g];
                    ctl_rows<F>(st.mkp, fn);
                }
            }
        }
    }
    // the direction's components on own stage q: node part from the solve (st.bx), slack parts recovered from the eliminated rows
    __device__ __forceinline__ void nw_dir_of(const LS &st, int q, double xt[5]) const {
        xt[0] = st.bx[q][0]; xt[1] = st.bx[q][1]; xt[2] = st.bx[q][2]; xt[3] = xt[4] = 0;
#pragma unroll
        for (int s = 0; s < T::NS; ++s) xt[3 + s] = (st.gs[q][s] - (st.hv[q][s][0] * xt[0] + st.hv[q][s][1] * xt[1] + st.hv[q][s][2] * xt[2])) * st.hi[q][s];
    }
    // MODE 0: c0, c1 of psi'(t) = c0 + c1 t + [inequality rows]  (lane-local partial sums; the caller reduces).  MODE 1: x += t d, v += t a.d.
    // The direction is where solve_two left it: st.bx / st.bxu[0], the neighbours' parts in st.bprev (previous stage + its control) and st.bnext.
    template <int MODE> __device__ __forceinline__ void nw_dir_pass(LS &st, double rho, double t, const unsigned cls0[SPL], unsigned clse0, unsigned clsc0, double &c0, double &c1, double &f0i) const {
        const double rho_eq = eq_step(rho);
        double re[T::NDYN];
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) re[r] = eq_row_step(rho_eq, r);
        double xp2 = 0, xn2 = 0;  // K, MODE 0: steering of the neighbouring stages at x (tridiagonal R block of P)
        if constexpr (MODE == 0 && F == F_K) {
            const int nst = nst_own();
            double xl[3] = {0, 0, 0}, pl[3], nf[3], xf[3] = {st.x[0][0], st.x[0][1], st.x[0][2]};
#pragma unroll
            for (int q = 0; q < SPL; ++q) if (q == nst - 1) { xl[0] = st.x[q][0]; xl[1] = st.x[q][1]; xl[2] = st.x[q][2]; }
            xchg<3>(xl, -1, pl, 0);
            xchg<3>(xf, +1, nf, 1);
            xp2 = pl[2]; xn2 = nf[2];
        }
        double a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
        for (int q = SPL - 1; q >= 0; --q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            NwDirFn<MODE> fn;
            fn.t = t; fn.rho = rho; fn.rho_eq = rho_eq; fn.c0 = fn.c1 = fn.f0 = 0; fn.cls_type = cls0[q]; fn.W = Wloc(j);
            nw_dir_of(st, q, fn.xt);
            fn.v = st.vl[q];
            local_rows<F>(si, P, fn);
            if (T::NEND && si.last) { fn.v = st.vend; fn.cls_type = clse0; fn.W = Wend(); end_rows<F>(si, P, fn); }
            if (q == SPL - 1 && j < N - 1) {  // the copy of the next chunk's incoming rows moves with them (MODE 1); counted by their owner (MODE 0)
                if constexpr (MODE == 1) {
                    const Dyn<F> d = dyn_out(st, q);
                    const double ut = T::HAS_U ? st.bxu[NG - 1] : 0.0;
#pragma unroll
                    for (int r = 0; r < T::NDYN; ++r)
                        st.vdo[r] += t * (d.f[r][0] * fn.xt[0] + d.f[r][1] * fn.xt[1] + d.f[r][2] * fn.xt[2] + d.beta[r] * ut - st.bnext[dyn_tau<F>(r)]);
                }
            }
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double s = -fn.xt[dyn_tau<F>(r)];
                    if constexpr (MODE == 0) { fn.c0 += re[r] * (st.vd[q][r] - st.bin0[r]) * s; fn.c1 += re[r] * s * s; }
                    else st.vd[q][r] += t * s;
                }
            } else {
                const Dyn<F> d = dyn_in(st, q);
                const double p0 = psel(q, st.bx[q > 0 ? q - 1 : 0][0], st.bprev[0]), p1 = psel(q, st.bx[q > 0 ? q - 1 : 0][1], st.bprev[1]), p2 = psel(q, st.bx[q > 0 ? q - 1 : 0][2], st.bprev[2]);
                const double ut = T::HAS_U ? psel(q, st.bxu[gIn(q)], st.bprev[3]) : 0.0;
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double s = d.f[r][0] * p0 + d.f[r][1] * p1 + d.f[r][2] * p2 + d.beta[r] * ut - fn.xt[dyn_tau<F>(r)];
                    if constexpr (MODE == 0) { fn.c0 += re[r] * (st.vd[q][r] - d.b[r]) * s; fn.c1 += re[r] * s * s; }
                    else st.vd[q][r] += t * s;
                }
            }
            if constexpr (MODE == 0) {
                double pd[5] = {p_diag_node<F>(0, j, N, P), 0.0, p_diag_node<F>(2, j, N, P), P.w_s1, T::NS > 1 ? P.w_s2 : 0.0};
                double px[5], pdd[5];
#pragma unroll
                for (int a = 0; a < 5; ++a) { px[a] = a < 3 + T::NS ? pd[a] * st.x[q][a < 3 + T::NS ? a : 0] : 0.0; pdd[a] = a < 3 + T::NS ? pd[a] * fn.xt[a] : 0.0; }
                if constexpr (F == F_K) {
                    if (j <= N - 2) {
                        if (j >= 1) { px[2] -= P.w_cr * (q > 0 ? st.x[q > 0 ? q - 1 : 0][2] : xp2); pdd[2] -= P.w_cr * (q > 0 ? st.bx[q > 0 ? q - 1 : 0][2] : st.bprev[2]); }
                        if (j + 1 <= N - 2) { px[2] -= P.w_cr * (q + 1 < SPL ? st.x[q + 1 < SPL ? q + 1 : q][2] : xn2); pdd[2] -= P.w_cr * (q + 1 < SPL ? st.bx[q + 1 < SPL ? q + 1 : q][2] : st.bnext[2]); }
                    }
                }
#pragma unroll
                for (int a = 0; a < 3 + T::NS; ++a) { fn.c0 += fn.xt[a] * px[a]; fn.c1 += fn.xt[a] * pdd[a]; }
                a0 += fn.c0; a1 += fn.c1; a2 += fn.f0;
            } else {
#pragma unroll
                for (int a = 0; a < 3 + T::NS; ++a) st.x[q][a] += t * fn.xt[a];
            }
        }
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (has_ctl(g)) {
                    NwDirFn<MODE> fn;
                    fn.t = t; fn.rho = rho; fn.rho_eq = rho_eq; fn.c0 = fn.c1 = fn.f0 = 0; fn.cls_type = clsc0; fn.W = Wctl();
                    fn.xt[0] = fn.xt[1] = fn.xt[4] = 0;
                    fn.xt[2] = st.bxu[g];
                    fn.xt[3] = T::HAS_SU ? (st.gsu - st.hus * fn.xt[2]) * st.hiu : 0.0;
                    fn.v = st.vc[g];
                    ctl_rows<F>(st.mkp, fn);
                    if constexpr (MODE == 0) {
                        fn.c0 += fn.xt[2] * (P.w_u * st.u[g]); fn.c1 += fn.xt[2] * (P.w_u * fn.xt[2]);
                        if constexpr (T::HAS_SU) { fn.c0 += fn.xt[3] * (P.w_su * st.su); fn.c1 += fn.xt[3] * (P.w_su * fn.xt[3]); }
                        a0 += fn.c0; a1 += fn.c1; a2 += fn.f0;
                    } else {
                        st.u[g] += t * fn.xt[2];
                        if constexpr (T::HAS_SU) st.su += t * fn.xt[3];
                    }
                }
            }
        }
        if constexpr (MODE == 0) { c0 = a0; c1 = a1; f0i = a2; }
    }
    // psi'(0), psi'(1) and the slope at 1 in one pass (NwLs01Fn), inequality rows only (block-wide sums)
    __device__ __forceinline__ void nw_ls_eval01(const LS &st, double rho, const unsigned cls0[SPL], unsigned clse0, unsigned clsc0, double &f0, double &f1, double &fp1) const {
        double a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            NwLs01Fn fn;
            fn.rho = rho; fn.f0 = fn.f1 = fn.fp1 = 0; fn.cls_type = cls0[q]; fn.W = Wloc(j);
            nw_dir_of(st, q, fn.xt);
            fn.v = st.vl[q];
            local_rows<F>(si, P, fn);
            if (T::NEND && si.last) { fn.v = st.vend; fn.cls_type = clse0; fn.W = Wend(); end_rows<F>(si, P, fn); }
            a0 += fn.f0; a1 += fn.f1; a2 += fn.fp1;
        }
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (has_ctl(g)) {
                    NwLs01Fn fn;
                    fn.rho = rho; fn.f0 = fn.f1 = fn.fp1 = 0; fn.cls_type = clsc0; fn.W = Wctl();
                    fn.xt[0] = fn.xt[1] = fn.xt[4] = 0;
                    fn.xt[2] = st.bxu[g];
                    fn.xt[3] = T::HAS_SU ? (st.gsu - st.hus * fn.xt[2]) * st.hiu : 0.0;
                    fn.v = st.vc[g];
                    ctl_rows<F>(st.mkp, fn);
                    a0 += fn.f0; a1 += fn.f1; a2 += fn.fp1;
                }
            }
        }
        double z_ = 0;
        block_sum2(a0, a1);
        block_sum2(a2, z_);
        f0 = a0; f1 = a1; fp1 = a2;
    }
    // psi'(t) and the slope of its current linear piece, inequality rows only (block-wide sums)
    __device__ __forceinline__ void nw_ls_eval(const LS &st, double rho, double t, const unsigned cls0[SPL], unsigned clse0, unsigned clsc0, double &f, double &fp) const {
        double a0 = 0, a1 = 0;
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            NwLsFn fn;
            fn.t = t; fn.rho = rho; fn.f = fn.fp = 0; fn.cls_type = cls0[q]; fn.W = Wloc(j);
            nw_dir_of(st, q, fn.xt);
            fn.v = st.vl[q];
            local_rows<F>(si, P, fn);
            if (T::NEND && si.last) { fn.v = st.vend; fn.cls_type = clse0; fn.W = Wend(); end_rows<F>(si, P, fn); }
            a0 += fn.f; a1 += fn.fp;
        }
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (has_ctl(g)) {
                    NwLsFn fn;
                    fn.t = t; fn.rho = rho; fn.f = fn.fp = 0; fn.cls_type = clsc0; fn.W = Wctl();
                    fn.xt[0] = fn.xt[1] = fn.xt[4] = 0;
                    fn.xt[2] = st.bxu[g];
                    fn.xt[3] = T::HAS_SU ? (st.gsu - st.hus * fn.xt[2]) * st.hiu : 0.0;
                    fn.v = st.vc[g];
                    ctl_rows<F>(st.mkp, fn);
                    a0 += fn.f; a1 += fn.fp;
                }
            }
        }
        block_sum2(a0, a1);
        f = a0; fp = a1;
    }

// ==================== [polish_passes] ====================
// members of Fast, part 11: the passes only OSQP's polish has.  TWO only, one lane per chunk (NWX 1, 4, 5: polish_kernel's static_assert).
//   pol_init    the active set of the ADMM point into st.pc / pce / pcc (2 bits per row), from v against the bounds (PolInitFn, [row_fns])
//   pol_reset   start of a reduced KKT solve: x = 0, v = the bound every active row is held at (PolResetFn)
//   pol_eval    residuals, objective and implied active set of the polished point (PolEvalFn -> PolRes)
// The solve itself is the ADMM iteration's: factor_blocks_two / rhs_pass_two / update_pass_two instantiated with POL wrap their row functors in PolWrap.
//   LDS     pol_eval: the xchg mailboxes and the cross-wave reduction at ex (NT > 64); the others touch none
//   lanes   pol_init reads vl, vend, vc, cls* and writes pc*; pol_reset writes x, u, su and every v; pol_eval writes nothing (the new codes go to the caller's pcn*)
//   called  polish_kernel ([kernels]) only
    // =====================================================================================================
    // POLISH (two-level mapping; opt-in, po_params.polish).  The solve kernels leave every lane's ADMM state (x and the one-number-per-row
    // v) in an HBM block (state_io, [newton_passes]); polish_kernel reloads it with the same (SPL, NT) shape.  See PolWrap ([row_fns]) for how the
    // reduced KKT solve maps onto the passes of the ADMM iteration.
    // =====================================================================================================
    // active set of the ADMM solution (st.cls* still hold the row classes of the bounds)
    __device__ __forceinline__ void pol_init(LS &st) const {
        st.pce = st.pcc = 0;
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            st.pc[q] = 0;
            if (stage(q) >= N) continue;
            const StageIn si = stage_in(st, q);
            PolInitFn fn{st.vl[q], st.cls[q], 0u};
            local_rows<F>(si, P, fn);
            st.pc[q] = fn.pc;
            if (T::NEND && si.last) { PolInitFn fe{st.vend, st.clse, 0u}; end_rows<F>(si, P, fe); st.pce = fe.pc; }
        }
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g) if (has_ctl(g)) { PolInitFn fc{st.vc[g], st.clsc, 0u}; ctl_rows<F>(st.mkp, fc); st.pcc = fc.pc; }  // (several controls per lane: KP's one free row, code 0 for every group)
        }
    }
    // start of a pass: x = 0 and y = 0 (v = b on every active row, the dynamics rows included) — OSQP solves (K + dK) s = [-q; b] from scratch
    __device__ __forceinline__ void pol_reset(LS &st) const {
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
#pragma unroll
            for (int a = 0; a < 3 + T::NS; ++a) st.x[q][a] = 0;
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            PolResetFn fn{st.vl[q], st.pc[q]};
            local_rows<F>(si, P, fn);
            if (T::NEND && si.last) { PolResetFn fe{st.vend, st.pce}; end_rows<F>(si, P, fe); }
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) st.vd[q][r] = st.bin0[r];
            } else {
                const Dyn<F> d = dyn_in(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) st.vd[q][r] = d.b[r];
            }
            if (q == SPL - 1 && j < N - 1) {
                const Dyn<F> d = dyn_out(st, q);
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) st.vdo[r] = d.b[r];
            }
        }
        st.su = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g) st.u[g] = 0;
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g) if (has_ctl(g)) { PolResetFn fc{st.vc[g], st.pcc}; ctl_rows<F>(st.mkp, fc); }
        }
    }
    // Residuals of the polished point after project_normalcone (unscaled, like update_info), 0.5 x'Px, and the active set the point implies
    // (written to pcn*; changes = rows whose code differs from st.pc*).  cls0* = the row classes of the bounds.
    __device__ __forceinline__ PolRes pol_eval(const LS &st, const unsigned cls0[SPL], unsigned clse0, unsigned clsc0, double delta,
                                               unsigned pcn[SPL], unsigned &pcne, unsigned &pcnc) const {
        const double idelta = 1.0 / delta;
        const int nst = nst_own();
        double xl[4] = {0, 0, 0, st.u[NG - 1]}, pl[4], nf[3], xf[3] = {st.x[0][0], st.x[0][1], st.x[0][2]};
#pragma unroll
        for (int q = 0; q < SPL; ++q) if (q == nst - 1) { xl[0] = st.x[q][0]; xl[1] = st.x[q][1]; xl[2] = st.x[q][2]; }
        xchg<4>(xl, -1, pl, 0);
        xchg<3>(xf, +1, nf, 1);
        const double nf2 = nf[2];
        double rp = 0, rd = 0, ob = 0, ytku[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) ytku[g] = 0;
        int changes = 0, bad = 0;
        pcne = pcnc = 0;
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            pcn[q] = 0;
            const int j = stage(q);
            if (j >= N) continue;
            const StageIn si = stage_in(st, q);
            PolEvalFn fn;
            fn.v = st.vl[q]; fn.W = Wloc(j); fn.cls = cls0[q]; fn.pc_old = st.pc[q]; fn.pc_new = 0; fn.idelta = idelta; fn.rp = fn.nAx = fn.nz = 0; fn.changes = 0;
#pragma unroll
            for (int a = 0; a < 5; ++a) { fn.x[a] = a < 3 + T::NS ? st.x[q][a] : 0.0; fn.aty[a] = 0; }
            local_rows<F>(si, P, fn);
            pcn[q] = fn.pc_new;
            if (T::NEND && si.last) {
                const unsigned keep_new = fn.pc_new;
                fn.v = st.vend; fn.W = Wend(); fn.cls = clse0; fn.pc_old = st.pce; fn.pc_new = 0;
                end_rows<F>(si, P, fn);
                pcne = fn.pc_new; fn.pc_new = keep_new;
            }
            changes += fn.changes;
            // dynamics rows into stage j (always active): y / W = (v - b) / delta, z = b after the projection, y_new = W (Ax - b) + y
            double bin[3] = {0, 0, 0}, ax[3] = {0, 0, 0};
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) { bin[r] = st.bin0[r]; ax[r] = -fn.x[dyn_tau<F>(r)]; }
            } else {
                const Dyn<F> d = dyn_in(st, q);
                const double p0 = q > 0 ? st.x[q > 0 ? q - 1 : 0][0] : pl[0], p1 = q > 0 ? st.x[q > 0 ? q - 1 : 0][1] : pl[1], p2 = q > 0 ? st.x[q > 0 ? q - 1 : 0][2] : pl[2];
                const double uu = T::HAS_U ? (q > 0 ? st.u[gIn(q)] : pl[3]) : 0.0;
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    bin[r] = d.b[r];
                    ax[r] = d.f[r][0] * p0 + d.f[r][1] * p1 + d.f[r][2] * p2 + d.beta[r] * uu - fn.x[dyn_tau<F>(r)];
                    if (q > 0) ytku[gIn(q)] += Wdyn()[r] * ((ax[r] - d.b[r]) + (st.vd[q][r] - d.b[r]) * idelta) * d.beta[r];
                }
            }
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) {
                const double y = Wdyn()[r] * ((ax[r] - bin[r]) + (st.vd[q][r] - bin[r]) * idelta);
                fn.rp = fmax(fn.rp, fabs(ax[r] - bin[r]));
                fn.aty[dyn_tau<F>(r)] -= y;
            }
            if (j < N - 1) {  // rows out of stage j: A x of the transition needs the next stage's node
                const Dyn<F> d = dyn_out(st, q);
                const double n0 = q + 1 < SPL ? st.x[q + 1 < SPL ? q + 1 : q][0] : nf[0], n1 = q + 1 < SPL ? st.x[q + 1 < SPL ? q + 1 : q][1] : nf[1];
                const double n2 = q + 1 < SPL ? st.x[q + 1 < SPL ? q + 1 : q][2] : nf2;
                const double nx[3] = {n0, n1, n2};
                const double uu = T::HAS_U ? st.u[gOut(q)] : 0.0;
#pragma unroll
                for (int r = 0; r < T::NDYN; ++r) {
                    const double vv = q + 1 < SPL ? st.vd[q + 1 < SPL ? q + 1 : q][r] : st.vdo[r];
                    const double axo = d.f[r][0] * fn.x[0] + d.f[r][1] * fn.x[1] + d.f[r][2] * fn.x[2] + d.beta[r] * uu - nx[dyn_tau<F>(r)];
                    const double y = Wdyn()[r] * ((axo - d.b[r]) + (vv - d.b[r]) * idelta);
                    fn.aty[0] += y * d.f[r][0]; fn.aty[1] += y * d.f[r][1]; fn.aty[2] += y * d.f[r][2];
                    if (q == SPL - 1) ytku[NG - 1] += y * d.beta[r];
                }
            }
            double px[5];
            px[0] = p_diag_node<F>(0, j, N, P) * fn.x[0];
            px[1] = 0.0;
            px[2] = p_diag_node<F>(2, j, N, P) * fn.x[2];
            if constexpr (F == F_K) {
                if (j <= N - 2) {
                    if (j >= 1) px[2] -= P.w_cr * (q > 0 ? st.x[q > 0 ? q - 1 : 0][2] : pl[2]);
                    if (j + 1 <= N - 2) px[2] -= P.w_cr * (q + 1 < SPL ? st.x[q + 1 < SPL ? q + 1 : q][2] : nf2);
                }
            }
            px[3] = P.w_s1 * fn.x[3];
            px[4] = T::NS > 1 ? P.w_s2 * fn.x[4] : 0.0;
#pragma unroll
            for (int a = 0; a < 3 + T::NS; ++a) {
                ob += fn.x[a] * px[a];
                bad |= nonfinite_bits(fn.x[a]) | nonfinite_bits(px[a] + fn.aty[a]);
                rd = fmax(rd, fabs(px[a] + fn.aty[a]));
            }
            rp = fmax(rp, fn.rp);
        }
        if constexpr (T::HAS_U) {
#pragma unroll
            for (int g = 0; g < NG; ++g)
            if (has_ctl(g)) {
                PolEvalFn fn;
                fn.v = st.vc[g]; fn.W = Wctl(); fn.cls = clsc0; fn.pc_old = st.pcc; fn.pc_new = 0; fn.idelta = idelta; fn.rp = fn.nAx = fn.nz = 0; fn.changes = 0;
                fn.x[0] = fn.x[1] = fn.x[4] = 0; fn.x[2] = st.u[g]; fn.x[3] = T::HAS_SU ? st.su : 0.0;
#pragma unroll
                for (int a = 0; a < 5; ++a) fn.aty[a] = 0;
                ctl_rows<F>(st.mkp, fn);
                pcnc = fn.pc_new; changes += fn.changes;
                fn.aty[2] += ytku[g];
                const double pxv[2] = {P.w_u * fn.x[2], T::HAS_SU ? P.w_su * fn.x[3] : 0.0};
#pragma unroll
                for (int a = 0; a < 1 + T::HAS_SU; ++a) {
                    ob += fn.x[2 + a] * pxv[a];
                    bad |= nonfinite_bits(fn.x[2 + a]) | nonfinite_bits(pxv[a] + fn.aty[2 + a]);
                    rd = fmax(rd, fabs(pxv[a] + fn.aty[2 + a]));
                }
                rp = fmax(rp, fn.rp);
            }
        }
        rp = wave_max(rp); rd = wave_max(rd); ob = wave_sum(ob);
        double chs = wave_sum((double)changes);
        bad = __any(bad) ? 1 : 0;
        if constexpr (NT > 64) {
            __syncthreads();
            double *red = S + L.ex;
            const int w = tid >> 6;
            if ((tid & 63) == 0) { red[w * 5] = rp; red[w * 5 + 1] = rd; red[w * 5 + 2] = ob; red[w * 5 + 3] = chs; red[w * 5 + 4] = bad ? 1.0 : 0.0; }
            __syncthreads();
            ob = 0; chs = 0;
            for (int k = 0; k < NT / 64; ++k) { rp = fmax(rp, red[k * 5]); rd = fmax(rd, red[k * 5 + 1]); ob += red[k * 5 + 2]; chs += red[k * 5 + 3]; bad |= red[k * 5 + 4] != 0.0; }
            __syncthreads();
        }
        PolRes R = {rp, rd, 0.5 * ob, (int)chs, bad};
        return R;
    }

// ==================== [output] ====================
// members of Fast, part 12 and last: output_pass, the map from the solution to what the caller gets (the reference's getOptimizedPath): per point
// x, y, heading, curvature / steering and the running arc length into in.out_states [N][5], and the raw QP solution into in.out_x when asked.  Every instantiation.
//   LDS     the [N][2] points and [N] segment lengths lie at bz: the rhs / solution region of the single-level mapping, the scan tables (phi) of the two-level one —
//           both dead once the last solve has run, so this is the LAST thing a kernel does with its LDS
//   lanes   reads st.x, st.u, st.su; writes nothing
//   called  by solve_body (unless a Newton launch follows and writes the outputs itself: DevBatch::nw_follows), the Newton kernels and polish_kernel ([kernels])
    // ---- output pass: getOptimizedPath ----
    __device__ __forceinline__ void output_pass(const LS &st) const {
        double *out = in.out_states + po * 5;
        // the reference point of every own stage FIRST, all loads in flight together: read where they are used, each of the 3 SPL loads waited out a round trip of its own
        // (the compiler cannot move a load above the stores to `out`, which may alias) — 38 k cycles per path and pass with the two trigonometric calls per stage
        double rz[SPL], rx[SPL], ry[SPL];
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            const size_t at = po + (j < N ? j : 0);
            rz[q] = in.ref_z[at]; rx[q] = in.ref_x[at]; ry[q] = in.ref_y[at];
        }
        for (int i = 5 * N + tid; i < 5 * in.N; i += NT) out[i] = 0.0;  // ragged batch: rows beyond this path's length
        double *pxy = S + L.bz;  // [N][2] scratch
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j >= N) continue;
            const double ey = st.x[q][0], ephi = st.x[q][1];
            const double ang = rz[q];
            const double na = wrap_angle(ang + kPi2);
            double sn, cn;
            sincos(na, &sn, &cn);  // (one argument reduction for both; the same bits as sin() and cos(): the library's three entry points share reduction and kernels)
            const double tx = rx[q] + __dmul_rn(ey, cn);
            const double ty = ry[q] + __dmul_rn(ey, sn);
            pxy[2 * j] = tx; pxy[2 * j + 1] = ty;
            out[5 * j + 0] = tx; out[5 * j + 1] = ty; out[5 * j + 2] = ang + ephi;
            if constexpr (F != F_K) out[5 * j + 3] = st.x[q][2];
            else if (j < N - 1) out[5 * j + 3] = st.x[q][2];
            if constexpr (F == F_K) { if (j == N - 2) out[5 * (N - 1) + 3] = st.x[q][2]; }  // last point re-uses the last control
        }
        __syncthreads();
        // arc length: the segment lengths |p_j - p_{j-1}| on the lanes that own stage j (the square root is what costs: ~35 instructions per point, 44 k cycles of ONE lane
        // for N = 200 when the whole recursion ran on lane 0 — in the warm start AND in the Newton kernel of every path), then the running sum on one lane, in path order
        // like the reference: the additions are what has to be sequential for s to round the same
        double *dsg = pxy + 2 * N;  // [N] (the scratch region holds 3 N + 3 / 4 N + 4 doubles: LayoutF)
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int j = stage(q);
            if (j < 1 || j >= N) continue;
            const double dx = pxy[2 * j] - pxy[2 * j - 2], dy = pxy[2 * j + 1] - pxy[2 * j - 1];
            dsg[j] = sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0;
            out[4] = 0;
            for (int j = 1; j < N; ++j) {
                s += dsg[j];
                out[5 * j + 4] = s;
            }
        }
        if (in.out_x) {
            double *ox = in.out_x + (size_t)b * in.n;
            for (int i = tid; i < in.n; i += NT) ox[i] = 0.0;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < SPL; ++q) {
                const int j = stage(q);
                if (j >= N) continue;
                if constexpr (F == F_K) {
                    ox[2 * j] = st.x[q][1]; ox[2 * j + 1] = st.x[q][0];
                    if (j < N - 1) ox[2 * N + j] = st.x[q][2];
                    ox[3 * N - 1 + j] = st.x[q][3];
                } else {
                    ox[3 * j] = st.x[q][0]; ox[3 * j + 1] = st.x[q][1]; ox[3 * j + 2] = st.x[q][2];
                    ox[3 * N + C + j] = st.x[q][3];
                    if constexpr (F == F_KPC) ox[3 * N + C + N + j] = st.x[q][4];
                }
            }
            if constexpr (T::HAS_U) {
#pragma unroll
                for (int g = 0; g < NG; ++g)
                    if (has_ctl(g)) { ox[3 * N + cidx(g)] = st.u[g]; if constexpr (T::HAS_SU) ox[3 * N + C + 2 * N + cidx(g)] = st.su; }
            }
        }
    }

};

// ==================== [loops] ====================
// after the struct, part 1: the two drivers that sequence Fast's passes for one path.  Free function templates on a Fast object and its lane state (not
// members: each kernel instantiates the one loop variant it needs).  They touch LDS and the lane state only through the passes; what they own are the wave-uniform
// scalars of the iteration (rho, counters, thresholds), kept in scalar registers with uni().
//   admm_loop<UNI, RESUME>                  every instantiation: factor, then per iteration rhs -> solve -> update (PO_FRESH_LANE_ID before each), residuals and OSQP's
//                                           termination / infeasibility tests every check_every, rho adaptation with rescale + refactorisation.  Called by solve_body
//   refine_phase_newton<.., PH, NFIX, CK>   TWO only: the semismooth Newton refinement — per step reclass, residuals, [refactorise], Newton right-hand side, solve,
//                                           exact line search, step; multiplier updates outside.  Called by the Newton kernels (PH 1 / 2: parks / resumes a path
//                                           through park[] and st.pc*) and by solve_body<REF = 2> (PH 0).  Sets fx.nw_req for its duration (Fast::eq_step)
// Dev switches that live here: PO_MARK labels (PO_MARKS builds), PO_NW_TRACE / PO_NW_TRACE_QUIET (cycle buckets through PO_NW_TICK, local to refine_phase_newton and
// #undef'd at its end; the factorisation's buckets come from Fast::dbgc).
//
// The ADMM loop of one path.  UNI (two-level mapping only): every lane's rows have the same class pattern — the passes then take the per-row
// steps and the slack-elimination data as wave-uniform numbers from LDS, and the per-lane copies (st.cls, st.hi, st.hv) are dead for the
// whole loop, which takes ~30 VGPRs off a kernel that sits at the 512-register limit.
struct LoopOut { int status, it, nref; double rho; Resid R; };
constexpr int kStatusSolvedOutOfIters = 2;  // admm_loop only: a round below eps ran out of iterations on a point that still meets the caller's eps — solved, no further refinement (the caller turns it into PO_STATUS_SOLVED)
constexpr int kStatusRestoreEntry = 3;  // admm_loop only: a round below eps ran out of iterations on a point that FAILS the caller's eps (ADMM residuals are not monotone): the caller
                                        // returns the point the round started from — it met eps in the round before — as PO_STATUS_SOLVED, not certified
// RESUME (kernels with the refinement phase, po_params.refine_rounds > 1): continue from `prev` (iteration count, rho, refactorisation count) with the
// termination thresholds scaled by eps_mul; the state is the one the refinement left, re-expressed for the type-based step vector.
template <bool UNI, bool RESUME, int F, int SPL, int NT, bool TWO, int NWX, int NFIX>
__device__ __forceinline__ LoopOut admm_loop(Fast<F, SPL, NT, TWO, NWX, NFIX> &fx, typename Fast<F, SPL, NT, TWO, NWX, NFIX>::LS &st, const DevBatch &in, const DevParams &P, long long tc[3], long long ph[8],
                                             double eps_mul = 1.0, bool resume = false, int it0 = 0, int nref0 = 0, double rho_prev = 0.0) {
    // (rho is wave-uniform and alive for the whole solve: scalar registers — uni(), po_device.hpp)
    double rho = uni(fmin(fmax(P.rho0, kRhoMin), kRhoMax));
    if constexpr (RESUME) { if (resume) rho = uni(rho_prev); eps_mul = uni(eps_mul); }
    const long long tf0 = in.dbg_cycles != nullptr ? __builtin_readcyclecounter() : 0;
    if constexpr (TWO) { fx.template factor_blocks_two<UNI>(st, rho); }
    else { fx.factor_blocks(st, rho); }
    const long long tf1 = in.dbg_cycles != nullptr ? __builtin_readcyclecounter() : 0;
    if constexpr (TWO) { fx.factor_chain_two(st, rho); }
    else { fx.factor_chain(); }
    if (in.dbg_cycles != nullptr) { ph[6] = tf1 - tf0; ph[7] = (long long)__builtin_readcyclecounter() - tf1; }  // dev: cycles of the first factorisation (blocks, chain)
    int status = PO_STATUS_UNSOLVED, it = 0, nref = 0;
    if constexpr (RESUME) { if (resume) { it = it0; nref = nref0 + 1; } }
    Resid R = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const bool prof = in.dbg_cycles != nullptr;
    for (it = it + 1; it <= P.max_iter; ++it) {
        const bool first = (it == 1);
        // The lane id goes through an empty asm at the start of each of the three passes: everything derived from it (per-stage predicate
        // masks, LDS addresses) is then recomputed per pass (a v_cmp / v_add each) instead of being hoisted out of the iteration loop, where
        // it overflowed the SGPR file and came back through v_readlane reloads (SGPR spills 260 -> 193; 126 -> 132 M path-iterations/s).
        PO_FRESH_LANE_ID(fx);
        long long t0 = prof ? __builtin_readcyclecounter() : 0;
        PO_MARK("rhs_begin");
        if constexpr (TWO) {
            if (first) fx.template rhs_pass_two<UNI, true>(st, rho);
            else { PO_MARK("rhs_hot"); fx.template rhs_pass_two<UNI, false>(st, rho); PO_MARK("rhs_hot_end"); }
        } else fx.rhs_pass(st, rho, first);
        long long t1 = prof ? __builtin_readcyclecounter() : 0;
        PO_MARK("solve_begin");
        PO_FRESH_LANE_ID(fx);
        if constexpr (NWX == 2 || NWX == 3) fx.solve_split(st, rho);
        else if constexpr (TWO) fx.solve_two(st, rho, prof ? ph : nullptr); else fx.chain_solve();
        PO_MARK("update_begin");
        PO_FRESH_LANE_ID(fx);
        long long t2 = prof ? __builtin_readcyclecounter() : 0;
        const bool can_check = P.check_every > 0 && (it % P.check_every == 0);
        typename Fast<F, SPL, NT, TWO, NWX, NFIX>::Cert cert = {0, 0, 0};
        if constexpr (TWO) {
            if (can_check) cert = fx.template update_pass_two<true, false, UNI>(st, rho, first);
            else if (first) (void)fx.template update_pass_two<false, true, UNI>(st, rho, true);
            else { PO_MARK("upd_hot"); (void)fx.template update_pass_two<false, false, UNI>(st, rho, false); PO_MARK("upd_hot_end"); }
        }
        else { if (can_check) cert = fx.template update_pass<true>(st, first, rho); else (void)fx.template update_pass<false>(st, first, rho); }
        long long t3 = prof ? __builtin_readcyclecounter() : 0;
        tc[0] += t1 - t0; tc[1] += t2 - t1; tc[2] += t3 - t2;
        PO_MARK("update_end");
        const bool can_adapt = P.adapt_every > 0 && (it % P.adapt_every == 0);
        if (can_check || can_adapt || it == P.max_iter) {
            if constexpr (TWO) R = fx.template residual_pass_two<UNI>(st, rho); else R = fx.residual_pass(st, rho);
            // a NaN / Inf anywhere in the iterate (non-finite inputs from the caller, a degenerate factorisation): never "solved" (checked at every
            // residual evaluation, before the convergence test, which cannot see it)
            if (R.bad) { status = PO_STATUS_NON_FINITE; break; }
            if (can_check || it == P.max_iter) {
                double eps_p = P.eps_abs + P.eps_rel * fmax(R.nAx, R.nz);
                double eps_d = P.eps_abs + P.eps_rel * fmax(R.nPx, R.nAty);
                if constexpr (RESUME) { eps_p *= eps_mul; eps_d *= eps_mul; }
                if (R.rp < eps_p && R.rd < eps_d) { status = PO_STATUS_SOLVED; break; }
                // OSQP is_primal_infeasible (q = 0 rules the dual certificate out); scaling constants cancel except
                // in the non-degeneracy test (DESIGN.md §4)
                if (can_check && !(R.rp < eps_p) && fx.sc[kScC] * cert.ndy > P.eps_pinf && cert.sup < -P.eps_pinf * cert.ndy &&
                    cert.natdy < P.eps_pinf * cert.ndy) { status = PO_STATUS_PRIMAL_INFEASIBLE; break; }
            }
            if (can_adapt) {
                // OSQP compute_rho_estimate works on the SCALED residuals / norms
                const double pr = R.rps / (fmax(R.nAxs, R.nzs) + 1e-10);
                const double dr = R.rds / (fmax(R.nPxs, R.nAtys) + 1e-10);
                double rn = rho * sqrt(pr / (dr + 1e-10));
                rn = fmin(fmax(rn, kRhoMin), kRhoMax);
                if (rn > rho * P.adapt_tol || rn < rho / P.adapt_tol) {
                    fx.template rescale_pass<UNI>(st, rho / rn);
                    rho = uni(rn);
                    if constexpr (TWO) { fx.template factor_blocks_two<UNI>(st, rho); fx.factor_chain_two(st, rho); }
                    else { fx.factor_blocks(st, rho); fx.factor_chain(); }
                    ++nref;
                }
            }
        }
    }
    if (it > P.max_iter) {
        it = P.max_iter;
        if (status == PO_STATUS_UNSOLVED) {
            status = PO_STATUS_MAX_ITER;
            if constexpr (RESUME) {
                // a round below eps (refine_extra_rounds) out of iterations: the path met the caller's eps in the last regular round; if the point it ends on (R: the
                // residuals of iteration max_iter, always evaluated) still passes OSQP's test at that eps it is solved — not certified, and no further refinement
                // runs (oracle: `exhausted`).  Out here, not in the loop: the hot loop's register allocation stays what it was.
                if (eps_mul < 1.0) status = (R.rp < P.eps_abs + P.eps_rel * fmax(R.nAx, R.nz) && R.rd < P.eps_abs + P.eps_rel * fmax(R.nPx, R.nAty)) ? kStatusSolvedOutOfIters : kStatusRestoreEntry;
            }
        }
    }
    LoopOut o = {status, it, nref, rho, R};
    return o;
}

struct RefineOut { bool take, stop; int it, nfac; Resid R; bool parked; };
// Sliced Newton launches (DevBatch::nw_phase; scheduling only, the arithmetic and its order are unchanged): what the phase keeps besides the lane state when it PARKS a path
// after DevParams::ref_nw_slice steps, and picks up again in the second launch.  [0] rb, [1] nw_req, [2] pri_outer, [3] nouter, [4] it2, [5] nfinal, [6] nfac, [7] certified, [8] nstag, [9] quiet, [10] rd_prev
constexpr int kNwParkScalars = 12;
// STAGNATION: full Newton steps on an unchanged factorisation (`quiet`: where the method converges quadratically) that do not even halve the dual residual, in a row, before an attempt
// gives up — the residual sits on a floor the method cannot get under (rounding of rho_eq (a.x - b) under extreme weights; a flat valley damped by the proximal terms).  The attempt
// ends uncertified like one out of steps, the rounds go on.  Without it such an attempt burns refine_newton_max = 300 steps in every round (oracle: PO_NW_STAGNATION).
constexpr int kNwStagnation = 8;
// Refinement, po_params.refine = 2: semismooth Newton on the augmented Lagrangian with an exact line search (Fast: NEWTON REFINEMENT; the oracle's
// `refine == 2` block is the same sequence of operations).  Contract: st is a lane state filled from the stored solved
// point (load() + state_io), on return st.cls* hold the row classes of the bounds and v is expressed for the type-based step vector at rho_solve.
// PH: 0 the whole phase; 1 first of the two sliced launches (parks); 2 second (resumes) — compile-time, each with its own register allocation (one body with both
// at run time: 77 -> 207 spilled VGPRs, the launch 3.8 -> 4.9 ms)
// CK (fixed lengths only; DESIGN.md section 36): the row classes BY TYPE that every pass of the phase decodes are compile-time constants — all stage-local rows
// inequalities, KP's control row free; the caller has checked that the path's classes are those (newton_kernel_std).  The end rows keep their run-time class.  The
// same operations on the same numbers: only the class tests fold.
template <int F, int SPL, int NT, int NWX, int PH = 0, int NFIX = 0, bool CK = false>
__device__ __forceinline__ RefineOut refine_phase_newton(Fast<F, SPL, NT, true, NWX, NFIX> &fx, typename Fast<F, SPL, NT, true, NWX, NFIX>::LS &st, const DevParams &P, double rho_solve, double rp0, double rd0,
                                                         int slice = 0, double *park = nullptr, int *park_key = nullptr) {
    constexpr bool resume = PH == 2;
    if constexpr (PH != 1) slice = 0;
    // slice > 0: after that many steps the path is PARKED (lane state and factor classes stay in st, the scalars go to park[], *park_key = how long it is expected to go on);
    // resume: the phase continues a parked path (st loaded by the caller, scalars from park[]).  Neither changes a number the phase computes.
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
#pragma unroll
        for (int s = 0; s < FormTraits<F>::NS; ++s) { st.hi[q][s] = 0; st.gs[q][s] = 0; st.hv[q][s][0] = st.hv[q][s][1] = st.hv[q][s][2] = 0; }
    }
    st.hiu = st.hus = st.gsu = 0;
    static_assert(!CK || (NFIX > 0 && F == F_KP), "constant row classes: the fixed-length KP kernels only");
    fx.bound_classes(st);
    unsigned cls0[SPL];
#pragma unroll
    for (int q = 0; q < SPL; ++q) cls0[q] = st.cls[q];
    const unsigned clse0 = st.clse, clsc0 = st.clsc;
    // CK: reclass_pass and nw_reexpress_pass get the constants (cls_k, clsc_k) in place of the run-time classes by type.  The direction pass and the line search do NOT:
    // with the constants their surviving rows were compiled with other multiply-add contractions and config 3 differed from the parent's results (DESIGN.md section 36)
    unsigned cls_std[SPL];
#pragma unroll
    for (int q = 0; q < SPL; ++q) cls_std[q] = kStdClsLoc;
    const unsigned *const cls_k = CK ? cls_std : cls0;
    const unsigned clsc_k = CK ? kStdClsCtl : clsc0;
    // (every scalar the phase carries from step to step is WAVE-UNIFORM and is kept in scalar registers on purpose: uni(), po_device.hpp)
    double rb = uni(fmin(fmax(P.ref_nw_rho, kRhoMin), kRhoMax)), pri_outer = -1.0;
    rho_solve = uni(rho_solve); rp0 = uni(rp0); rd0 = uni(rd0);
    fx.nw_req = uni(P.ref_nw_rho_eq);  // the equality rows' penalty for every pass of the phase (Fast::eq_step); grows only when the multiplier updates stall (refine_newton_rho_eq_max)
    int nfac = 0, it2 = 0, nouter = 0, nfinal = 0, nsmall = 0, nstag = 0;
    bool stop = false, dirty = true, certified = false, parked = false, refac_uncounted = false, quiet = false;
    double rd_prev = -1.0;
    bool first_pass = true;
    unsigned clsf[SPL], clsef = 0, clscf = 0;  // the row classes of the current factorisation
#pragma unroll
    for (int q = 0; q < SPL; ++q) clsf[q] = 0;
    if constexpr (resume) {  // the factorisation itself is gone (LDS): it is rebuilt before the next step, and counted only if the classes changed as well
        rb = uni(park[0]); fx.nw_req = uni(park[1]); pri_outer = uni(park[2]); nouter = uni((int)park[3]); it2 = uni((int)park[4]); nfinal = uni((int)park[5]); nfac = uni((int)park[6]);
        certified = uni((int)(park[7] != 0.0)) != 0;
        nstag = uni((int)park[8]); quiet = uni((int)(park[9] != 0.0)) != 0; rd_prev = uni(park[10]);
#pragma unroll
        for (int q = 0; q < SPL; ++q) clsf[q] = st.pc[q];
        clsef = st.pce; clscf = st.pcc;
        dirty = false; refac_uncounted = true;
    }
    Resid R = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#ifdef PO_NW_TRACE  // dev: cycles per part of the phase, path 0 (tools/newton_trace.py)
    long long tcy[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = __builtin_readcyclecounter();
    int nev = 0;
#define PO_NW_TICK(i) { const long long n_ = __builtin_readcyclecounter(); tcy[i] += n_ - tlast; tlast = n_; }
#else
#define PO_NW_TICK(i)
#endif
    PO_FRESH_LANE_ID(fx);
    if constexpr (!resume) fx.nw_reexpress_pass(st, rho_solve / rb, kRhoEqOverIneq * rho_solve / fx.nw_req, cls_k, clse0, clsc_k);  // w = a.x + y / rho_i with the multipliers of the ADMM point
    for (;;) {
        PO_FRESH_LANE_ID(fx);
        PO_MARK("nw_reclass");
        (void)fx.reclass_pass(st, cls_k, clse0, clsc_k, rb, rb, 3);  // rows outside their bounds: class 0 (step rho), inside: class 2 (RHO_MIN)
        PO_NW_TICK(0)
        PO_MARK("nw_residual");
        R = fx.template residual_pass_two<false>(st, rb);                      // (x, z = clip(w), y = rho (w - z)): the dual residual is the gradient of the merit
        R.rp = uni(R.rp); R.rd = uni(R.rd); R.obj = uni(R.obj);                // (carried to the next step — pri_outer, rd_prev — and out of the phase)
        PO_NW_TICK(1)
        PO_MARK("nw_test");
        if (R.bad) break;
        const double tol_d = P.ref_eps + P.ref_eps * fmax(R.nPx, R.nAty);
        const bool dual_ok = R.rd < tol_d;
        stop = dual_ok && R.rp < P.ref_eps + P.ref_eps * fmax(R.nAx, R.nz);
        // po_params.refine_newton_final: from the certified point Newton steps go on (tight line search) until the dual residual — the gradient of the merit — sits 1e3 x below its
        // tolerance, at most that many steps
        // (round 5) `stop` is the test on THIS point — the points the correction steps produce included —, so status_refine = 1 always describes the point that is returned; a
        // correction step that leaves the test's region (one that changes the active set can land with a larger dual residual) sends the path back to the regular iteration
        // (a RESUMED path re-evaluates the residual of the point it was parked at: that evaluation was counted before the park — nstag, rd_prev come from park[] — and
        //  counting it again would end a quiet attempt after kNwStagnation - 1 non-halving steps instead of kNwStagnation: ADVICE r5)
        if (!(resume && first_pass)) {
            if (quiet && rd_prev >= 0.0 && R.rd > 0.5 * rd_prev) ++nstag; else nstag = 0;
            rd_prev = R.rd;
        }
        first_pass = false;
        if (stop) {
            if (P.ref_nw_final <= 0 || R.rd < 1e-3 * tol_d || nfinal >= P.ref_nw_final) break;
            certified = true;
        } else {
            certified = false;
            if (it2 >= P.ref_nw_max) break;
            if (nstag >= kNwStagnation) break;
            if constexpr (PH == 1) { if (it2 >= slice) { parked = true; break; } }  // (first launch of a sliced pair: every path stops here at the latest)
        }
        if (!certified && dual_ok) {  // the inner problem is solved: multiplier update; one that did not cut the primal residual by 4 raises the penalty 10 x
            if (++nouter > 50) break;
            double ratio = 1.0, ratio_eq = 1.0;
            if (pri_outer >= 0.0 && R.rp > 0.25 * pri_outer) {
                // (a long stall — a degenerate optimum — raises both caps: po_params.refine_newton_escalate)
                const double esc = P.ref_nw_esc > 0 && nouter >= P.ref_nw_esc ? (nouter >= 2 * P.ref_nw_esc ? 100.0 : 10.0) : 1.0;
                // (the escalated caps stay inside what every other pass clamps to: kRhoMax for the inequality rows, 1e8 for the equality rows)
                if (rb * 10.0 <= fmin(P.ref_nw_rho_max * esc, kRhoMax)) { ratio = 0.1; rb = uni(rb * 10.0); dirty = true; }
                else if (fx.nw_req * 10.0 <= fmin(P.ref_nw_rho_eq_max * esc, 1e8)) { ratio_eq = 0.1; fx.nw_req = uni(fx.nw_req * 10.0); dirty = true; }
            }
            pri_outer = R.rp;
            PO_FRESH_LANE_ID(fx);
            fx.nw_reexpress_pass(st, ratio, ratio_eq, cls_k, clse0, clsc_k);
            quiet = false;
            continue;
        }
        PO_MARK("nw_factor");
        {   // refactorise when the step vector differs from the one of the current factorisation (a class that flipped and flipped back costs nothing)
            bool diff = st.clse != clsef || (fx.has_ctl() && st.clsc != clscf);
#pragma unroll
            for (int q = 0; q < SPL; ++q) diff = diff || st.cls[q] != clsf[q];
            if (fx.block_any(diff)) dirty = true;
        }
        quiet = !dirty;  // (a factorisation rebuilt only because the path was parked does not count: the classes are those of the step before)
        if (dirty || (resume && refac_uncounted)) {
            fx.template factor_blocks_two<false>(st, rb); fx.factor_chain_two(st, rb);
            if (!resume || dirty) ++nfac;
            dirty = false; refac_uncounted = false;
#pragma unroll
            for (int q = 0; q < SPL; ++q) clsf[q] = st.cls[q];
            clsef = st.clse; clscf = st.clsc;
        }
        PO_NW_TICK(2)
#if defined(PO_NW_TRACE) && !defined(PO_NW_TRACE_QUIET)  // (QUIET: only the cycle totals at the end — the per-step line costs ~400 k cycles of printf, which land in the rhs bucket)
        if (fx.b == 0 && fx.tid == 0) printf("  dev step %d outer %d nfac %d certified %d  r_prim %.3e r_dual %.3e (tol %.3e)\n", it2, nouter, nfac, (int)certified, R.rp, R.rd, tol_d);
#endif
        PO_FRESH_LANE_ID(fx);
        PO_MARK("nw_rhs");
        fx.template rhs_pass_two<false, false, false, true>(st, rb);
        PO_NW_TICK(3)
        PO_FRESH_LANE_ID(fx);
        PO_MARK("nw_solve");
        if constexpr (NWX == 2 || NWX == 3) fx.solve_split(st, rb); else fx.solve_two(st, rb, nullptr);
        PO_NW_TICK(4)
        PO_FRESH_LANE_ID(fx);
        PO_MARK("nw_dir0");
        double c0 = 0, c1 = 0, f0i = 0, dum_ = 0;
        fx.template nw_dir_pass<0>(st, rb, 0.0, cls0, clse0, clsc0, c0, c1, f0i);
        fx.block_sum2(c0, c1);
        c0 = uni(c0); c1 = uni(c1);
        PO_NW_TICK(5)
        // exact line search: safeguarded Newton on the piecewise-linear psi'
        // psi'(0) and the first trial step t = 1 come out of ONE pass over the rows (nw_ls_eval01); the same numbers as the oracle's two evaluations
        double t = 1.0, lo = 0.0, hi = -1.0, f0 = 0.0, f = 0.0, fp = 0.0;
        PO_MARK("nw_ls_begin");
        fx.nw_ls_eval01(st, rb, cls0, clse0, clsc0, f0, f, fp);
#ifdef PO_NW_TRACE
        nev += 2;
#endif
        f0 = uni(f0 + c0); f = uni(f + (c0 + c1)); fp = uni(fp + c1);
        const bool fail = !(f0 < 0.0);
        if (!fail) {
            const double ls_tol = certified ? fmin(P.ref_ls_tol, 1e-4) : P.ref_ls_tol;  // (the final correction steps: always the tight search)
            for (int ev = 0;;) {
                if (fabs(f) <= ls_tol * fabs(f0)) break;
                if (f < 0) lo = t; else hi = t;
                double tn = fp > 0 ? t - f / fp : -1.0;
                if (!(tn > lo && (hi < 0 || tn < hi))) tn = hi < 0 ? 2.0 * t : 0.5 * (lo + hi);
                t = uni(tn);
                if (++ev >= P.ref_ls_max) break;
                fx.nw_ls_eval(st, rb, t, cls0, clse0, clsc0, f, fp);
#ifdef PO_NW_TRACE
                ++nev;
#endif
                f = uni(f + (c0 + c1 * t)); fp = uni(fp + c1);
            }
        }
        PO_MARK("nw_ls_end");
        PO_NW_TICK(6)
        if (fail) { stop = certified; break; }  // not a descent direction (rounding at the bottom of the merit): the attempt ends here — certified if it was
        double d0 = 0, d1 = 0;
        PO_MARK("nw_dir1");
        fx.template nw_dir_pass<1>(st, rb, t, cls0, clse0, clsc0, d0, d1, dum_);
        PO_MARK("nw_step_end");
        PO_NW_TICK(7)
        ++it2;
        if (certified) ++nfinal;
        quiet = quiet && t == 1.0;
        if constexpr (PH == 1) { if (t < 0.5) ++nsmall; }
    }
    if constexpr (PH == 1) if (parked) {
        // expected remaining work, longest first: a path still in its FIRST inner solve (no multiplier update yet) is where the long tails are — the more short steps it
        // took, the longer the crawl; the others have about one or two steps per remaining update left (tools/tail_sim.py, DESIGN.md section 11)
        if (fx.tid == 0) {
            park[0] = rb; park[1] = fx.nw_req; park[2] = pri_outer; park[3] = nouter; park[4] = it2; park[5] = nfinal; park[6] = nfac; park[7] = certified ? 1.0 : 0.0;
            park[8] = nstag; park[9] = quiet ? 1.0 : 0.0; park[10] = rd_prev;
            // (round 6) the key is a PREDICTION of the remaining steps, in 2/3-step buckets: [short steps so far, while still in the first inner solve] + 2 log10(r_prim) + 14 — the
            // multiplier phase takes about one step per decade of primal residual still to go.  Fitted on the oracle's traces of BASELINE config 3 and checked on config 4's
            // 8 192 other paths and on the K formulation (list-scheduling simulation on 1 024 wave slots, in steps: config 3 36.6 -> 32.4 = its longest path; K 69.6 -> 58.2 of 55.0;
            // round 5's 4-bit key: first-inner flag + short steps, else 7 - updates).  kNwKeys = 32 buckets.
            const float kf = (nouter == 0 ? (float)nsmall : 0.0f) + 2.0f * __log10f((float)fmax(R.rp, 1e-30)) + 14.0f;
            const int ki = (int)floorf(1.5f * kf);
            *park_key = ki < 0 ? 0 : (ki > kNwKeys - 1 ? kNwKeys - 1 : ki);
        }
#pragma unroll
        for (int q = 0; q < SPL; ++q) st.pc[q] = clsf[q];
        st.pce = clsef; st.pcc = clscf;
        fx.nw_req = 0.0;
        RefineOut o = {false, false, it2, nfac, R, true};
        return o;
    }
#ifdef PO_NW_TRACE
    if (fx.b == 0 && fx.tid == 0)
        printf("  dev newton: %d steps %d fac %d outer %d ls evals; cycles: reclass %lld residual %lld factor %lld (pivots %lld phi %lld tables %lld) rhs %lld solve %lld dir0 %lld ls %lld dir1 %lld\n", it2, nfac, nouter, nev,
               tcy[0], tcy[1], tcy[2], fx.dbgc[0], fx.dbgc[1], fx.dbgc[2], tcy[3], tcy[4], tcy[5], tcy[6], tcy[7]);
#endif
#undef PO_NW_TICK
    (void)fx.reclass_pass(st, cls_k, clse0, clsc_k, rb, rho_solve, 2, fx.nw_req, kRhoEqOverIneq * rho_solve);
    fx.nw_req = 0.0;
    RefineOut o = {!R.bad && (stop || (R.rp <= rp0 && R.rd <= rd0)), stop && !R.bad, it2, nfac, R, false};
    return o;
}

// ==================== [kernels] ====================
// after the struct, part 2: the kernels.  Each builds one Fast object per workgroup (= per path), load()s the lane state, zeroes its LDS, copies the
// equilibration block (scale_to_lds) and runs a loop of [loops]; po_solve_form.hip instantiates them per shape, po_kernels.hip launches them.
//   solve_kernel_fast (solve_body<REF = 0>)    every F / TWO / NWX / NFIX; load -> [classify] -> admm_loop -> state block (when a Newton / polish launch follows) -> outputs
//   newton_kernel, newton_kernel_std           TWO; the text is po_newton_kernel.inc, included twice below; refine_phase_newton on the state block the warm start left
//   newton_std_select_kernel                   NFIX > 0, NT 64: sorts the paths of a batch between those two by their row classes; reads the inputs only
//   newton_fallback_kernel (solve_body<REF = 2>)   TWO, general variant: the later rounds of what a Newton launch handed back (DevBatch::fb_list)
//   polish_kernel                              TWO, NWX 1 / 4 / 5: OSQP's polish on the state block
// Global memory: in.out_info (po_info per path: status, counters, residuals — also the hand-over between the launches), in.pol_state (state_io), in.nw_state (park_io),
// in.out_states / in.out_x (output_pass, zero_outputs), in.dbg_cycles (dev).  LDS: only through the Fast object, except polish_kernel's rescaling of cst (sigma -> delta).
//
// One launch = one loop variant.  The two-level mapping is launched twice on the same stream: UNI = true solves every path whose row
// classes are uniform (all of them on BASELINE's corridors) and marks the others kStatusDeferred in out_info; UNI = false picks exactly
// those up (its other blocks leave after one 4-byte read).  Two loop variants inside ONE kernel cost more registers than either needs
// (measured: 114 -> 82 M path-iterations/s), a kernel with only the uniform variant spills 14 instead of 53 VGPRs (114 -> 122 M).

// a path that is reported without a solution (non-finite inputs): defined outputs — zeros — instead of whatever the buffers held
__device__ __forceinline__ void zero_outputs(const DevBatch &in, int b, int nt) {
    double *os = in.out_states + (size_t)b * in.N * 5;
    for (int i = threadIdx.x; i < in.N * 5; i += nt) os[i] = 0.0;
    if (in.out_x != nullptr) {
        double *ox = in.out_x + (size_t)b * in.n;
        for (int i = threadIdx.x; i < in.n; i += nt) ox[i] = 0.0;
    }
}

// REF = 0: the plain solve kernels (also the warm start of the Newton refinement: they leave state and po_info where newton_kernel / polish_kernel find them).
// REF = 2 (newton_fallback_kernel only, general variant): round `in.round` >= 1 of a path the Newton launch did not certify — the type-based iteration resumed from the
// state block at a 10 x tighter eps, then the Newton refinement again (po_params.refine_rounds / refine_extra_rounds; round 5 removed the chained-rounds queue, the
// speculative continuations, the probe launches and the refine = 1 phase that used to live here: the Newton split launches beat them on every shape, DESIGN.md §10).
template <int F, int SPL, int NT, bool TWO, bool UNI, int NWX, int REF = 0, int NFIX = 0> __device__ __forceinline__ void solve_body(const DevBatch &in, const DevParams &P, int b_given = -1) {
    static_assert(TWO || !UNI, "the single-level mapping has no uniform variant");
    static_assert(REF == 0 || (REF == 2 && TWO && !UNI), "the later rounds run on the general variant of the two-level mapping");
    static_assert(NFIX == 0 || (REF == 0 && UNI), "fixed length: the uniform warm start only");
    extern __shared__ double smem[];
    // workgroup i lands on XCD i mod 8 (a static partition of the launch): a bit-mixing bijection on [0, B) (xorshift / odd multiply on
    // perm_bits bits, cycle-walking back into range) keeps any regular pattern in the caller's path order — periodic or clustered — from
    // pinning the expensive paths to one XCD.  perm_bits == 0: blockIdx order.  All scalar.
    int b;
    const int round = in.round;
    if (b_given >= 0) b = b_given;  // (newton_fallback_kernel: the path comes from its work list)
    else b = in.order ? in.order[blockIdx.x] : perm_index(blockIdx.x, in.perm_bits, in.B);  // caller's scheduling hint, or the engine's own mixing
    if ((unsigned)b >= (unsigned)in.B) return;
    if constexpr (REF) { if (round > 0 && in.out_info[b].status != kStatusDeferred - round) return; }  // round r > 0 takes only what round r - 1 handed back
    if constexpr (TWO && !UNI) {
        if (in.only_deferred && round == 0 && in.out_info[b].status != kStatusDeferred) return;  // solved by the UNI = true launch that went before
    }
    Fast<F, SPL, NT, TWO, NWX, NFIX> fx(P, in, smem, b);
    typename Fast<F, SPL, NT, TWO, NWX, NFIX>::LS st;
    fx.load(st);
    if (fx.inputs_have_nan()) {  // block-uniform; never "solved", nothing computed: the path's outputs are zeroed (a defined value, not the buffer's previous content)
        zero_outputs(in, b, NT);
        if (fx.tid == 0) { po_info o = {PO_STATUS_NON_FINITE, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0, 0}; in.out_info[b] = o; }
        return;
    }
    if constexpr (UNI) {
        if (!fx.classify(st)) {  // block-uniform decision
            if (fx.tid == 0 && round == 0) in.out_info[b].status = kStatusDeferred;
            return;
        }
    }
    for (int i = fx.tid; i < fx.L.total; i += NT) smem[i] = 0.0;
    __syncthreads();
    fx.scale_to_lds();
    long long tc[3] = {0, 0, 0}, ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    LoopOut lo;
    int sref = 0;  // po_info.status_refine
    if constexpr (!REF) {
        lo = admm_loop<UNI, false>(fx, st, in, P, tc, ph);
        if constexpr (TWO) {  // polish / Newton refinement requested: leave the ADMM state where polish_kernel / newton_kernel (same shape) find it
            if (in.pol_state != nullptr) fx.template state_io<true>(st, in.pol_state + (size_t)b * in.pol_stride);
        }
    } else {
        // refine_rounds = R > 1: round 0 (the plain kernels + newton_kernel) stops the solve at 10^(R-1) x eps; a refinement that is not certified at refine_eps hands the
        // path back (status kStatusDeferred - (round + 1), iterate in the state block, counters in out_info) and the next round resumes the type-based iteration at a
        // 10 x tighter eps, down to eps itself, then refine_extra_rounds more below it.
        double *state = in.pol_state + (size_t)b * in.pol_stride;  // (never null here)
        const int rounds = P.ref_rounds > 1 ? P.ref_rounds : 1;
        const int rounds_total = rounds + P.ref_extra;
        double eps_mul = 1.0;
        for (int r = round + 1; r < rounds; ++r) eps_mul *= 10.0;
        for (int r = rounds; r <= round; ++r) eps_mul *= 0.1;
        // counters of the rounds before: iterations of the type-based loop (its check / adaption cadence continues) and of the refinements
        const po_info *oi0 = in.out_info + b;
        const int it0 = oi0->status_polish, nref0 = oi0->n_refactor;
        int ref_it = oi0->iters - oi0->status_polish;
        const double rho_prev = oi0->rho;
        sref = oi0->status_refine;  // the last attempt's verdict (-1): what the path reports if no later refinement runs (it ends at max_iter)
        fx.template state_io<false>(st, state);
        lo = admm_loop<UNI, true>(fx, st, in, P, tc, ph, eps_mul, true, it0, nref0, rho_prev);
        if (lo.status == kStatusRestoreEntry) {
            // a round below eps never unsolves a path: `state` still holds the point this round started from (nothing has been stored over it) and po_info its residuals
            fx.template state_io<false>(st, state);
            const po_info *oi = in.out_info + b;
            lo.R.rp = oi->r_prim; lo.R.rd = oi->r_dual; lo.R.obj = oi->obj; lo.rho = oi->rho;
            lo.status = kStatusSolvedOutOfIters;
        } else fx.template state_io<true>(st, state);
        bool hand_back = false;
        if (P.refine && lo.status == PO_STATUS_SOLVED) {
            const bool last = round + 1 >= rounds_total;
            __syncthreads();
            typename Fast<F, SPL, NT, TWO, NWX, NFIX>::LS st2;
            fx.load(st2);
            fx.template state_io<false>(st2, state);
            const RefineOut ro = refine_phase_newton<F, SPL, NT, NWX, 0, NFIX>(fx, st2, P, lo.rho, lo.R.rp, lo.R.rd);
            __syncthreads();
            // (an early return here costs the whole kernel its register allocation: a failed attempt leaves through the hand-back exit below instead)
            if (ro.take) fx.template state_io<true>(st2, state);  // else: out of iterations and not better — the solved point stays
            ref_it += ro.it; lo.nref += ro.nfac;
            if (ro.take) lo.R = ro.R;
            sref = ro.stop ? 1 : -1;
            hand_back = !ro.stop && !last;
            __syncthreads();
            fx.template state_io<false>(st, state);
        }
        if (hand_back) {
            if (fx.tid == 0) {
                po_info *oi = in.out_info + b;
                oi->status = kStatusDeferred - (round + 1); oi->iters = lo.it + ref_it; oi->status_polish = lo.it; oi->n_refactor = lo.nref;
                oi->r_prim = lo.R.rp; oi->r_dual = lo.R.rd; oi->rho = lo.rho; oi->obj = lo.R.obj; oi->status_refine = sref;
            }
            return;
        }
        if (lo.status == kStatusSolvedOutOfIters) lo.status = PO_STATUS_SOLVED;
        lo.it += ref_it;
    }
    // (a split solve: newton_kernel follows and writes the outputs of every path reported SOLVED here — the map costs 8 sin / cos per lane and a sequential sum)
    bool outputs_later = false;
    if constexpr (!REF) outputs_later = in.nw_follows != 0 && lo.status == PO_STATUS_SOLVED;
    if (!outputs_later) fx.output_pass(st);
    if (fx.tid == 0) {
        po_info o;
        o.status = lo.status; o.iters = lo.it; o.n_refactor = lo.nref; o.status_polish = 0;
        o.r_prim = lo.R.rp; o.r_dual = lo.R.rd; o.rho = lo.rho; o.obj = lo.R.obj;
        o.status_refine = sref; o.reserved = 0;
        in.out_info[b] = o;
        if (in.dbg_cycles != nullptr) { long long *d = in.dbg_cycles + (size_t)b * 16; d[0] = tc[0]; d[1] = tc[1]; d[2] = tc[2]; d[3] = lo.it; for (int i = 0; i < 8; ++i) d[4 + i] = ph[i]; d[12] = UNI ? 1 : 0; }
    }
}
template <int F, int SPL, int NT, bool TWO, bool UNI, int NWX = 1, int NFIX = 0> __global__ PO_KERNEL_ATTR __launch_bounds__(NT) void solve_kernel_fast(DevBatch in, DevParams P) {
    solve_body<F, SPL, NT, TWO, UNI, NWX, 0, NFIX>(in, P);
}

// OSQP's polish on the paths the solve kernels reported solved (po_params.polish; launched after both loop variants, same shape and LDS layout).
// polish.c: one reduced KKT solve with `refine` steps of iterative refinement, adopted when polish_successful's residual test holds.
template <int F, int SPL, int NT, int NWX = 1> __global__ PO_KERNEL_ATTR __launch_bounds__(NT) void polish_kernel(DevBatch in, DevParams P0) {
    static_assert(NWX == 1 || NWX == 4 || NWX == 5, "polish: one lane per chunk (one or several groups per lane)");
    using FX = Fast<F, SPL, NT, true, NWX>;
    extern __shared__ double smem[];
    const int b = in.order ? in.order[blockIdx.x] : perm_index(blockIdx.x, in.perm_bits, in.B);  // caller's scheduling hint, or the engine's own mixing
    if ((unsigned)b >= (unsigned)in.B) return;
    if (in.out_info[b].status != PO_STATUS_SOLVED) return;  // like OSQP: only a solved problem is polished
    DevParams P = P0;
    P.alpha = 1.0;  // iterative refinement = the same recursion without relaxation
    FX fx(P, in, smem, b);
    typename FX::LS st;
    fx.load(st);
    for (int i = fx.tid; i < fx.L.total; i += NT) smem[i] = 0.0;
    __syncthreads();
    fx.scale_to_lds();
    if (fx.tid < kNVC) smem[fx.L.cst + kScSig + fx.tid] *= P.pol_delta / P.sigma;  // sigma / (c D^2) -> delta / (c D^2): delta I on the scaled problem
    __syncthreads();
    fx.template state_io<false>(st, in.pol_state + (size_t)b * in.pol_stride);
    unsigned cls0[SPL];
#pragma unroll
    for (int q = 0; q < SPL; ++q) cls0[q] = st.cls[q];
    const unsigned clse0 = st.clse, clsc0 = st.clsc;
    fx.pol_init(st);
#pragma unroll
    for (int q = 0; q < SPL; ++q) st.cls[q] = kPolAllEq;
    st.clse = st.clsc = kPolAllEq;
    const double rho = 1.0 / (P.pol_delta * kRhoEqOverIneq);  // the passes use rho_eq = 1e3 rho on equality rows: rho_eq = 1 / delta
    PolRes R = {0, 0, 0, 1, 0};
    {
        fx.pol_reset(st);
        fx.template factor_blocks_two<false, true>(st, rho);
        fx.factor_chain_two(st, rho);
        for (int it = 0; it <= P.pol_refine; ++it) {
            PO_FRESH_LANE_ID(fx);
            fx.template rhs_pass_two<false, false, true>(st, rho);
            PO_FRESH_LANE_ID(fx);
            fx.solve_two(st, rho, nullptr);
            PO_FRESH_LANE_ID(fx);
            (void)fx.template update_pass_two<false, false, false, true>(st, rho, false);
        }
        unsigned pcn[SPL], pcne, pcnc;
        R = fx.pol_eval(st, cls0, clse0, clsc0, P.pol_delta, pcn, pcne, pcnc);
    }
    // polish_successful (polish.c)
    po_info *oi = in.out_info + b;  // (fields read and written one by one, late: a po_info held in registers across the kernel is spilled)
    const double rp0 = oi->r_prim, rd0 = oi->r_dual;
    const bool ok = !R.bad && ((R.rp < rp0 && R.rd < rd0) || (R.rp < rp0 && rd0 < 1e-10) || (R.rd < rd0 && rp0 < 1e-10));
    if (ok) fx.output_pass(st);
    if (fx.tid == 0) {
        oi->status_polish = ok ? 1 : -1;
        if (ok) { oi->r_prim = R.rp; oi->r_dual = R.rd; oi->obj = R.obj; }
    }
}

// newton_fallback_kernel: the later rounds of the paths whose round-0 Newton attempt was not certified (rare: no path of the BASELINE batches).
// newton_kernel appends such a path to a
// device-side work list (DevBatch::fb_list: count, then path ids); this kernel is launched with a SMALL fixed grid (kFallbackGrid workgroups) that walks the list, each
// path through its rounds one after the other in the general-variant body of the kernels with the phase (solve_body<..., REF = 2>, non-chained: it picks the path up by
// its hand-back status).  Why not B workgroups that look at their own path's status and leave: a kernel's launch cost grows with its private segment, and the loops
// around the body put this one at 1.2 KB per lane — measured 0.51 ms for 4096 workgroups that do nothing (the plain general kernel, 192 B: 4 us), 7 % of the whole solve.
// Why not inside newton_kernel: tried as a cold __noinline__ call there — 4 KB of scratch per lane, the Newton launch 6.6 -> 10.8 ms.  A batch on which MANY paths fall
// back (a starved refine_newton_max) runs them kFallbackGrid at a time: slow, correct, and not what the setting is for.
constexpr int kFallbackGrid = 256;
template <int F, int SPL, int NT, int NWX = 1> __global__ PO_KERNEL_ATTR __launch_bounds__(NT) void newton_fallback_kernel(DevBatch in, DevParams P) {
    const int count = in.fb_list[0];
    const int rounds = P.ref_rounds > 1 ? P.ref_rounds : 1, rounds_total = rounds + P.ref_extra;
    DevBatch rb = in;
    rb.only_deferred = 0;
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
        const int b = in.fb_list[1 + i];
        for (int r = 1; r < rounds_total; ++r) {
            __threadfence();
            __syncthreads();  // po_info and the state block of the round before are visible to every wave of the workgroup
            rb.round = r;
            solve_body<F, SPL, NT, true, false, NWX, 2>(rb, P, b);
        }
        __syncthreads();
    }
}

// newton_kernel — po_params.refine = 2: the Newton refinement of round 0 as a KERNEL OF ITS OWN.  The plain solve kernels (no refinement phase in them: their own
// register allocation) run the short type-based warm start of every path — all paths take the same 25 .. 50 iterations, so that launch has no tail — and leave state
// and po_info as for a polish; this kernel picks every solved path up, runs refine_phase_newton, and either finishes it (outputs, po_info, status_refine) or hands it
// back (status kStatusDeferred - 1, iterate in the state block, counters in po_info, the path appended to DevBatch::fb_list) to newton_fallback_kernel above, which
// takes the rare path that was not certified through the later rounds.  The phase is compiled alone: no ADMM hot loop shares its registers.
// The kernel's text is po_newton_kernel.inc: newton_kernel, and newton_kernel_std — the Newton launches of a fixed length with the STANDARD row classes as compile-time
// constants (DESIGN.md section 36): every stage-local row an inequality, KP's control row free, which is every path with positive margin and kmax and non-degenerate
// corridors.  Which paths those are is decided by newton_std_select_kernel (below) in a launch of its own; the engine hands newton_kernel_std the standard paths and
// newton_kernel of the same phase and length the others, right behind it (std_lists, po_device.hpp).  (The test at the entry of newton_kernel_std itself was tried
// first: with nothing else changed the kernel then computed other roundings — 3.8 of 4.1 million elements of config 3 differed from the parent's by up to 1.3e-13; DESIGN.md section 36.)
#define PO_NW_KERNEL newton_kernel
#define PO_NW_CK false
#include "po_newton_kernel.inc"
#undef PO_NW_KERNEL
#undef PO_NW_CK
#define PO_NW_KERNEL newton_kernel_std
#define PO_NW_CK true
#include "po_newton_kernel.inc"
#undef PO_NW_KERNEL
#undef PO_NW_CK
// Workgroup i looks at the path the first Newton launch gives workgroup i (the caller's order, else the engine's permutation): are its row classes by type the standard
// ones on every lane?  (load() leaves the classes of the bounds in st.cls*; one wave per path: the vote is block-uniform.)  Slot i of StdLists::order or of
// StdLists::left1 gets the path — both were filled with -1 by scale_kernel, and a first launch's workgroup leaves on -1 —, flag[path] says which, for the sort that
// splits the parked paths between the two second launches.  Reads only the inputs of the path.
template <int F, int SPL, int NT, int NFIX> __global__ PO_KERNEL_ATTR __launch_bounds__(NT) void newton_std_select_kernel(DevBatch in, DevParams P) {
    static_assert(NT == 64, "constant row classes: one wave per path");
    using FX = Fast<F, SPL, NT, true, 1, NFIX>;
    extern __shared__ double smem[];
    const int b = in.order ? in.order[blockIdx.x] : perm_index(blockIdx.x, in.perm_bits, in.B);
    if ((unsigned)b >= (unsigned)in.B) return;
    FX fx(P, in, smem, b);
    typename FX::LS st;
    fx.load(st);
    bool standard = st.clsc == kStdClsCtl;
#pragma unroll
    for (int q = 0; q < SPL; ++q) standard = standard && st.cls[q] == kStdClsLoc;
    const bool all = __all(standard) != 0;
    if (fx.tid == 0) {
        const StdLists sl = std_lists(in.nw_keys, in.B);
        (all ? sl.order : sl.left1)[blockIdx.x] = b;
        sl.flag[b] = all ? 1 : 0;  // (no count here: 4 096 atomic adds on one word made this launch 60 us instead of 18, DESIGN.md section 36 — po_debug_get sums the flags)
    }
}
