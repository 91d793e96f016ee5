// po_solve_form.hip — the kernel instantiations of ONE object of po_launch.hpp's PO_SOLVE_OBJECTS (-DPO_ENTRY=<object>): the rows of po_solve_common.hpp's table whose
// formulation and group the object holds, in the kind of kernel it holds —
//   kObjUni / kObjGen    the solve kernels, uniform-row-class / general loop variant (the general object also holds the polish kernels);
//   kObjNewton           the Newton refinement (po_params.refine = 2): newton_kernel + newton_fallback_kernel, nothing else (built with -DPO_REF=3: po_device.hpp);
//   kObjFix...           KP only: the length-specialised kernels of the headline shape (Makefile: PO_FIXED_N) — the uniform warm start / the first / the second Newton launch,
//                        and the two Newton launches with the standard row classes as compile-time constants (kObjFixNewtonStd1 / 2: newton_kernel_std; the first also holds newton_std_select_kernel).
// Each object exports ONE entry, named like the object.  The dispatcher (po_kernels.hip) has resolved the shape and its LDS bytes and calls the one object that holds the
// row; the entry launches the instance that EQUALS the shape, and answers hipErrorNotSupported when it has none.  -DPO_DEV_HEADLINE (dev builds only) keeps just one shape.
#include "po_solve_common.hpp"

#ifndef PO_ENTRY
#error "compile with -DPO_ENTRY=<an object of PO_SOLVE_OBJECTS (po_launch.hpp)>"
#endif
#define PO_STR2(x) #x
#define PO_STR(x) PO_STR2(x)

namespace {  // (unnamed: every object instantiates these templates with a body of its own, and the linker would fold same-named ones into one)
using namespace po;
struct Object { int form, kind, groups; };
constexpr bool same(const char *a, const char *b) { return *a == *b && (!*a || same(a + 1, b + 1)); }
constexpr Object me() {
#define PO_X(name, form, kind, groups) if (same(#name, PO_STR(PO_ENTRY))) return {form, kind, groups};
    PO_SOLVE_OBJECTS(PO_X)
#undef PO_X
    return {-1, -1, 0};
}
static_assert(me().form >= 0, "PO_ENTRY names no object of PO_SOLVE_OBJECTS");
constexpr bool newton_object(int kind) { return kind == kObjNewton || kind == kObjFixNewton1 || kind == kObjFixNewton2 || kind == kObjFixNewtonStd1 || kind == kObjFixNewtonStd2; }
#ifdef PO_REF
static_assert(newton_object(me().kind), "-DPO_REF=3 is for the Newton objects");
#else
static_assert(!newton_object(me().kind), "the Newton objects build with -DPO_REF=3");
#endif
// does an object of groups G instantiate this row?  (dev builds: the one shape of -DPO_DEV_SPL / NT / NWX — default BASELINE config 3 — whatever its group)
[[maybe_unused]] constexpr bool holds(int G, bool two, int spl, int nt, int nwx, int g) {
#ifdef PO_DEV_HEADLINE
#ifndef PO_DEV_SPL
#define PO_DEV_SPL 4
#endif
#ifndef PO_DEV_NWX
#define PO_DEV_NWX 1
#endif
#ifndef PO_DEV_NT
#define PO_DEV_NT 64
#endif
    return two && spl == PO_DEV_SPL && nt == PO_DEV_NT && nwx == PO_DEV_NWX;
#else
    return (G & g) != 0;
#endif
}
// K is one of: solve (UNI or not), Newton phase 1 / 2, fallback, polish.  F and G are template parameters so that every `if constexpr` below is DEPENDENT: a row the
// object does not hold is discarded before its kernel is named, and instantiates nothing.
template <int F, int G, bool UNI> hipError_t launch_rows(int launch, const Shape &s, size_t lds, const DevBatch *in, const DevParams *P, hipStream_t st) {
#define PO_X(F_, TWO_, SPL_, NT_, NWX_, G_)                                                                                                     \
    if constexpr (F == F_ && holds(G, TWO_, SPL_, NT_, NWX_, G_) && (TWO_ || !UNI)) {                                                           \
        if (is_shape(s, TWO_, SPL_, NT_, NWX_)) return launch1(&solve_kernel_fast<F, SPL_, NT_, TWO_, TWO_ && UNI, NWX_>, in, P, NT_, lds, st); \
    }
    if (launch == kLaunchSolve) { PO_SHAPE_ROWS(PO_X) }
#undef PO_X
#define PO_X(F_, TWO_, SPL_, NT_, NWX_, G_)                                                                                                     \
    if constexpr (!UNI && F == F_ && TWO_ && holds(G, TWO_, SPL_, NT_, NWX_, G_) && has_polish_kernel(Shape{NT_, SPL_, TWO_, NWX_})) {          \
        if (is_shape(s, TWO_, SPL_, NT_, NWX_)) return launch1(&polish_kernel<F, SPL_, NT_, NWX_>, in, P, NT_, lds, st);                         \
    }
    if (launch == kLaunchPolish) { PO_SHAPE_ROWS(PO_X) }
#undef PO_X
    return hipErrorNotSupported;
}
// FB: the fallback launch behind the Newton launches (newton_fallback_kernel walks the work list of the paths newton_kernel handed back; a small fixed grid)
template <int F, int G, bool FB> hipError_t launch_newton(const Shape &s, size_t lds, const DevBatch *in, const DevParams *P, hipStream_t st) {
#define PO_X(F_, TWO_, SPL_, NT_, NWX_, G_)                                                                                                     \
    if constexpr (F == F_ && TWO_ && holds(G, TWO_, SPL_, NT_, NWX_, G_)) {                                                                     \
        if (is_shape(s, TWO_, SPL_, NT_, NWX_)) {                                                                                               \
            if constexpr (FB) return launch_grid(&newton_fallback_kernel<F, SPL_, NT_, NWX_>, in, P, kFallbackGrid, NT_, lds, st);              \
            else if (in->nw_phase == 2) return launch1(&newton_kernel<F, SPL_, NT_, NWX_, 2>, in, P, NT_, lds, st);                             \
            else return launch1(&newton_kernel<F, SPL_, NT_, NWX_, 1>, in, P, NT_, lds, st);                                                    \
        }                                                                                                                                       \
    }
    PO_SHAPE_ROWS(PO_X)
#undef PO_X
    return hipErrorNotSupported;
}
// the length-specialised kernels: the dispatcher has checked is_fixed_shape; a length that is not on the list is an error
template <int F, int KIND> hipError_t launch_fixed(int launch, const DevBatch *in, const DevParams *P, size_t lds, hipStream_t st) {
#define PO_X(N_)                                                                                                                                \
    if (in->N == N_) {                                                                                                                          \
        if constexpr (KIND == kObjFixUni) return launch1(&solve_kernel_fast<F, kFixSpl, kFixNt, true, true, 1, N_>, in, P, kFixNt, lds, st);    \
        else if constexpr (KIND == kObjFixNewtonStd1) {                                                                                         \
            /* (no LDS: the kernel touches none, and with the solve's 38 KB only four of its short workgroups fit a CU) */               \
            if (launch == kLaunchStdSelect) return launch1(&newton_std_select_kernel<F, kFixSpl, kFixNt, N_>, in, P, kFixNt, 0, st);            \
            return launch1(&newton_kernel_std<F, kFixSpl, kFixNt, 1, 1, N_>, in, P, kFixNt, lds, st);                                           \
        }                                                                                                                                       \
        else if constexpr (KIND == kObjFixNewtonStd2) return launch1(&newton_kernel_std<F, kFixSpl, kFixNt, 1, 2, N_>, in, P, kFixNt, lds, st);    \
        else return launch1(&newton_kernel<F, kFixSpl, kFixNt, 1, KIND == kObjFixNewton2 ? 2 : 1, N_>, in, P, kFixNt, lds, st);                 \
    }
    PO_FIXED_LIST(PO_X)
#undef PO_X
    return hipErrorNotSupported;
}
template <int F, int KIND, int G> hipError_t entry(int launch, const Shape &s, size_t lds, const DevBatch *in, const DevParams *P, hipStream_t st) {
    if constexpr (KIND == kObjUni || KIND == kObjGen) return launch_rows<F, G, KIND == kObjUni>(launch, s, lds, in, P, st);
    else if constexpr (KIND == kObjNewton) {
        if (launch == kLaunchNewton) return launch_newton<F, G, false>(s, lds, in, P, st);
        if (launch == kLaunchFallback) return launch_newton<F, G, true>(s, lds, in, P, st);
        return hipErrorNotSupported;
    } else return launch_fixed<F, KIND>(launch, in, P, lds, st);
}
}  // namespace
extern "C" hipError_t PO_ENTRY(int launch, const po::Shape &s, size_t lds, const po::DevBatch *in, const po::DevParams *P, hipStream_t st) {
    return entry<me().form, me().kind, me().groups>(launch, s, lds, in, P, st);
}
