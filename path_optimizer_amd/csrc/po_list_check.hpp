// po_list_check.hpp — host-side check of the second sliced Newton launch's work lists (po_debug_get "newton_list_ok", po_capi.cpp).  Plain C++, no HIP: the stand-alone
// program of tests/test_fixed_classes_edges.py compiles it with the host compiler under the address and undefined-behaviour sanitizers.
//
// What nw_sort_kernel (po_kernels.hip) promises of a list (count, then path ids): every id is a parked path (keys[id] >= 0) of the batch, none twice, in descending key
// order with ties in path order; the lists hold every parked path between them.  With the constant-class kernels there are two lists, split by
// StdLists::flag (po_device.hpp): the first holds the paths with flag 1 (newton_kernel_std resumes them), the second those with flag 0 (newton_kernel).  A path on the
// wrong list would be run by the wrong kernel and still return a plausible point, so the check reads the flags too.
#pragma once
#include <cstddef>
#include <vector>

namespace po {

enum class ListFault {
    kNone = 0,
    kCount,      // a list's count is negative or above B
    kId,         // an entry is not a path of the batch
    kNotParked,  // an entry's key says "finished in the first launch"
    kDuplicate,  // a path is listed twice, on one list or on both
    kOrder,      // keys ascend, or a tie is not in path order
    kFlag,       // a flag-0 path on the first list or a flag-1 path on the second
    kMissing,    // a parked path is on no list
};

// keys [B]; list = the first (or only) list; list2 = the second list or nullptr; flag [B] or nullptr (no flag is looked at; one list: never).  The first fault in
// list order, entries before what follows them; kMissing only when every entry is in order.
inline ListFault newton_list_fault(const int *keys, const int *list, const int *list2, const int *flag, int B) {
    if (B < 0 || !keys || !list) return ListFault::kCount;
    std::vector<char> seen((size_t)B, 0);
    long long listed = 0;
    const int *const lists[2] = {list, list2};
    for (int w = 0; w < 2; ++w) {
        const int *const l = lists[w];
        if (!l) continue;
        const int n = l[0];
        if (n < 0 || n > B) return ListFault::kCount;
        for (int i = 0; i < n; ++i) {
            const int b = l[1 + i];
            if (b < 0 || b >= B) return ListFault::kId;
            if (keys[b] < 0) return ListFault::kNotParked;
            if (seen[(size_t)b]) return ListFault::kDuplicate;
            seen[(size_t)b] = 1;
            if (i > 0) {
                const int a = l[i];
                if (!(keys[a] > keys[b] || (keys[a] == keys[b] && a < b))) return ListFault::kOrder;
            }
            if (list2 && flag && flag[b] != (w == 0 ? 1 : 0)) return ListFault::kFlag;
        }
        listed += n;
    }
    long long parked = 0;
    for (int b = 0; b < B; ++b) parked += keys[b] >= 0;
    return listed == parked ? ListFault::kNone : ListFault::kMissing;
}

inline bool newton_list_ok(const int *keys, const int *list, const int *list2, const int *flag, int B) {
    return newton_list_fault(keys, list, list2, flag, B) == ListFault::kNone;
}

}  // namespace po
