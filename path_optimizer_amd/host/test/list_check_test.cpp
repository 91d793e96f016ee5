// list_check_test.cpp — stand-alone program around csrc/po_list_check.hpp (no HIP): hand-made work lists of the second sliced Newton launch, one defect each, and the
// fault the check must name for it.  tests/test_fixed_classes_edges.py builds it with the host compiler under -fsanitize=address,undefined and runs it; every list lives
// in a heap block of exactly its length, so a check that reads past a list (a count above B) is caught by the sanitizer, not by luck.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../csrc/po_list_check.hpp"

namespace {
using po::ListFault;
using V = std::vector<int>;

const char *name(ListFault f) {
    switch (f) {
    case ListFault::kNone: return "none";
    case ListFault::kCount: return "count";
    case ListFault::kId: return "id";
    case ListFault::kNotParked: return "not parked";
    case ListFault::kDuplicate: return "duplicate";
    case ListFault::kOrder: return "order";
    case ListFault::kFlag: return "flag";
    case ListFault::kMissing: return "missing";
    }
    return "?";
}

int failures = 0;
// list2 / flag: an empty vector stands for nullptr
void expect(const char *what, ListFault want, const V &keys, const V &list, const V &list2 = {}, const V &flag = {}) {
    const int B = (int)keys.size();
    const int *l2 = list2.empty() ? nullptr : list2.data(), *fl = flag.empty() ? nullptr : flag.data();
    const ListFault got = po::newton_list_fault(keys.data(), list.data(), l2, fl, B);
    const bool ok = po::newton_list_ok(keys.data(), list.data(), l2, fl, B);
    const bool pass = got == want && ok == (want == ListFault::kNone);
    std::printf("%-4s %-46s fault: %-10s (expected %s), ok %d\n", pass ? "ok" : "FAIL", what, name(got), name(want), (int)ok);
    failures += !pass;
}
}  // namespace

int main() {
    // B = 8.  Parked: 0 (key 5), 2 (7), 3 (5), 5 (2), 6 (7), 7 (0); paths 1 and 4 finished in the first launch.  Descending keys, ties in path order: 2 6 0 3 5 7.
    const V keys = {5, -1, 7, 5, -1, 2, 7, 0};
    // flagged standard: 0 1 3 6 7.  The parked ones of them, in order: 6 0 3 7; the parked others: 2 5.
    const V flag = {1, 1, 0, 1, 0, 0, 1, 1};
    const V one = {6, 2, 6, 0, 3, 5, 7}, first = {4, 6, 0, 3, 7}, second = {2, 2, 5};

    expect("a correct single list", ListFault::kNone, keys, one);
    expect("a correct single list, flags ignored", ListFault::kNone, keys, one, {}, flag);
    expect("a correct pair", ListFault::kNone, keys, first, second, flag);
    expect("a correct pair, no flags given", ListFault::kNone, keys, first, second);
    expect("nothing parked, an empty list", ListFault::kNone, V{-1, -1, -1}, V{0});
    expect("nothing parked, two empty lists", ListFault::kNone, V{-1, -1, -1}, V{0}, V{0}, V{1, 0, 1});
    expect("everything on the second list", ListFault::kNone, V{3, 4, 4}, V{0}, V{3, 1, 2, 0}, V{0, 0, 0});
    expect("everything on the first list", ListFault::kNone, V{3, 4, 4}, V{3, 1, 2, 0}, V{0}, V{1, 1, 1});

    expect("a duplicate (0 twice, 3 lost)", ListFault::kDuplicate, keys, V{6, 2, 6, 0, 0, 5, 7});
    expect("a missing parked path (7)", ListFault::kMissing, keys, V{5, 2, 6, 0, 3, 5});
    expect("a missing parked path of a pair (5)", ListFault::kMissing, keys, first, V{1, 2}, flag);
    expect("a listed path that is not parked (1)", ListFault::kNotParked, keys, V{7, 2, 6, 0, 3, 5, 7, 1});
    expect("descending order violated (7 before 5)", ListFault::kOrder, keys, V{6, 2, 6, 0, 3, 7, 5});
    expect("descending order violated on the second list", ListFault::kOrder, keys, first, V{2, 5, 2}, flag);
    expect("a tie in the wrong path order (6 before 2)", ListFault::kOrder, keys, V{6, 6, 2, 0, 3, 5, 7});
    expect("a count above B", ListFault::kCount, keys, V{9});
    expect("a negative count", ListFault::kCount, keys, V{-1});
    expect("a count above B on the second list", ListFault::kCount, keys, first, V{9}, flag);
    expect("a negative id", ListFault::kId, keys, V{6, 2, 6, 0, -1, 5, 7});
    expect("an id equal to B", ListFault::kId, keys, V{6, 2, 6, 0, 8, 5, 7});
    expect("a flag-0 path on the first list (2)", ListFault::kFlag, keys, V{5, 2, 6, 0, 3, 7}, V{1, 5}, flag);
    expect("a flag-1 path on the second list (3)", ListFault::kFlag, keys, V{3, 6, 0, 7}, V{3, 2, 3, 5}, flag);
    expect("the same path on both lists (0), no flags", ListFault::kDuplicate, keys, first, V{3, 2, 0, 5});
    expect("the same path on both lists (0), with flags", ListFault::kDuplicate, keys, first, V{3, 2, 0, 5}, flag);
    std::printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
