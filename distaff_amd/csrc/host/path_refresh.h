// Following ordered writes with held authentication paths (dst_rescue_refresh_paths): what needs neither HIP nor field arithmetic.  A client holds
// the paths of H keys under a root and receives the witnesses of M ordered writes (dst_rtree_apply, dst_stree_apply, dst_wtree_apply).  Write i
// has the chain c_i[0] = its new leaf, c_i[t] = digest(c_i[t - 1], its witness node t) ordered by bit t - 1 of its key: the nodes above the
// written leaf right after the write.  The chains are hashed elsewhere (kernels_hash.hip on a device, host_rescue.h on the host).  Here is the plan
// that says which write supplies which node of which held path:
//     sel[j][0] = the LAST write i with key_i == h_j,
//     sel[j][k] = the LAST write i with (key_i >> (k - 1)) == ((h_j >> (k - 1)) ^ 1)                  for 1 <= k < n,
// -1 where there is none: the held node stays.  Position 0 takes write sel's new leaf, position k its chain node c[k - 1].  The last write wins
// because a later write under the same subtree has the earlier one inside its own witness; a write outside the subtree cannot touch the node.
// A write with a key other than h lies under exactly one sibling subtree of h, so it competes for exactly one position.
//
// No H x M step: the write numbers are sorted by (key, i) once; the writes under a subtree are then a contiguous range of that order, found by two
// binary searches on the shifted keys, and "the last of them" is a range maximum over write numbers, answered by a maximum tree over the sorted
// order.  O(M log M) for the sort, O(M) for the tree, O(log M) per position: O((M + H n) log M) in all, O(M) memory beside sel.
// Stated once over the key type K: uint64_t (n <= 64) and unsigned __int128 (the _w calls, n <= 128); the sibling of a prefix and the width a key
// type serves are those of host/stree_levels.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "stree_levels.h"

#define PR_KEEP (-1)                                      // sel: no write supplies the position

// the maximum of v[lo .. hi) over a bottom-up maximum tree t of 2 m entries whose leaves t[m + x] = v[x]; PR_KEEP for an empty range
inline int32_t pr_range_max(const std::vector<int32_t>& t, size_t m, size_t lo, size_t hi) {
    int32_t best = PR_KEEP;
    for (lo += m, hi += m; lo < hi; lo >>= 1, hi >>= 1) {
        if (lo & 1) best = std::max(best, t[lo++]);
        if (hi & 1) best = std::max(best, t[--hi]);
    }
    return best;
}

// sel[held * n]: see above.  n >= 2, n - 1 <= stree_max_depth<K>(), count < 2^31 (write numbers are int32), every key below 2^(n-1) -- the caller
// has checked (pv_check_shape_of)
template <class K> inline void pr_plan(uint32_t n, const K* indices, size_t count, const K* held_indices, size_t held, int32_t* sel) {
    static_assert(stree_max_depth<K>() == 8 * sizeof(K) - 1, "a shift by n - 2 <= depth - 1 stays inside the key");
    std::vector<int32_t> order(count);
    for (size_t i = 0; i < count; i++) order[i] = (int32_t)i;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return indices[a] != indices[b] ? indices[a] < indices[b] : a < b; });
    std::vector<K> keys(count);
    for (size_t x = 0; x < count; x++) keys[x] = indices[order[x]];
    std::vector<int32_t> tree(2 * count, PR_KEEP);
    for (size_t x = 0; x < count; x++) tree[count + x] = order[x];
    for (size_t x = count; x-- > 1;) tree[x] = std::max(tree[2 * x], tree[2 * x + 1]);
    // the sorted writes whose key, shifted right by s, equals `want`
    auto range_max = [&](K want, uint32_t s) {
        const size_t lo = std::partition_point(keys.begin(), keys.end(), [&](K k) { return (K)(k >> s) < want; }) - keys.begin();
        const size_t hi = std::partition_point(keys.begin() + lo, keys.end(), [&](K k) { return (K)(k >> s) == want; }) - keys.begin();
        return pr_range_max(tree, count, lo, hi);
    };
    for (size_t j = 0; j < held; j++) {
        const K h = held_indices[j];
        int32_t* const row = sel + (size_t)n * j;
        row[0] = range_max(h, 0u);
        for (uint32_t k = 1; k < n; k++) row[k] = range_max(stree_sibling((K)(h >> (k - 1))), k - 1);
    }
}
