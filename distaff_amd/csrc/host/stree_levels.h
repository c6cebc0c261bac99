// Sparse Rescue Merkle trees (dst_stree_*, dst_wtree_*): the integer bookkeeping, free of HIP and of field arithmetic.  A tree of depth D stores,
// per level l (D = the leaves, 0 = the root), the sorted distinct prefixes key >> (D - l) of its keys; a node is found by a lower-bound search for
// its prefix.  Here: that search (shared with the kernels of kernels_hash.hip, hence STREE_HD), and the plan of a dst_stree_set -- the merge of the
// new keys into every level, where each node of the merged level comes from, and which nodes have to be hashed -- and the plan of a removal
// (dst_stree_remove, dst_stree_compact), the same three things for the pruned levels.  The host path and the device path run the same plan.
// Everything is stated once over the key type K: uint64_t (dst_stree_*, depth <= 63), and for the wide trees (dst_wtree_*, depth <= 127)
// unsigned __int128 on the host and stree_wide, the same 16 bytes as two 64-bit halves, on the device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define STREE_HD __host__ __device__ inline
#else
#define STREE_HD inline
#endif

#define STREE_MAX_DEPTH 63u
#define STREE_WIDE_MAX_DEPTH 127u
#define STREE_ABSENT (~(size_t)0)                        // no such prefix on the level
#define STREE_NEW 0xFFFFFFFFu                            // stree_plan::src of a node that the set writes (a new leaf, a hashed parent)

// the deepest tree a key type serves: one bit less than the key holds (63, 127), so that index + 2^depth -- the tape rule -- still fits
template <class K> constexpr uint32_t stree_max_depth() { return (uint32_t)(8 * sizeof(K) - 1); }

// a 128-bit key as the device reads it: the memory image of a little-endian u128.  The comparison and the shift are stated here, once; a shift
// by D - l crosses the halves for every level that lies more than 64 above the leaves
struct stree_wide { uint64_t lo, hi; };
STREE_HD bool operator<(const stree_wide& a, const stree_wide& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }
STREE_HD bool operator>(const stree_wide& a, const stree_wide& b) { return b < a; }
STREE_HD bool operator==(const stree_wide& a, const stree_wide& b) { return a.lo == b.lo && a.hi == b.hi; }
STREE_HD bool operator!=(const stree_wide& a, const stree_wide& b) { return !(a == b); }
STREE_HD stree_wide operator>>(const stree_wide& a, uint32_t s) {                          // s < 128
    if (s >= 64) return stree_wide{a.hi >> (s - 64), 0};
    return s ? stree_wide{(a.lo >> s) | (a.hi << (64 - s)), a.hi >> s} : a;
}
// what the searches ask of a prefix besides < and ==: the child 2q + side, the sibling q ^ 1, bit s
STREE_HD stree_wide stree_child(const stree_wide& q, uint32_t side) { return stree_wide{(q.lo << 1) | side, (q.hi << 1) | (q.lo >> 63)}; }
STREE_HD stree_wide stree_sibling(const stree_wide& q) { return stree_wide{q.lo ^ 1, q.hi}; }
STREE_HD uint32_t stree_bit(const stree_wide& q, uint32_t s) { return (uint32_t)((s < 64 ? q.lo >> s : q.hi >> (s - 64)) & 1u); }
template <class K> STREE_HD K stree_child(K q, uint32_t side) { return (K)(2 * q + side); }
template <class K> STREE_HD K stree_sibling(K q) { return q ^ (K)1; }
template <class K> STREE_HD uint32_t stree_bit(K q, uint32_t s) { return (uint32_t)(q >> s) & 1u; }

// the first position in the sorted pref[0 .. cnt) whose prefix is not below `want`; cnt when there is none
template <class K> STREE_HD size_t stree_lower_bound(const K* pref, size_t cnt, K want) {
    size_t lo = 0;
    while (cnt) {
        const size_t half = cnt >> 1;
        if (pref[lo + half] < want) { lo += half + 1; cnt -= half + 1; }
        else cnt = half;
    }
    return lo;
}
template <class K> STREE_HD size_t stree_find(const K* pref, size_t cnt, K want) {
    const size_t i = stree_lower_bound(pref, cnt, want);
    return i < cnt && pref[i] == want ? i : STREE_ABSENT;
}
// stree_lower_bound for a run of ascending wants: the search starts at `from`, a position with only smaller prefixes before it, and gallops
// forward, so a sorted batch costs a walk along the list, not a search from the top each
template <class K> STREE_HD size_t stree_advance(const K* pref, size_t cnt, size_t from, K want) {
    size_t hi = from, step = 1;
    while (hi < cnt && pref[hi] < want) { from = hi + 1; hi += step; step <<= 1; }
    return from + stree_lower_bound(pref + from, (hi < cnt ? hi : cnt) - from, want);
}
// the children of the parent with prefix q among the child level's prefixes: the positions of 2q and 2q + 1, STREE_ABSENT for an empty side
template <class K> STREE_HD void stree_children(const K* cpref, size_t ccnt, K q, size_t& left, size_t& right) {
    const K lq = stree_child(q, 0u), rq = stree_child(q, 1u);
    const size_t i = stree_lower_bound(cpref, ccnt, lq);
    const bool has_left = i < ccnt && cpref[i] == lq;
    const size_t j = i + (has_left ? 1 : 0);
    left = has_left ? i : STREE_ABSENT;
    right = j < ccnt && cpref[j] == rq ? j : STREE_ABSENT;
}
// node k of the authentication path [leaf, sibling, uncle, ...] of `index`: its level and its prefix there
template <class K> STREE_HD void stree_path_slot(uint32_t depth, K index, uint32_t k, uint32_t& level, K& prefix) {
    if (k == 0) { level = depth; prefix = index; return; }
    level = depth - (k - 1);
    prefix = stree_sibling((K)(index >> (k - 1)));
}

// the stored nodes of a tree: level l's sorted prefixes at pref[start[l] .. start[l] + cnt[l]).  The node values live in an array of the same
// layout (host: u128 pairs, device: fe pairs); a "flat position" indexes both.  Levels are laid out from the leaves (depth) to the root (0).
template <class K> struct stree_shape_t {
    uint32_t depth = 0;
    std::vector<K> pref;
    size_t start[stree_max_depth<K>() + 1] = {0}, cnt[stree_max_depth<K>() + 1] = {0};
    size_t total() const { return pref.size(); }
};
typedef stree_shape_t<uint64_t> stree_shape;
// what a set, or a removal, of sorted distinct keys does to a shape
template <class K> struct stree_plan_t {
    stree_shape_t<K> next;                                    // the merged (set) or pruned (removal) levels
    std::vector<uint32_t> src;                           // per flat position of `next`: the flat position in the old shape the node is carried over from, or STREE_NEW
    std::vector<uint32_t> dirty;                         // flat positions in `next` of the touched nodes: level l's, sorted, at dirty[doff[l] .. doff[l] + dcnt[l]);
    size_t doff[stree_max_depth<K>() + 1] = {0}, dcnt[stree_max_depth<K>() + 1] = {0};      // level depth: the new leaves, in the order of the sorted keys
    uint64_t digests = 0;                                // parents to hash: the distinct ancestors of the keys = sum of dcnt[l] over l < depth
};
typedef stree_plan_t<uint64_t> stree_plan;
// flat positions are 32 bits: old.total() + keys.size() * (depth + 1) must stay below STREE_NEW (the caller checks)
template <class K> inline stree_plan_t<K> stree_plan_set(const stree_shape_t<K>& old, std::vector<K> cur /* sorted, distinct, below 2^depth */) {
    stree_plan_t<K> p;
    const uint32_t depth = old.depth;
    p.next.depth = depth;
    const size_t most = old.total() + cur.size() * (depth + 1);
    p.next.pref.reserve(most); p.src.reserve(most); p.dirty.reserve(cur.size() * (depth + 1));
    for (uint32_t l = depth;; l--) {                     // cur = the touched prefixes of level l
        const K* o = old.pref.data() + old.start[l];
        const size_t on = old.cnt[l];
        p.next.start[l] = p.next.pref.size(); p.doff[l] = p.dirty.size(); p.dcnt[l] = cur.size();
        if (l < depth) p.digests += cur.size();
        for (size_t i = 0, j = 0; i < on || j < cur.size();) {
            if (j == cur.size() || (i < on && o[i] < cur[j])) {
                p.next.pref.push_back(o[i]); p.src.push_back((uint32_t)(old.start[l] + i)); i++;
            } else {
                if (i < on && o[i] == cur[j]) i++;
                p.dirty.push_back((uint32_t)p.next.pref.size());
                p.next.pref.push_back(cur[j]); p.src.push_back(STREE_NEW); j++;
            }
        }
        p.next.cnt[l] = p.next.pref.size() - p.next.start[l];
        if (l == 0) break;
        for (auto& v : cur) v >>= 1;
        cur.erase(std::unique(cur.begin(), cur.end()), cur.end());
    }
    return p;
}
// the plan of a removal: the stored keys `gone` leave, and with them every node that has no stored key below it any more.  A touched node --
// an ancestor of a removed key -- that keeps a child on the pruned level below is on its level's dirty list and is written by the plan
// (src = STREE_NEW) when `rehash`; without `rehash` it is carried over like the untouched ones and nothing is dirty: the removal of keys that
// hold the empty leaf, whose ancestors do not change (dst_stree_compact).  dcnt[depth] = 0: there are no new leaves.
template <class K> inline stree_plan_t<K> stree_plan_remove(const stree_shape_t<K>& old, std::vector<K> cur /* sorted, distinct, stored */, bool rehash = true) {
    stree_plan_t<K> p;
    const uint32_t depth = old.depth;
    p.next.depth = depth;
    p.next.pref.reserve(old.total()); p.src.reserve(old.total());
    if (rehash) p.dirty.reserve(cur.size() * depth);
    for (uint32_t l = depth;; l--) {                     // cur = the touched prefixes of level l, all of them stored
        const K* o = old.pref.data() + old.start[l];
        const size_t on = old.cnt[l];
        p.next.start[l] = p.next.pref.size(); p.doff[l] = p.dirty.size();
        const K* c = l < depth ? p.next.pref.data() + p.next.start[l + 1] : nullptr;      // the pruned level below, complete
        const size_t cn = l < depth ? p.next.cnt[l + 1] : 0;
        for (size_t i = 0, j = 0, at = 0; i < on; i++) {
            const bool touched = j < cur.size() && cur[j] == o[i];
            if (touched) {
                j++;
                at = stree_advance(c, cn, at, stree_child(o[i], 0u));               // the touched prefixes ascend: one walk along the children
                if (at == cn || c[at] > stree_child(o[i], 1u)) continue;            // nothing stored below it any more: pruned
                if (rehash) p.dirty.push_back((uint32_t)p.next.pref.size());
            }
            p.next.pref.push_back(o[i]);
            p.src.push_back(touched && rehash ? STREE_NEW : (uint32_t)(old.start[l] + i));
        }
        p.next.cnt[l] = p.next.pref.size() - p.next.start[l];
        p.dcnt[l] = p.dirty.size() - p.doff[l];
        p.digests += p.dcnt[l];
        if (l == 0) break;
        for (auto& v : cur) v >>= 1;
        cur.erase(std::unique(cur.begin(), cur.end()), cur.end());
    }
    return p;
}
