// Ordered leaf writes to Rescue Merkle trees (dst_rtree_apply, dst_stree_apply): the integer bookkeeping, free of HIP and of field arithmetic.
// Operation i of a sequence writes leaf index_i; v_i^l is the value of index_i's ancestor at level l (depth = the leaves, 0 = the root) once
// operations 0 .. i are applied.  v_i^l = digest of v_i^(l+1) and of the sibling node as operations 0 .. i-1 left it: the version v_j^(l+1) of
// the last earlier operation j whose ancestor that sibling is, or the node the tree held before the call.  Everything level l needs thus lies
// on level l + 1, so one launch per level hashes all operations; the plan made here says, per operation and level, where the sibling is read.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// a source word: version j of the level below (TSEQ_VERSION | j, j < 2^31), the tree's own node at a position below TSEQ_EMPTY (dense: the
// node-array position; sparse: the flat position), or TSEQ_EMPTY: no stored node, the value of an empty subtree of that level
#define TSEQ_VERSION 0x80000000u
#define TSEQ_EMPTY 0x7FFFFFFFu
#define TSEQ_MAX_DEPTH 63u

// K: the type of an index -- uint64_t (depth <= 63) or, for the wide sparse trees, unsigned __int128 (depth <= 127): one bit more than the depth
template <class K> struct tseq_plan_t {
    uint32_t depth = 0;
    size_t count = 0;
    // row 0: where the old value of operation i's own leaf is read; row k (1 .. depth): where node k of its authentication path is, the sibling
    // on level depth - k + 1 -- src[k * count + i]
    std::vector<uint32_t> src;
    // the nodes the sequence writes and the last operation through each: level l's, sorted by prefix = index >> (depth - l), at
    // [toff[l], toff[l] + tcnt[l]).  Level depth: the distinct indices with the operation whose value stays.
    std::vector<K> tpref;
    std::vector<uint32_t> tlast;
    size_t toff[8 * sizeof(K)] = {0}, tcnt[8 * sizeof(K)] = {0};
    size_t touched() const { return tpref.size(); }
};
typedef tseq_plan_t<uint64_t> tseq_plan;

// original(level, prefix) -> the source word of that node before the call (a position or TSEQ_EMPTY).  count < 2^31, indices below 2^depth.
// One sort by (index, i); then, per level going up, one pass over the operations, held as groups of equal prefix, each in the order of i:
// two sibling groups are merged by i, which says for every operation the last earlier one on the other side, and the merged group is the
// parent's.  O(count * depth) after the sort, besides the calls of `original` (at most two per group and level).
template <class K, class Original>
inline tseq_plan_t<K> tseq_plan_make(uint32_t depth, const K* indices, size_t count, Original original) {
    tseq_plan_t<K> p;
    p.depth = depth; p.count = count;
    p.src.assign((size_t)(depth + 1) * count, TSEQ_EMPTY);
    p.tpref.reserve(count * 2); p.tlast.reserve(count * 2);
    std::vector<uint32_t> ord(count), next(count);
    for (size_t i = 0; i < count; i++) ord[i] = (uint32_t)i;
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return indices[a] != indices[b] ? indices[a] < indices[b] : a < b; });
    for (uint32_t l = depth; l >= 1; l--) {
        const uint32_t shift = depth - l;
        uint32_t* row = p.src.data() + (size_t)(depth - l + 1) * count;
        p.toff[l] = p.tpref.size();
        auto group_end = [&](size_t a, K q) { while (a < count && (indices[ord[a]] >> shift) == q) a++; return a; };
        auto touch = [&](size_t a, size_t b, K q) {             // the group [a, b) of prefix q
            p.tpref.push_back(q); p.tlast.push_back(ord[b - 1]);
            if (l != depth) return;
            for (size_t t = a; t < b; t++) p.src[ord[t]] = t == a ? original(depth, q) : TSEQ_VERSION | ord[t - 1];
        };
        size_t w = 0;
        for (size_t a = 0; a < count;) {
            const K q = indices[ord[a]] >> shift;
            const size_t b = group_end(a, q);
            touch(a, b, q);
            const size_t c = (q & 1) == 0 ? group_end(b, q | 1) : b;
            if (c == b) {                                                // the sibling node is not written by this sequence
                const uint32_t o = original(l, q ^ 1);
                for (size_t t = a; t < b; t++) { row[ord[t]] = o; next[w++] = ord[t]; }
            } else {
                touch(b, c, q | 1);
                uint32_t left = original(l, q), right = original(l, q | 1);       // what an operation on the other side reads: updated as the merge passes
                for (size_t x = a, y = b; x < b || y < c;) {
                    const bool from_left = y == c || (x < b && ord[x] < ord[y]);
                    const uint32_t op = from_left ? ord[x++] : ord[y++];
                    row[op] = from_left ? right : left;
                    (from_left ? left : right) = TSEQ_VERSION | op;
                    next[w++] = op;
                }
            }
            a = c;
        }
        p.tcnt[l] = p.tpref.size() - p.toff[l];
        ord.swap(next);
    }
    p.toff[0] = p.tpref.size();
    if (count) { p.tpref.push_back(0); p.tlast.push_back((uint32_t)(count - 1)); }
    p.tcnt[0] = p.tpref.size() - p.toff[0];
    return p;
}
