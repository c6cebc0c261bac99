// Compressed batch openings (multiproofs) of the Rescue trees: the plan, pure integer work -- no HIP, no field arithmetic.  Node (l, p) is the node
// of level l at position p < 2^l; level D = depth holds the leaves, level 0 the root.  For a set S of distinct leaf indices, K_D = S and
// K_{l-1} = { p >> 1 : p in K_l }; the SUPPLIED siblings of level l are the (l, p ^ 1) with p in K_l and p ^ 1 not in K_l.  A multiproof is the
// leaves of S in the caller's order and the supplied siblings of level D, then of level D - 1, ... down to level 1, each level ascending by
// position: the node set of the reference's BatchMerkleProof (src/crypto/merkle.rs:64-124), laid out level by level.
// Everything is hashed over one POOL of nodes indexed by 32-bit words: [count leaves | M supplied nodes | the results of level D - 1 | ... | the
// root].  From the sorted set the plan makes the supplied positions, one list of digest jobs (left, right, out) per level -- every ancestor
// once -- and, for the expansion into full paths, the pool index of each of the count * (D + 1) path nodes.  The tree-side calls, the size
// query, the host path and the device path all run this one plan.
// The plan is stated once over the position type K: uint64_t (depth <= 63) and stree_wide (host/stree_levels.h; depth <= 127, the _w calls).
// KNOWN-EMPTY NODES (the compact form of the wide calls): a sparse tree's proof need not ship a sibling that is an empty subtree, and nobody need
// hash a parent of two empty subtrees -- its value is E_l, the empty subtree of its level.  Given one bit per supplied node ("not shipped: it is
// E_l") and one flag per leaf ("its value is E_D"), a parent is known-empty exactly when both children are: no job is made for it, and whoever
// refers to it refers to the pool entry of E_l.  The pool is then [count leaves | S shipped nodes | E_0 .. E_D | results]; a level may have no
// job at all, and a proof in which everything is known-empty has none: its root is the entry of E_0.  Without bits nothing is known-empty, there
// is no table, and the plan is the plain one above.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "stree_levels.h"

#define MP_MAX_DEPTH 63u
#define MP_WIDE_MAX_DEPTH STREE_WIDE_MAX_DEPTH
enum { MP_SUPPLIED = 1u, MP_JOBS = 2u, MP_WHERE = 4u };      // what mp_plan_make fills

struct mp_sizes {
    uint64_t nodes = 0;                                  // M = sum over l = 1 .. D of #{ p in K_l : p ^ 1 not in K_l }
    uint64_t digests = 0;                                // sum over l = 0 .. D - 1 of |K_l|; with known-empty nodes: of the members that are not
};
// the number of bits of a ^ b for a != b: 1 .. 64, 1 .. 128
inline uint32_t mp_diff_bits(uint64_t a, uint64_t b) { return 64u - (uint32_t)__builtin_clzll(a ^ b); }
inline uint32_t mp_diff_bits(const stree_wide& a, const stree_wide& b) { return a.hi != b.hi ? 128u - (uint32_t)__builtin_clzll(a.hi ^ b.hi) : mp_diff_bits(a.lo, b.lo); }
// one level: cur = K_l, sorted -> K_{l-1} in place; fn(j, pair, w): cur[j] (and cur[j + 1] when `pair`: the two children of one parent are
// both in the set) has the parent that becomes cur[w].  fn runs before cur[w] is written
template <class K, class F>
inline void mp_level(std::vector<K>& cur, F fn) {
    size_t w = 0;
    for (size_t j = 0; j < cur.size();) {
        const bool pair = !stree_bit(cur[j], 0u) && j + 1 < cur.size() && cur[j + 1] == stree_sibling(cur[j]);
        fn(j, pair, w);
        cur[w++] = cur[j] >> 1u;
        j += pair ? 2 : 1;
    }
    cur.resize(w);
}
// the sizes in one pass over the sorted set: two neighbours a < b whose a ^ b has t bits have the same ancestor on level l when t <= D - l, and
// are the two children of one parent there when t == D - l + 1 -- every pair of siblings in K_l comes from exactly one pair of neighbours.  So
// with hist[t] = the number of neighbours of t bits, |K_l| = 1 + sum of hist[t] over t > D - l, of which 2 hist[D - l + 1] have their sibling in K_l
template <class K>
inline mp_sizes mp_count(const std::vector<K>& set /* sorted, distinct, below 2^depth */, uint32_t depth) {
    mp_sizes s;
    if (set.empty()) return s;
    uint64_t hist[8 * sizeof(K) + 1] = {0};              // up to 128 bit lengths
    for (size_t j = 1; j < set.size(); j++) hist[mp_diff_bits(set[j - 1], set[j])]++;
    uint64_t width = set.size();                         // |K_l|, l = depth first
    for (uint32_t l = depth; l >= 1; l--) {
        const uint64_t pairs = hist[depth - l + 1];
        s.nodes += width - 2 * pairs;
        width -= pairs;                                  // |K_{l-1}|
        s.digests += width;
    }
    return s;
}

template <class K> struct mp_plan_t {
    uint32_t depth = 0;
    size_t count = 0;
    mp_sizes sizes;
    std::vector<uint32_t> slevel;                        // MP_SUPPLIED: supplied node m is (slevel[m], spos[m])
    std::vector<K> spos;
    std::vector<uint32_t> jobs;                          // MP_JOBS: 3 words (left, right, out) per job; the jobs that write level l at jobs[3 joff[l] ..), jcnt[l] of them
    size_t joff[stree_max_depth<K>()] = {0}, jcnt[stree_max_depth<K>()] = {0};
    std::vector<uint32_t> where;                         // MP_WHERE: where[i * (depth + 1) + k] = the pool index of node k of the path of indices[i]
    size_t shipped = 0;                                  // S: the supplied nodes that are in the pool; M without bits
    size_t table = 0;                                    // depth + 1 entries E_0 .. E_depth behind them with bits, else none
    uint32_t levels = 0;                                 // how many levels have a job
    uint32_t root = 0;                                   // the pool index of the root: the last node of the pool, or the entry of E_0 when there is no job
    size_t empty_at(uint32_t l) const { return count + shipped + l; }
    size_t inputs() const { return count + shipped + table; }
    size_t pool() const { return inputs() + (size_t)sizes.digests; }
};
typedef mp_plan_t<uint64_t> mp_plan;

// bit m of the bytes `bits`
inline bool mp_bit(const uint8_t* bits, uint64_t m) { return (bits[m >> 3] >> (m & 7)) & 1u; }
// how many of bits[0 .. M) are set, and whether the padding bits of the last byte are all 0
inline uint64_t mp_popcount(const uint8_t* bits, uint64_t M, bool* padding_clear) {
    uint64_t n = 0;
    for (uint64_t b = 0; b < M / 8; b++) n += (uint64_t)__builtin_popcount(bits[b]);
    *padding_clear = true;
    if (M & 7) {
        const uint8_t last = bits[M / 8], mask = (uint8_t)((1u << (M & 7)) - 1u);
        n += (uint64_t)__builtin_popcount(last & mask);
        *padding_clear = !(last & ~mask);
    }
    return n;
}

// nullptr and the plan of `count` >= 1 indices below 2^depth (1 <= depth <= 63 or 127, count < 2^31), in any order; else what is wrong with them.
// absent_bits (MP_JOBS or MP_WHERE only; ceil(M / 8) bytes): bit m = supplied node m is known-empty and not in the pool; leaf_empty (with
// absent_bits; may be nullptr: none): leaf_empty[i] != 0 = the leaf of indices[i] is known-empty
template <class K>
inline const char* mp_plan_make(uint32_t depth, const K* indices, size_t count, uint32_t what, mp_plan_t<K>& p, const uint8_t* absent_bits = nullptr, const uint8_t* leaf_empty = nullptr) {
    const size_t n = (size_t)depth + 1;
    const bool hashes = what & (MP_JOBS | MP_WHERE), ascending = std::is_sorted(indices, indices + count);
    std::vector<K> cur(indices, indices + count);
    std::vector<uint32_t> order;                         // sorted position -> the caller's position = the leaf's pool index
    auto in_order = [&] { order.resize(count); for (size_t i = 0; i < count; i++) order[i] = (uint32_t)i; };
    if (!ascending && hashes) {
        in_order();
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return indices[a] < indices[b]; });
        for (size_t s = 0; s < count; s++) cur[s] = indices[order[s]];
    } else if (!ascending) std::sort(cur.begin(), cur.end());
    if (std::adjacent_find(cur.begin(), cur.end()) != cur.end()) return "a leaf index is repeated";
    p.depth = depth; p.count = count;
    p.sizes = mp_count(cur, depth);
    p.shipped = (size_t)p.sizes.nodes; p.table = 0; p.levels = 0;
    if ((uint64_t)count + p.sizes.nodes + p.sizes.digests + (absent_bits ? n : 0) >= ((uint64_t)1 << 32)) return "2^32 pool nodes or more (leaves + supplied nodes + digests)";
    if (ascending && hashes) in_order();
    if (what & MP_SUPPLIED) { p.slevel.reserve(p.sizes.nodes); p.spos.reserve(p.sizes.nodes); }
    if (what & MP_JOBS) p.jobs.reserve(3 * p.sizes.digests);
    if (!hashes) {                                       // the sizes, or the positions, alone
        for (uint32_t l = depth; l >= 1 && (what & MP_SUPPLIED); l--)
            mp_level(cur, [&](size_t j, bool pair, size_t) { if (!pair) { p.slevel.push_back(l); p.spos.push_back(stree_sibling(cur[j])); } });
        return nullptr;
    }
    const bool sparse = absent_bits != nullptr;
    if (sparse) {
        bool clear;
        p.shipped = (size_t)(p.sizes.nodes - mp_popcount(absent_bits, p.sizes.nodes, &clear));
        if (!clear) return "a padding bit of absent_bits is set";
        p.table = n;
    }
    std::vector<uint32_t> ref(order), sib(count), par(count), anc;      // per member of K_l: its pool index, its sibling's, its parent's place in K_{l-1}
    std::vector<uint8_t> ke(count, 0);                   // per member of K_l: known-empty
    if (sparse && leaf_empty) for (size_t s = 0; s < count; s++) ke[s] = leaf_empty[order[s]] ? 1 : 0;
    if (what & MP_WHERE) {
        p.where.resize(count * n);
        anc.resize(count);                               // per sorted leaf: the place of its ancestor in K_l
        for (size_t s = 0; s < count; s++) { anc[s] = (uint32_t)s; p.where[(size_t)order[s] * n] = ke[s] ? (uint32_t)p.empty_at(depth) : order[s]; }
    }
    uint32_t supplied = (uint32_t)count, result = (uint32_t)p.inputs();
    uint64_t m = 0;                                      // the number of the next supplied node
    size_t done = 0;
    for (uint32_t l = depth; l >= 1; l--) {
        p.joff[l - 1] = done;
        size_t made = 0;
        mp_level(cur, [&](size_t j, bool pair, size_t w) {
            uint32_t left = ref[j], right;
            bool empty = ke[j];
            if (pair) { right = ref[j + 1]; empty = empty && ke[j + 1]; sib[j] = right; sib[j + 1] = left; par[j + 1] = (uint32_t)w; }
            else {
                const bool absent = sparse && mp_bit(absent_bits, m);
                m++;
                right = absent ? (uint32_t)p.empty_at(l) : supplied++;
                empty = empty && absent;
                if (what & MP_SUPPLIED) { p.slevel.push_back(l); p.spos.push_back(stree_sibling(cur[j])); }
                sib[j] = right;
                if (stree_bit(cur[j], 0u)) std::swap(left, right);                 // the member is the right child: the sibling goes first
            }
            par[j] = (uint32_t)w;
            if (empty) { ref[w] = (uint32_t)p.empty_at(l - 1); ke[w] = 1; return; }      // a parent of two empty subtrees is E_{l-1}: nothing to hash
            if (what & MP_JOBS) { p.jobs.push_back(left); p.jobs.push_back(right); p.jobs.push_back(result); }
            ref[w] = result++; ke[w] = 0;
            made++;
        });
        p.jcnt[l - 1] = made;
        done += made;
        if (made) p.levels++;
        if (what & MP_WHERE)
            for (size_t s = 0; s < count; s++) { p.where[(size_t)order[s] * n + (depth - l + 1)] = sib[anc[s]]; anc[s] = par[anc[s]]; }
    }
    p.sizes.digests = done;
    p.root = ref[0];
    return nullptr;
}
