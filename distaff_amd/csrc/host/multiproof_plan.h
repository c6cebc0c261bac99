// Compressed batch openings (multiproofs) of the Rescue trees: the plan, pure integer work -- no HIP, no field arithmetic.  Node (l, p) is the node
// of level l at position p < 2^l; level D = depth holds the leaves, level 0 the root.  For a set S of distinct leaf indices, K_D = S and
// K_{l-1} = { p >> 1 : p in K_l }; the SUPPLIED siblings of level l are the (l, p ^ 1) with p in K_l and p ^ 1 not in K_l.  A multiproof is the
// leaves of S in the caller's order and the supplied siblings of level D, then of level D - 1, ... down to level 1, each level ascending by
// position: the node set of the reference's BatchMerkleProof (src/crypto/merkle.rs:64-124), laid out level by level.
// Everything is hashed over one POOL of nodes indexed by 32-bit words: [count leaves | M supplied nodes | the results of level D - 1 | ... | the
// root].  From the sorted set the plan makes the supplied positions, one list of digest jobs (left, right, out) per level -- every ancestor
// once -- and, for the expansion into full paths, the pool index of each of the count * (D + 1) path nodes.  The tree-side calls, the size
// query, the host path and the device path all run this one plan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#define MP_MAX_DEPTH 63u
enum { MP_SUPPLIED = 1u, MP_JOBS = 2u, MP_WHERE = 4u };      // what mp_plan_make fills

struct mp_sizes {
    uint64_t nodes = 0;                                  // M = sum over l = 1 .. D of #{ p in K_l : p ^ 1 not in K_l }
    uint64_t digests = 0;                                // sum over l = 0 .. D - 1 of |K_l|
};
// one level: cur = K_l, sorted -> K_{l-1} in place; fn(j, pair, w): cur[j] (and cur[j + 1] when `pair`: the two children of one parent are
// both in the set) has the parent that becomes cur[w].  fn runs before cur[w] is written
template <class F>
inline void mp_level(std::vector<uint64_t>& cur, F fn) {
    size_t w = 0;
    for (size_t j = 0; j < cur.size();) {
        const bool pair = !(cur[j] & 1) && j + 1 < cur.size() && cur[j + 1] == cur[j] + 1;
        fn(j, pair, w);
        cur[w++] = cur[j] >> 1;
        j += pair ? 2 : 1;
    }
    cur.resize(w);
}
// the sizes in one pass over the sorted set: two neighbours a < b whose a ^ b has t bits have the same ancestor on level l when t <= D - l, and
// are the two children of one parent there when t == D - l + 1 -- every pair of siblings in K_l comes from exactly one pair of neighbours.  So
// with hist[t] = the number of neighbours of t bits, |K_l| = 1 + sum of hist[t] over t > D - l, of which 2 hist[D - l + 1] have their sibling in K_l
inline mp_sizes mp_count(const std::vector<uint64_t>& set /* sorted, distinct, below 2^depth */, uint32_t depth) {
    mp_sizes s;
    if (set.empty()) return s;
    uint64_t hist[65] = {0};
    for (size_t j = 1; j < set.size(); j++) hist[64 - __builtin_clzll(set[j - 1] ^ set[j])]++;
    uint64_t width = set.size();                         // |K_l|, l = depth first
    for (uint32_t l = depth; l >= 1; l--) {
        const uint64_t pairs = hist[depth - l + 1];
        s.nodes += width - 2 * pairs;
        width -= pairs;                                  // |K_{l-1}|
        s.digests += width;
    }
    return s;
}

struct mp_plan {
    uint32_t depth = 0;
    size_t count = 0;
    mp_sizes sizes;
    std::vector<uint32_t> slevel;                        // MP_SUPPLIED: supplied node m is (slevel[m], spos[m])
    std::vector<uint64_t> spos;
    std::vector<uint32_t> jobs;                          // MP_JOBS: 3 words (left, right, out) per job; the jobs that write level l at jobs[3 joff[l] ..), jcnt[l] of them
    size_t joff[MP_MAX_DEPTH] = {0}, jcnt[MP_MAX_DEPTH] = {0};
    std::vector<uint32_t> where;                         // MP_WHERE: where[i * (depth + 1) + k] = the pool index of node k of the path of indices[i]
    size_t inputs() const { return count + (size_t)sizes.nodes; }
    size_t pool() const { return inputs() + (size_t)sizes.digests; }      // the root is the last node of the pool
};

// nullptr and the plan of `count` >= 1 indices below 2^depth (1 <= depth <= 63, count < 2^31), in any order; else what is wrong with them
inline const char* mp_plan_make(uint32_t depth, const uint64_t* indices, size_t count, uint32_t what, mp_plan& p) {
    const size_t n = (size_t)depth + 1;
    const bool hashes = what & (MP_JOBS | MP_WHERE), ascending = std::is_sorted(indices, indices + count);
    std::vector<uint64_t> cur(indices, indices + count);
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
    if ((uint64_t)count + p.sizes.nodes + p.sizes.digests >= ((uint64_t)1 << 32)) return "2^32 pool nodes or more (leaves + supplied nodes + digests)";
    if (ascending && hashes) in_order();
    if (what & MP_SUPPLIED) { p.slevel.reserve(p.sizes.nodes); p.spos.reserve(p.sizes.nodes); }
    if (what & MP_JOBS) p.jobs.reserve(3 * p.sizes.digests);
    if (!(what & (MP_JOBS | MP_WHERE))) {                // the sizes, or the positions, alone
        for (uint32_t l = depth; l >= 1 && (what & MP_SUPPLIED); l--)
            mp_level(cur, [&](size_t j, bool pair, size_t) { if (!pair) { p.slevel.push_back(l); p.spos.push_back(cur[j] ^ 1); } });
        return nullptr;
    }
    std::vector<uint32_t> ref(order), sib(count), par(count), anc;      // per member of K_l: its pool index, its sibling's, its parent's place in K_{l-1}
    if (what & MP_WHERE) {
        p.where.resize(count * n);
        anc.resize(count);                               // per sorted leaf: the place of its ancestor in K_l
        for (size_t s = 0; s < count; s++) { anc[s] = (uint32_t)s; p.where[(size_t)order[s] * n] = order[s]; }
    }
    uint32_t supplied = (uint32_t)count, result = (uint32_t)p.inputs();
    size_t done = 0;
    for (uint32_t l = depth; l >= 1; l--) {
        p.joff[l - 1] = done;
        mp_level(cur, [&](size_t j, bool pair, size_t w) {
            uint32_t left = ref[j], right;
            if (pair) { right = ref[j + 1]; sib[j] = right; sib[j + 1] = left; par[j + 1] = (uint32_t)w; }
            else {
                right = supplied++;
                if (what & MP_SUPPLIED) { p.slevel.push_back(l); p.spos.push_back(cur[j] ^ 1); }
                sib[j] = right;
                if (cur[j] & 1) std::swap(left, right);                     // the member is the right child: the sibling goes first
            }
            par[j] = (uint32_t)w;
            if (what & MP_JOBS) { p.jobs.push_back(left); p.jobs.push_back(right); p.jobs.push_back(result); }
            ref[w] = result++;
        });
        p.jcnt[l - 1] = cur.size();
        done += cur.size();
        if (what & MP_WHERE)
            for (size_t s = 0; s < count; s++) { p.where[(size_t)order[s] * n + (depth - l + 1)] = sib[anc[s]]; anc[s] = par[anc[s]]; }
    }
    return nullptr;
}
