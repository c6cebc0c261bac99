// Which rank and which heap hold a leaf or a node of a Merkle tree whose leaves are split over the ranks by columns (DESIGN.md section 6;
// distaff_amd/sharded.py TreeGeometry states the same without the k-range mode).  Pure integer code: shard.hip plans the openings with it,
// tests/shard_geometry/shard_geometry_check.cpp walks it on its own.
#pragma once
#include <cstdint>

struct Geometry {                      // L natural-order leaves Bt*k + j', columns j' split evenly over G ranks (Bct each), K values of k
    uint64_t L, Bt, G, Bct, K;
    bool krange;                       // levels between the rank-local ones and the top log2(G): owned by k-ranges (dst_prove_sharded) instead of replicated
    Geometry(uint64_t leaves, uint64_t bt, uint64_t g, bool kr = false) : L(leaves), Bt(bt), G(g), Bct(bt / g), K(leaves / bt), krange(kr && g > 1) {}
    void leaf(uint64_t i, int& g, uint64_t& local) const { uint64_t k = i / Bt, j = i % Bt; g = (int)(j / Bct); local = k * Bct + (j - (uint64_t)g * Bct); }
    // zone: 0 rank-local heap, 1 replicated heap (global indices), 2 the owner's subtree heap (k-range mode)
    void node(uint64_t heap, int& g, uint64_t& idx, int* zone = nullptr) const {
        uint64_t level = 1; while (level * 2 <= heap) level *= 2;              // nodes on this level
        uint64_t t = heap - level, span = L / level;
        if (zone) *zone = 0;
        if (span >= Bct) {
            if (krange && level > G) {                                         // subtree of the rank that owns k in [g*K/G, (g+1)*K/G): level/G nodes of this level each
                const uint64_t per = level / G;
                g = (int)(t / per); idx = per + t % per;
                if (zone) *zone = 2;
                return;
            }
            g = -1; idx = heap;
            if (zone) *zone = 1;
            return;
        }
        uint64_t local_leaf; leaf(t * span, g, local_leaf);
        idx = L / (G * span) + local_leaf / span;                              // nodes of this level held by one rank = L / (G * span), also when L < Bt
    }
};
