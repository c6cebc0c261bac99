// Stand-alone walk over distaff_amd/csrc/host/shard_geometry.h (which rank and which heap hold a leaf or a node of a sharded Merkle tree): for
// every case on standard input, "L Bt G krange", every leaf and every heap node 1 .. L-1 of the tree over L leaves is asked for its home
// (owner, zone, index) and
//   (a) no two of them share a home;
//   (b) the index lies inside the buffer that shard.hip reads for that zone (read_buffer), with the sizes that ensure_shard_buffers, the
//       context's own allocations and k_upper_tree's layout give it (heap_entries below);
//   (+) the children of a node that live in the same heap as the node sit at 2 idx and 2 idx + 1 with the same owner: what lets k_merkle
//       build that heap level by level.
// A violation is reported on standard error and ends the program with status 1.  With krange = 0 the homes are printed, "l leaf owner index" /
// "n node owner index" (owner -1: replicated): tests/test_shard_geometry.py compares them with distaff_amd.sharded.TreeGeometry line by line.
// Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include "host/shard_geometry.h"

enum { LEAVES = -1 };       // the rank-local leaf array, beside the three node zones of Geometry::node

// entries of the buffer behind a zone (index 0 of a heap is unused, so a heap over m leaves has 2 m entries of which 1 .. 2 m - 1 are nodes)
static uint64_t heap_entries(const Geometry& geo, int zone) {
    const uint64_t local = geo.L / geo.G;                  // leaves a rank holds: Bct * K; the whole tree when one rank holds it (L < Bt included)
    switch (zone) {
        case LEAVES: return local;                         // trace_leaves: Bc n; fri_leaves[d]: the rank's share of the layer's rows
        case 0: return local;                              // trace_nodes, cnodes, fri_nodes[d]: as many entries as local leaves
        // one rank: "upper" names that same full heap.  Otherwise trace_upper, c_upper: 2 n G; fri_upper[d]: 2 nb G (ensure_shard_buffers),
        // of which k-range mode fills the first 2 G as the heap over the ranks' subtree roots (tree_exchange)
        case 1: return geo.G == 1 ? local : geo.krange ? 2 * geo.G : 2 * geo.K * geo.G;
        case 2: return 2 * geo.K;                          // k_upper_tree(gathered, upper + 2 G, K / G, G): the heap over K / G * G boundary nodes
    }
    return 0;
}

static int fail(const Geometry& geo, const char* what, uint64_t i) {
    fprintf(stderr, "L=%llu Bt=%llu G=%llu krange=%d: %s at %llu\n", (unsigned long long)geo.L, (unsigned long long)geo.Bt, (unsigned long long)geo.G, (int)geo.krange, what, (unsigned long long)i);
    return 1;
}

int main() {
    unsigned long long L, Bt, G; int kr;
    while (scanf("%llu %llu %llu %d", &L, &Bt, &G, &kr) == 4) {
        const Geometry geo(L, Bt, G, kr != 0);
        printf("# %llu %llu %llu %d\n", L, Bt, G, kr);
        if (geo.krange && 2 * G + heap_entries(geo, 2) > 2 * geo.K * G) return fail(geo, "the subtree heap does not fit behind the top heap", 0);
        std::set<std::tuple<int, int, uint64_t>> homes;    // (owner, zone, index)
        for (uint64_t i = 0; i < L; i++) {
            int g = -2; uint64_t idx = 0;
            geo.leaf(i, g, idx);
            if (g < 0 || (uint64_t)g >= G || idx >= heap_entries(geo, LEAVES)) return fail(geo, "leaf outside the leaf array", i);
            if (!homes.insert({g, LEAVES, idx}).second) return fail(geo, "two leaves share a home", i);
            if (!kr) printf("l %llu %d %llu\n", (unsigned long long)i, g, (unsigned long long)idx);
        }
        for (uint64_t h = 1; h < L; h++) {
            int g = -2, zone = -2; uint64_t idx = 0;
            geo.node(h, g, idx, &zone);
            if (zone < 0 || zone > 2 || (zone == 2 && !geo.krange)) return fail(geo, "unknown zone", h);
            if (zone == 1 ? g != -1 : (g < 0 || (uint64_t)g >= G)) return fail(geo, "owner out of range", h);
            if (idx < 1 || idx >= heap_entries(geo, zone)) return fail(geo, "node outside its heap", h);
            if (!homes.insert({g, zone, idx}).second) return fail(geo, "two nodes share a home", h);
            for (uint64_t child = 2 * h; child <= 2 * h + 1 && child < L; child++) {
                int cg = -2, czone = -2; uint64_t cidx = 0;
                geo.node(child, cg, cidx, &czone);
                if (czone == zone && (cg != g || cidx != 2 * idx + (child & 1))) return fail(geo, "children not at 2 idx, 2 idx + 1", h);
            }
            int g2 = -2; uint64_t idx2 = 0;
            geo.node(h, g2, idx2);                          // without the zone: what the Python statement answers
            if (g2 != g || idx2 != idx) return fail(geo, "node() answers differently without a zone", h);
            if (!kr) printf("n %llu %d %llu\n", (unsigned long long)h, g, (unsigned long long)idx);
        }
    }
    return 0;
}
