// BLAKE3 Merkle trees (kernels_hash.hip): which kernel builds which level, free of HIP.  A tree over 2^a leaves is a heap nodes[1 .. 2^a) with
// the level of `count` nodes at nodes[count .. 2 count); the leaves are an array of their own.  merkle_plan turns "this level is filled, build
// down to that one" into the list of launches, and the functions below it give a launch's name, profiling bytes and grid.  k_merkle walks the
// list and is the only place that launches the four kernels.
#pragma once
#include <cstddef>
#include <vector>

#define MERKLE_THREADS 256u                              // lanes per workgroup of all four kernels
#define MERKLE_LEVEL2_MIN ((size_t)1 << 19)              // grandparents per launch from which two levels are built per launch (DISTAFF_MERKLE_LEVEL2_LOG)
#define MERKLE_SUBTREE_MAX ((size_t)1 << 19)             // the widest level the subtree kernel starts from: wider levels are work-bound, one launch each
#define MERKLE_SUBTREE_NODES 512u                        // nodes that one workgroup of the subtree kernel hashes down to one: nine levels
#define MERKLE_TOP_MAX ((size_t)1024)                    // the widest level the single-workgroup top kernel starts from

enum merkle_kind { MERKLE_LEVEL, MERKLE_LEVEL2, MERKLE_SUBTREE, MERKLE_TOP };
// count: the kernel's count argument -- parents (level), grandparents (level2), nodes of the filled level it starts from (subtree, top)
struct merkle_launch { merkle_kind kind; size_t count; };

// The launches that build a tree from a filled level of `count` children down to the level of `stop_count` nodes; stop_count = 0: down to the
// root, and nodes[0] is cleared.  in_place: the children are nodes[count .. 2 count) (otherwise a leaf array, which only the two level kernels
// read).  level2_min: see MERKLE_LEVEL2_MIN; levels_only (DISTAFF_MERKLE_LEVELS): one launch per level.
//   * subtree kernel: only on the way to the root, from a level in the heap of at most MERKLE_SUBTREE_MAX nodes that splits into whole workgroups;
//   * top kernel: ends every build to the root, from at most MERKLE_TOP_MAX nodes;
//   * two levels per launch: from level2_min grandparents on, and never past the stop level.
inline std::vector<merkle_launch> merkle_plan(size_t count, bool in_place, size_t stop_count, size_t level2_min, bool levels_only) {
    std::vector<merkle_launch> plan;
    const bool to_root = stop_count == 0;
    const size_t until = to_root ? MERKLE_TOP_MAX : stop_count;
    while (!in_place || count > until) {
        const size_t grand = count >> 2;
        if (to_root && in_place && !levels_only && count <= MERKLE_SUBTREE_MAX && count % MERKLE_SUBTREE_NODES == 0) {
            plan.push_back({MERKLE_SUBTREE, count});
            count /= MERKLE_SUBTREE_NODES;
        } else if (!levels_only && grand >= level2_min && grand > 0 && grand >= stop_count) {
            plan.push_back({MERKLE_LEVEL2, grand});
            count = grand;
        } else {
            plan.push_back({MERKLE_LEVEL, count >> 1});
            count >>= 1;
        }
        in_place = true;
    }
    if (to_root) plan.push_back({MERKLE_TOP, count});
    return plan;
}

// the kernel and profiling name of a launch
inline const char* merkle_launch_name(const merkle_launch& l) {
    switch (l.kind) {
        case MERKLE_LEVEL: return "merkle_level_kernel";
        case MERKLE_LEVEL2: return "merkle_level2_kernel";
        case MERKLE_SUBTREE: return "merkle_subtree_kernel";
        default: return "merkle_top_kernel";
    }
}
// profiling bytes: 64 read + 32 written per parent (three parents per grandparent); the subtree kernel: 64 per node of the level it starts from
inline double merkle_launch_bytes(const merkle_launch& l) {
    return l.kind == MERKLE_LEVEL2 ? 96.0 * 3 * l.count : l.kind == MERKLE_SUBTREE ? 64.0 * l.count : 96.0 * l.count;
}
// workgroups of MERKLE_THREADS lanes: a lane per parent / grandparent, a workgroup per subtree, one workgroup for the top
inline size_t merkle_launch_blocks(const merkle_launch& l) {
    return l.kind == MERKLE_TOP ? 1 : l.kind == MERKLE_SUBTREE ? l.count / MERKLE_SUBTREE_NODES : (l.count + MERKLE_THREADS - 1) / MERKLE_THREADS;
}
// the lowest level the launch leaves filled, as its node count: where the next launch reads
inline size_t merkle_launch_filled(const merkle_launch& l) {
    return l.kind == MERKLE_SUBTREE ? l.count / MERKLE_SUBTREE_NODES : l.kind == MERKLE_TOP ? 1 : l.count;
}
