// Stand-alone print-out of distaff_amd/csrc/host/merkle_plan.h (which kernel builds which level of a BLAKE3 tree): for every case on standard
// input, "a in_place stop_log level2_log levels_only", the launches of the tree over 2^a children as k_merkle (kernels_hash.hip) issues them --
// profiling name, profiling bytes, grid.x, block.x, the kernel's count argument, where it reads ("leaves" or an offset into the node array) and
// the lowest offset it writes.  stop_log < 0: to the root; level2_log < 0: the default width.  Built with -fsanitize=address,undefined by
// tests/test_merkle_launch_plan.py, which compares the lines with what the launch code printed before the plan existed.
#include <cstdio>
#include "host/merkle_plan.h"

int main() {
    int a, in_place, stop_log, level2_log, levels_only;
    while (scanf("%d %d %d %d %d", &a, &in_place, &stop_log, &level2_log, &levels_only) == 5) {
        printf("# %d %d %d %d %d\n", a, in_place, stop_log, level2_log, levels_only);
        const size_t count = (size_t)1 << a, stop_count = stop_log < 0 ? 0 : (size_t)1 << stop_log;
        const size_t level2_min = level2_log < 0 ? MERKLE_LEVEL2_MIN : (size_t)1 << level2_log;
        size_t filled = count;                                // the level the next launch reads
        bool leaves = !in_place;
        for (const merkle_launch& l : merkle_plan(count, in_place != 0, stop_count, level2_min, levels_only != 0)) {
            // the lowest node written: the parents (level), the parents below the grandparents (level2), the first of nine levels (subtree), nodes[0] (top)
            const size_t dst = l.kind == MERKLE_LEVEL ? l.count : l.kind == MERKLE_LEVEL2 ? 2 * l.count : l.kind == MERKLE_SUBTREE ? l.count / 2 : 0;
            printf("%s %.0f %zu %u %zu ", merkle_launch_name(l), merkle_launch_bytes(l), merkle_launch_blocks(l), MERKLE_THREADS, l.count);
            if (leaves) printf("leaves %zu\n", dst); else printf("%zu %zu\n", filled, dst);
            filled = merkle_launch_filled(l);
            leaves = false;
        }
    }
    return 0;
}
