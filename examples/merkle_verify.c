/* "checking witnesses": builds the counter tree of merkle_sequence.c (leaf i = (2i + 1, 2i + 2)) over 2^k leaves, applies the same sequence of leaf
 * writes with ONE dst_rtree_apply, and then checks every witness with ONE dst_rescue_verify_writes -- the call a host makes that holds nothing but
 * the root before the sequence: each path with its old leaf resolves to the root before its write, the same siblings with the new leaf to the root
 * after it (compute_merkle_root, src/examples/merkle.rs:112-145 of the reference), and root_after is the state the host holds from then on.  On a
 * device all 2 * writes chains run in one launch, where merkle_sequence.c hashes them one digest at a time.  Then it flips one bit of a sibling and
 * shows what the check reports, and proves membership of a few leaves under the final root with dst_rescue_verify_paths.  C99, the header and
 * libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_verify examples/merkle_verify.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_verify <k: 1..26> <writes: 1..1000> [device, default 0; -1 = on the host, no GPU]
 *
 * Write j goes to leaf (7 j + 3) mod 2^k, except that every fourth write repeats the index of the write before it; its value is
 * (2^64 + j, 2^65 + j). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

static void print_element(const uint8_t* e) { int i; for (i = 15; i >= 0; i--) printf("%02x", e[i]); }
static void print_root(const char* label, const uint8_t* root) { printf("%s ", label); print_element(root); printf(" "); print_element(root + 16); printf("\n"); }

int main(int argc, char** argv) {
    unsigned k, n;
    unsigned long long i, leaves_n;
    unsigned long j, count;
    int device, rc, b;
    uint8_t *leaves, *new_leaves, *paths, *roots, *open3, before[32], after[32], got[32];
    uint64_t *indices, some[3];
    int64_t first_bad = 0;
    uint32_t why = 0;
    dst_rtree* tree = NULL;
    if (argc < 3) { fprintf(stderr, "usage: %s <k: 1..26> <writes: 1..1000> [device | -1 for the host]\n", argv[0]); return 2; }
    k = (unsigned)strtoul(argv[1], NULL, 10);
    count = strtoul(argv[2], NULL, 10);
    device = argc > 3 ? atoi(argv[3]) : 0;
    if (k < 1 || k > 26 || count < 1 || count > 1000) { fprintf(stderr, "k must be 1..26, writes 1..1000\n"); return 2; }
    n = k + 1;
    leaves_n = 1ull << k;
    leaves = (uint8_t*)calloc((size_t)leaves_n, 32);
    new_leaves = (uint8_t*)calloc(count, 32);
    indices = (uint64_t*)calloc(count, sizeof(uint64_t));
    paths = (uint8_t*)calloc(count * n, 32);
    roots = (uint8_t*)calloc(count, 32);
    open3 = (uint8_t*)calloc(3 * (size_t)n, 32);
    if (!leaves || !new_leaves || !indices || !paths || !roots || !open3) { fprintf(stderr, "out of memory\n"); return 2; }
    for (i = 0; i < leaves_n; i++) {                            /* leaf i = (2i + 1, 2i + 2), little-endian */
        unsigned long long v0 = 2 * i + 1, v1 = 2 * i + 2;
        for (b = 0; b < 8; b++) { leaves[32 * i + b] = (uint8_t)(v0 >> (8 * b)); leaves[32 * i + 16 + b] = (uint8_t)(v1 >> (8 * b)); }
    }
    for (j = 0; j < count; j++) {                               /* write j: leaf (7 j + 3) mod 2^k or the one before, value (2^64 + j, 2^65 + j) */
        indices[j] = (j & 3) == 3 ? indices[j - 1] : (7ull * j + 3) & (leaves_n - 1);
        for (b = 0; b < 8; b++) { new_leaves[32 * j + b] = new_leaves[32 * j + 16 + b] = (uint8_t)((unsigned long long)j >> (8 * b)); }
        new_leaves[32 * j + 8] = 1; new_leaves[32 * j + 16 + 8] = 2;
    }
    some[0] = 0; some[1] = leaves_n - 1; some[2] = indices[count - 1];
    rc = dst_rtree_build(device, leaves, k, &tree);
    free(leaves);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_build: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    rc = dst_rtree_root(tree, before);
    if (rc == DST_OK) rc = dst_rtree_apply(tree, indices, new_leaves, count, paths, roots);
    if (rc == DST_OK) rc = dst_rtree_root(tree, got);
    if (rc == DST_OK) rc = dst_rtree_paths(tree, some, 3, open3);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree: %d %s\n", rc, dst_rtree_last_error(tree)); dst_rtree_destroy(tree); return 1; }
    dst_rtree_destroy(tree);
    /* from here on: no tree.  What a client that holds `before` does with the witnesses */
    rc = dst_rescue_verify_writes(device, before, paths, n, indices, new_leaves, roots, count, &first_bad, &why, after, NULL);
    if (rc != DST_OK) { fprintf(stderr, "dst_rescue_verify_writes: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    if (first_bad != -1 || why != DST_PATH_OK) { fprintf(stderr, "write %ld does not verify: %u\n", (long)first_bad, (unsigned)why); return 1; }
    if (memcmp(after, got, 32)) { fprintf(stderr, "root_after is not the tree's root\n"); return 1; }
    print_root("root before", before);
    print_root("root after", after);
    printf("%lu writes, %lu witnesses of %u nodes checked in one call\n", count, count, n);
    /* one flipped bit in the sibling of write count / 2: that write no longer resolves to the root before it */
    paths[32 * ((size_t)n * (count / 2) + 1)] ^= 1;
    rc = dst_rescue_verify_writes(device, before, paths, n, indices, new_leaves, roots, count, &first_bad, &why, NULL, NULL);
    if (rc != DST_OK) { fprintf(stderr, "dst_rescue_verify_writes: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    printf("tampered write %lu: first_bad %ld why %u\n", count / 2, (long)first_bad, (unsigned)why);
    /* membership under the final root: leaves 0 and 2^k - 1 and the leaf of the last write, which holds the value written last */
    rc = dst_rescue_verify_paths(device, after, open3, n, some, NULL, 3, &first_bad, &why, NULL);
    if (rc == DST_OK && first_bad == -1) rc = dst_rescue_verify_paths(device, after, open3 + 32 * 2 * (size_t)n, n, some + 2, new_leaves + 32 * (count - 1), 1, &first_bad, &why, NULL);
    if (rc != DST_OK) { fprintf(stderr, "dst_rescue_verify_paths: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    if (first_bad != -1) { fprintf(stderr, "path %ld does not open under the final root: %u\n", (long)first_bad, (unsigned)why); return 1; }
    printf("3 leaves open under the final root, leaf %llu holds the value of write %lu\n", (unsigned long long)some[2], count - 1);
    free(new_leaves); free(indices); free(paths); free(roots); free(open3);
    return 0;
}
