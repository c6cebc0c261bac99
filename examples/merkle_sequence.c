/* "ordered writes": builds the counter tree of merkle_membership.c (leaf i = (2i + 1, 2i + 2)) over 2^k leaves and applies a sequence of leaf
 * writes, one index of which repeats, with ONE call of dst_rtree_apply.  Every write comes back with its witness -- the authentication path of
 * its leaf in the tree as the earlier writes left it -- and with the root after it.  Each witness is then checked here as a verifier would: the
 * path with the OLD leaf folds to the previous root and the same siblings with the NEW leaf fold to the returned root, by
 * dst_rescue_digest_many on the host (compute_merkle_root, src/examples/merkle.rs:112-145 of the reference).  C99, the header and
 * libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_sequence examples/merkle_sequence.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_sequence <k: 1..26> <writes: 1..1000> [device, default 0; -1 = on the host, no GPU]
 *
 * Write j goes to leaf (7 j + 3) mod 2^k, except that every fourth write repeats the index of the write before it; its value is
 * (2^64 + j, 2^65 + j).  Prints the root before the sequence and the root after every write. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

static void print_element(const uint8_t* e) { int i; for (i = 15; i >= 0; i--) printf("%02x", e[i]); }
static void print_root(const char* label, unsigned long j, const uint8_t* root) { printf("%s %lu ", label, j); print_element(root); printf(" "); print_element(root + 16); printf("\n"); }

/* the root that `leaf` and the siblings path[1 .. n) give for `index` */
static int fold(const uint8_t* leaf, const uint8_t* path, unsigned n, uint64_t index, uint8_t* root) {
    uint8_t in[64];
    unsigned k;
    memcpy(root, leaf, 32);
    for (k = 1; k < n; k++, index >>= 1) {
        memcpy(in + ((index & 1) ? 32 : 0), root, 32);
        memcpy(in + ((index & 1) ? 0 : 32), path + 32 * k, 32);
        if (dst_rescue_digest_many(-1, in, 1, root) != DST_OK) return -1;
    }
    return 0;
}

int main(int argc, char** argv) {
    unsigned k, n;
    unsigned long long i, leaves_n;
    unsigned long j, count;
    int device, rc, b;
    uint8_t *leaves, *new_leaves, *paths, *roots, before[32], got[32];
    uint64_t* indices;
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
    if (!leaves || !new_leaves || !indices || !paths || !roots) { fprintf(stderr, "out of memory\n"); return 2; }
    for (i = 0; i < leaves_n; i++) {                            /* leaf i = (2i + 1, 2i + 2), little-endian */
        unsigned long long v0 = 2 * i + 1, v1 = 2 * i + 2;
        for (b = 0; b < 8; b++) { leaves[32 * i + b] = (uint8_t)(v0 >> (8 * b)); leaves[32 * i + 16 + b] = (uint8_t)(v1 >> (8 * b)); }
    }
    for (j = 0; j < count; j++) {                               /* write j: leaf (7 j + 3) mod 2^k or the one before, value (2^64 + j, 2^65 + j) */
        indices[j] = (j & 3) == 3 ? indices[j - 1] : (7ull * j + 3) & (leaves_n - 1);
        for (b = 0; b < 8; b++) { new_leaves[32 * j + b] = new_leaves[32 * j + 16 + b] = (uint8_t)((unsigned long long)j >> (8 * b)); }
        new_leaves[32 * j + 8] = 1; new_leaves[32 * j + 16 + 8] = 2;
    }
    rc = dst_rtree_build(device, leaves, k, &tree);
    free(leaves);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_build: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    rc = dst_rtree_root(tree, before);
    if (rc == DST_OK) rc = dst_rtree_apply(tree, indices, new_leaves, count, paths, roots);
    if (rc == DST_OK) rc = dst_rtree_root(tree, got);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree: %d %s\n", rc, dst_rtree_last_error(tree)); dst_rtree_destroy(tree); return 1; }
    dst_rtree_destroy(tree);
    if (memcmp(got, roots + 32 * (count - 1), 32)) { fprintf(stderr, "the tree's root is not the last returned root\n"); return 1; }
    print_root("root before", 0, before);
    for (j = 0; j < count; j++) {
        const uint8_t* path = paths + 32 * (size_t)n * j;
        if (fold(path, path, n, indices[j], got) || memcmp(got, j ? roots + 32 * (j - 1) : before, 32)) { fprintf(stderr, "write %lu: the old leaf does not open under the previous root\n", j); return 1; }
        if (fold(new_leaves + 32 * j, path, n, indices[j], got) || memcmp(got, roots + 32 * j, 32)) { fprintf(stderr, "write %lu: the new leaf does not open under the returned root\n", j); return 1; }
        print_root("root after write", j, roots + 32 * j);
    }
    printf("%lu writes, %lu witnesses of %u nodes checked\n", count, count, n);
    free(new_leaves); free(indices); free(paths); free(roots);
    return 0;
}
