/* "the set changes": builds the counter tree of merkle_membership.c (leaf i = (2i + 1, 2i + 2)) over 2^k leaves, replaces one leaf in place with
 * dst_rtree_update -- only the k ancestors of that leaf are hashed again, the tree is not rebuilt -- prints the root before and after, and writes
 * the secret tapes of that leaf and of a second one with ONE call of dst_rtree_tapes_many.  C99, the header and libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_update examples/merkle_update.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_update <k: 1..26> <index> <second index> [device, default 0; -1 = on the host, no GPU] [output prefix, default "update"]
 *
 * The new leaf is (2^64 + index, 2^65 + index), which no counter leaf equals.  Writes <prefix>.root (32 bytes, the new root) and <prefix>.tape_a /
 * <prefix>.tape_b: two blocks of 3n - 2 elements of 16 little-endian bytes each, n = k + 1, the first for <index>, the second for <second index>.
 * Each block is the `ProgramInputs::new(&[], &a, &b)` of the program of merkle_membership.c for its index (src/examples/merkle.rs:46-94 of the
 * reference). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

static void print_element(const uint8_t* e) { int i; for (i = 15; i >= 0; i--) printf("%02x", e[i]); }
static void print_root(const char* label, const uint8_t* root) { printf("%s ", label); print_element(root); printf(" "); print_element(root + 16); printf("\n"); }

static int write_file(const char* prefix, const char* suffix, const uint8_t* data, size_t bytes) {
    char name[512];
    FILE* f;
    snprintf(name, sizeof(name), "%s.%s", prefix, suffix);
    f = fopen(name, "wb");
    if (!f || fwrite(data, 1, bytes, f) != bytes) { perror(name); if (f) fclose(f); return -1; }
    return fclose(f);
}

int main(int argc, char** argv) {
    unsigned k;
    unsigned long long i, n;
    uint64_t indices[2];
    int device, rc, b;
    const char* prefix;
    uint8_t *leaves, *tape_a = NULL, *tape_b = NULL, old_root[32], new_root[32], leaf[32];
    size_t each = 0;
    dst_rtree* tree = NULL;
    if (argc < 4) { fprintf(stderr, "usage: %s <k: 1..26> <index> <second index> [device | -1 for the host] [output prefix]\n", argv[0]); return 2; }
    k = (unsigned)strtoul(argv[1], NULL, 10);
    indices[0] = strtoull(argv[2], NULL, 10);
    indices[1] = strtoull(argv[3], NULL, 10);
    device = argc > 4 ? atoi(argv[4]) : 0;
    prefix = argc > 5 ? argv[5] : "update";
    if (k < 1 || k > 26) { fprintf(stderr, "k must be 1..26\n"); return 2; }
    n = 1ull << k;
    leaves = (uint8_t*)calloc((size_t)n, 32);
    if (!leaves) { fprintf(stderr, "out of memory\n"); return 2; }
    for (i = 0; i < n; i++) {                                   /* leaf i = (2i + 1, 2i + 2), little-endian */
        unsigned long long v0 = 2 * i + 1, v1 = 2 * i + 2;
        for (b = 0; b < 8; b++) { leaves[32 * i + b] = (uint8_t)(v0 >> (8 * b)); leaves[32 * i + 16 + b] = (uint8_t)(v1 >> (8 * b)); }
    }
    rc = dst_rtree_build(device, leaves, k, &tree);
    free(leaves);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_build: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    memset(leaf, 0, sizeof(leaf));                              /* the new leaf: (2^64 + index, 2^65 + index) */
    for (b = 0; b < 8; b++) { leaf[b] = leaf[16 + b] = (uint8_t)(indices[0] >> (8 * b)); }
    leaf[8] = 1; leaf[16 + 8] = 2;
    rc = dst_rtree_root(tree, old_root);
    if (rc == DST_OK) rc = dst_rtree_update(tree, indices, leaf, 1);           /* an index past the end is refused here, the tree stays as it was */
    if (rc == DST_OK) rc = dst_rtree_root(tree, new_root);
    if (rc == DST_OK) rc = dst_rtree_tapes_many(tree, indices, 2, 3, NULL, NULL, 0, &each);       /* size query: 3 (k + 1) - 2 per leaf */
    if (rc == DST_OK) {
        tape_a = (uint8_t*)malloc(2 * 16 * each);
        tape_b = (uint8_t*)malloc(2 * 16 * each);
        if (!tape_a || !tape_b) { fprintf(stderr, "out of memory\n"); free(tape_a); free(tape_b); dst_rtree_destroy(tree); return 2; }
        rc = dst_rtree_tapes_many(tree, indices, 2, 3, tape_a, tape_b, each, &each);
    }
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree: %d %s\n", rc, dst_rtree_last_error(tree)); free(tape_a); free(tape_b); dst_rtree_destroy(tree); return 1; }
    dst_rtree_destroy(tree);
    if (write_file(prefix, "root", new_root, 32) || write_file(prefix, "tape_a", tape_a, 2 * 16 * each) || write_file(prefix, "tape_b", tape_b, 2 * 16 * each)) { free(tape_a); free(tape_b); return 1; }
    print_root("old root", old_root);
    print_root("new root", new_root);
    printf("%lu elements per tape and leaf, leaves %llu and %llu, smpath.%u / pmpath.%u\n", (unsigned long)each, (unsigned long long)indices[0], (unsigned long long)indices[1], k + 1, k + 1);
    free(tape_a); free(tape_b);
    return 0;
}
