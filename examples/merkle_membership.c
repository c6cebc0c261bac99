/* "x is in this set", the part before the proof: builds the Rescue Merkle tree that the VM's smpath / pmpath authenticate over 2^k leaves
 * derived from a counter (leaf i = (2i + 1, 2i + 2)), writes the root and the secret tapes for one leaf, prints the root.  C99, the header and
 * libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_membership examples/merkle_membership.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_membership <k: 1..26> <index> [device, default 0; -1 = on the host, no GPU] [output prefix, default "membership"]
 *
 * Writes <prefix>.root (32 bytes), <prefix>.tape_a and <prefix>.tape_b (3n - 2 elements of 16 little-endian bytes each, n = k + 1).  The tapes
 * are the `ProgramInputs::new(&[], &a, &b)` of the program
 *   begin read.ab dup.2 smpath.n swap.2 push.<index> roll.4 swap swap.2 pmpath.n end
 * (src/examples/merkle.rs:46-56 of the reference), whose four outputs are (root1, root0, root1, root0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

static void print_element(const uint8_t* e) { int i; for (i = 15; i >= 0; i--) printf("%02x", e[i]); }

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
    unsigned long long index, i, n;
    int device, rc;
    const char* prefix;
    uint8_t *leaves, *tape_a, *tape_b, root[32];
    size_t elems = 0;
    dst_rtree* tree = NULL;
    if (argc < 3) { fprintf(stderr, "usage: %s <k: 1..26> <index> [device | -1 for the host] [output prefix]\n", argv[0]); return 2; }
    k = (unsigned)strtoul(argv[1], NULL, 10);
    index = strtoull(argv[2], NULL, 10);
    device = argc > 3 ? atoi(argv[3]) : 0;
    prefix = argc > 4 ? argv[4] : "membership";
    if (k < 1 || k > 26) { fprintf(stderr, "k must be 1..26\n"); return 2; }
    n = 1ull << k;
    leaves = (uint8_t*)calloc((size_t)n, 32);
    if (!leaves) { fprintf(stderr, "out of memory\n"); return 2; }
    for (i = 0; i < n; i++) {                                   /* leaf i = (2i + 1, 2i + 2), little-endian */
        unsigned long long v0 = 2 * i + 1, v1 = 2 * i + 2;
        int b;
        for (b = 0; b < 8; b++) { leaves[32 * i + b] = (uint8_t)(v0 >> (8 * b)); leaves[32 * i + 16 + b] = (uint8_t)(v1 >> (8 * b)); }
    }
    rc = dst_rtree_build(device, leaves, k, &tree);
    free(leaves);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_build: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    rc = dst_rtree_tapes(tree, index, 3, NULL, NULL, 0, &elems);               /* size query: 3 (k + 1) - 2 */
    if (rc != DST_OK) { fprintf(stderr, "index %llu is not a leaf of a tree of 2^%u leaves\n", index, k); dst_rtree_destroy(tree); return 1; }
    tape_a = (uint8_t*)malloc(16 * elems);
    tape_b = (uint8_t*)malloc(16 * elems);
    if (!tape_a || !tape_b) { fprintf(stderr, "out of memory\n"); free(tape_a); free(tape_b); dst_rtree_destroy(tree); return 2; }
    rc = dst_rtree_root(tree, root);
    if (rc == DST_OK) rc = dst_rtree_tapes(tree, index, 3, tape_a, tape_b, elems, &elems);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree: %d %s\n", rc, dst_rtree_last_error(tree)); free(tape_a); free(tape_b); dst_rtree_destroy(tree); return 1; }
    dst_rtree_destroy(tree);
    if (write_file(prefix, "root", root, 32) || write_file(prefix, "tape_a", tape_a, 16 * elems) || write_file(prefix, "tape_b", tape_b, 16 * elems)) { free(tape_a); free(tape_b); return 1; }
    printf("root "); print_element(root); printf(" "); print_element(root + 16);
    printf("\n%lu elements per tape for leaf %llu, smpath.%u / pmpath.%u\n", (unsigned long)elems, index, k + 1, k + 1);
    free(tape_a); free(tape_b);
    return 0;
}
