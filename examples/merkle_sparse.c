/* "a set addressed by a key": builds a sparse Rescue Merkle tree of depth D (keys below 2^D, D up to 63) from k keys with ONE dst_stree_set, prints
 * the root, writes the secret tapes of one key that is stored and of one that is not -- the second is a proof that the key is empty: its path
 * starts with the empty leaf (0, 0) -- with ONE call of dst_stree_tapes_many, then inserts m more keys (only their ancestors are hashed) and prints
 * the new root.  C99, the header and libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_sparse examples/merkle_sparse.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_sparse <depth: 1..63> <k> <m> [device, default 0; -1 = on the host, no GPU] [output prefix, default "sparse"]
 *
 * Key i (i = 0 .. k + m) is ((i + 1) * 0x9E3779B97F4A7C15) mod 2^depth -- distinct while k + m + 1 <= 2^depth, the multiplier being odd -- and
 * its leaf is (2i + 1, 2i + 2).  The stored key of the tapes is key 0, the absent one key k + m (never inserted).  Writes <prefix>.root (32 bytes,
 * the first root) and <prefix>.tape_a / <prefix>.tape_b: two blocks of 3n - 2 elements of 16 little-endian bytes, n = depth + 1, the first for the
 * stored key, the second for the absent one.  Each block is the `ProgramInputs::new(&[], &a, &b)` of the program
 * `read.ab dup.2 smpath.n swap.2 push.<key> roll.4 swap swap.2 pmpath.n` (src/examples/merkle.rs:46-94 of the reference). */
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
    unsigned depth;
    unsigned long long i, k, m, mask;
    uint64_t *keys, ask[2];
    int device, rc, b;
    const char* prefix;
    uint8_t *leaves, *tape_a = NULL, *tape_b = NULL, root[32], new_root[32];
    size_t each = 0;
    dst_stree* tree = NULL;
    dst_stree_info_t info;
    if (argc < 4) { fprintf(stderr, "usage: %s <depth: 1..63> <k> <m> [device | -1 for the host] [output prefix]\n", argv[0]); return 2; }
    depth = (unsigned)strtoul(argv[1], NULL, 10);
    k = strtoull(argv[2], NULL, 10);
    m = strtoull(argv[3], NULL, 10);
    device = argc > 4 ? atoi(argv[4]) : 0;
    prefix = argc > 5 ? argv[5] : "sparse";
    if (depth < 1 || depth > 63) { fprintf(stderr, "depth must be 1..63\n"); return 2; }
    mask = (1ull << depth) - 1;
    if (k < 1 || k + m > (1ull << 30) || k + m + 1 > mask + 1) { fprintf(stderr, "1 <= k and k + m + 1 <= min(2^30, 2^depth)\n"); return 2; }
    keys = (uint64_t*)malloc((size_t)(k + m + 1) * sizeof(uint64_t));
    leaves = (uint8_t*)calloc((size_t)(k + m), 32);
    if (!keys || !leaves) { fprintf(stderr, "out of memory\n"); return 2; }
    for (i = 0; i <= k + m; i++) keys[i] = ((i + 1) * 0x9E3779B97F4A7C15ull) & mask;
    for (i = 0; i < k + m; i++) {                               /* leaf i = (2i + 1, 2i + 2), little-endian */
        unsigned long long v0 = 2 * i + 1, v1 = 2 * i + 2;
        for (b = 0; b < 8; b++) { leaves[32 * i + b] = (uint8_t)(v0 >> (8 * b)); leaves[32 * i + 16 + b] = (uint8_t)(v1 >> (8 * b)); }
    }
    ask[0] = keys[0]; ask[1] = keys[k + m];
    rc = dst_stree_create(device, depth, NULL, &tree);
    if (rc != DST_OK) { fprintf(stderr, "dst_stree_create: %d %s\n", rc, dst_stree_last_error(NULL)); return 1; }
    rc = dst_stree_set(tree, keys, leaves, (size_t)k);                                             /* building a tree is create + one set */
    if (rc == DST_OK) rc = dst_stree_root(tree, root);
    if (rc == DST_OK) rc = dst_stree_tapes_many(tree, ask, 2, 3, NULL, NULL, 0, &each);           /* size query: 3 (depth + 1) - 2 per key */
    if (rc == DST_OK) {
        tape_a = (uint8_t*)malloc(2 * 16 * each);
        tape_b = (uint8_t*)malloc(2 * 16 * each);
        if (!tape_a || !tape_b) { fprintf(stderr, "out of memory\n"); free(tape_a); free(tape_b); dst_stree_destroy(tree); return 2; }
        rc = dst_stree_tapes_many(tree, ask, 2, 3, tape_a, tape_b, each, &each);
    }
    if (rc == DST_OK) rc = dst_stree_set(tree, keys + k, leaves + 32 * k, (size_t)m);              /* the set grows: m keys more */
    if (rc == DST_OK) rc = dst_stree_root(tree, new_root);
    if (rc == DST_OK) rc = dst_stree_info(tree, &info);
    if (rc != DST_OK) { fprintf(stderr, "dst_stree: %d %s\n", rc, dst_stree_last_error(tree)); free(tape_a); free(tape_b); dst_stree_destroy(tree); return 1; }
    dst_stree_destroy(tree);
    free(keys); free(leaves);
    if (write_file(prefix, "root", root, 32) || write_file(prefix, "tape_a", tape_a, 2 * 16 * each) || write_file(prefix, "tape_b", tape_b, 2 * 16 * each)) { free(tape_a); free(tape_b); return 1; }
    print_root("root", root);
    print_root("new root", new_root);
    printf("%llu keys in %llu stored nodes, %llu digests for the last %llu keys; %lu elements per tape and key, stored key %llu, absent key %llu, smpath.%u / pmpath.%u\n",
           (unsigned long long)info.keys, (unsigned long long)info.nodes, (unsigned long long)info.last_digests, m, (unsigned long)each,
           (unsigned long long)ask[0], (unsigned long long)ask[1], depth + 1, depth + 1);
    free(tape_a); free(tape_b);
    return 0;
}
