/* "a set addressed by a hash": a wide-key sparse Rescue Merkle tree (dst_wtree_*, depth 127) whose keys are derived by hashing, as account
 * addresses, note commitments and nullifiers are.  Key i is the first element of dst_rescue_digest_many over (i, 1, 2, 3) masked to 127 bits --
 * a 16-byte little-endian integer, the layout of a field element -- and its leaf is (2i + 1, 2i + 2).  ONE dst_wtree_set inserts k keys; key 0,
 * a member, and key k, never inserted, are opened with ONE dst_wtree_paths and checked against the root alone with dst_rescue_verify_paths_w:
 * the member against its leaf, the other against the empty leaf (0, 0), which proves that the key is absent.  Their secret tapes are printed:
 * each is the `ProgramInputs::new(&[], &a, &b)` of `read.ab dup.2 smpath.128 swap.2 push.<key> roll.4 swap swap.2 pmpath.128`
 * (src/examples/merkle.rs:46-94 of the reference).  C99, the header and libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_wide examples/merkle_wide.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_wide <k> [device, default 0; -1 = on the host, no GPU] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

#define DEPTH 127u
#define NODES (DEPTH + 1u)

static void print_element(const uint8_t* e) { int i; for (i = 15; i >= 0; i--) printf("%02x", e[i]); }
static void put_u64(uint8_t* at, unsigned long long v) { int b; for (b = 0; b < 8; b++) at[b] = (uint8_t)(v >> (8 * b)); }

int main(int argc, char** argv) {
    unsigned long long i, k;
    int device, rc;
    uint8_t *in, *digests, *keys, *leaves, *paths, *tape_a = NULL, *tape_b = NULL, root[32], want[2 * 32];
    size_t each = 0, e;
    int64_t first_bad = 0;
    uint32_t why = 0;
    dst_wtree* tree = NULL;
    dst_stree_info_t info;
    if (argc < 2) { fprintf(stderr, "usage: %s <k> [device | -1 for the host]\n", argv[0]); return 2; }
    k = strtoull(argv[1], NULL, 10);
    device = argc > 2 ? atoi(argv[2]) : 0;
    if (k < 1 || k > (1ull << 20)) { fprintf(stderr, "1 <= k <= 2^20\n"); return 2; }
    in = (uint8_t*)calloc((size_t)(k + 1), 64);
    digests = (uint8_t*)malloc((size_t)(k + 1) * 32);
    keys = (uint8_t*)malloc((size_t)(k + 1) * 16);
    leaves = (uint8_t*)calloc((size_t)k, 32);
    paths = (uint8_t*)malloc(2 * NODES * 32);
    if (!in || !digests || !keys || !leaves || !paths) { fprintf(stderr, "out of memory\n"); return 2; }
    for (i = 0; i <= k; i++) { put_u64(in + 64 * i, i); in[64 * i + 16] = 1; in[64 * i + 32] = 2; in[64 * i + 48] = 3; }
    rc = dst_rescue_digest_many(device, in, (size_t)(k + 1), digests);
    if (rc != DST_OK) { fprintf(stderr, "dst_rescue_digest_many: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    for (i = 0; i <= k; i++) { memcpy(keys + 16 * i, digests + 32 * i, 16); keys[16 * i + 15] &= 0x7f; }     /* one element, masked to 127 bits */
    for (i = 0; i < k; i++) { put_u64(leaves + 32 * i, 2 * i + 1); put_u64(leaves + 32 * i + 16, 2 * i + 2); }
    rc = dst_wtree_create(device, DEPTH, NULL, &tree);
    if (rc != DST_OK) { fprintf(stderr, "dst_wtree_create: %d %s\n", rc, dst_wtree_last_error(NULL)); return 1; }
    memcpy(in, keys, 16); memcpy(in + 16, keys + 16 * k, 16);                                                 /* the two keys asked: a member, an absent one */
    rc = dst_wtree_set(tree, keys, leaves, (size_t)k);                                                        /* building a tree is create + one set */
    if (rc == DST_OK) rc = dst_wtree_root(tree, root);
    if (rc == DST_OK) rc = dst_wtree_paths(tree, in, 2, paths);
    if (rc == DST_OK) rc = dst_wtree_tapes_many(tree, in, 2, 3, NULL, NULL, 0, &each);                        /* size query: 3 * 128 - 2 per key */
    if (rc == DST_OK) {
        tape_a = (uint8_t*)malloc(2 * 16 * each);
        tape_b = (uint8_t*)malloc(2 * 16 * each);
        if (!tape_a || !tape_b) { fprintf(stderr, "out of memory\n"); dst_wtree_destroy(tree); return 2; }
        rc = dst_wtree_tapes_many(tree, in, 2, 3, tape_a, tape_b, each, &each);
    }
    if (rc == DST_OK) rc = dst_wtree_info(tree, &info);
    if (rc != DST_OK) { fprintf(stderr, "dst_wtree: %d %s\n", rc, dst_wtree_last_error(tree)); dst_wtree_destroy(tree); return 1; }
    dst_wtree_destroy(tree);
    /* a client that holds the root alone: the member's path starts with its leaf, the other's with the empty leaf */
    memcpy(want, leaves, 32); memset(want + 32, 0, 32);
    rc = dst_rescue_verify_paths_w(device, root, paths, NODES, in, want, 2, &first_bad, &why, NULL);
    if (rc != DST_OK) { fprintf(stderr, "dst_rescue_verify_paths_w: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    if (first_bad != -1) { fprintf(stderr, "path %ld does not verify: why = %u\n", (long)first_bad, why); return 1; }
    in[15] ^= 0x40;                                                                                           /* the member's path under another key: bit 126 */
    rc = dst_rescue_verify_paths_w(device, root, paths, NODES, in, want, 2, &first_bad, &why, NULL);
    if (rc != DST_OK || first_bad != 0 || why != DST_PATH_BAD_ROOT) { fprintf(stderr, "a path verified under the wrong key\n"); return 1; }
    in[15] ^= 0x40;
    printf("root "); print_element(root); printf(" "); print_element(root + 16); printf("\n");
    printf("%llu keys of 127 bits in %llu stored nodes, %llu digests\n", (unsigned long long)info.keys, (unsigned long long)info.nodes, (unsigned long long)info.last_digests);
    printf("member "); print_element(in); printf(" and absent key "); print_element(in + 16); printf(" verified against the root alone; the wrong key is rejected\n");
    for (i = 0; i < 2; i++) {
        printf("%s tape a:", i ? "absent" : "member");
        for (e = 0; e < each; e++) { printf(" "); print_element(tape_a + 16 * (each * i + e)); }
        printf("\n%s tape b:", i ? "absent" : "member");
        for (e = 0; e < each; e++) { printf(" "); print_element(tape_b + 16 * (each * i + e)); }
        printf("\n");
    }
    printf("%lu elements per tape and key, smpath.%u / pmpath.%u\n", (unsigned long)each, NODES, NODES);
    free(in); free(digests); free(keys); free(leaves); free(paths); free(tape_a); free(tape_b);
    return 0;
}
