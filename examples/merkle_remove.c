/* "a set that shrinks": a sparse Rescue Merkle tree of depth 63 takes k keys with one dst_stree_set, loses the first m of them with one
 * dst_stree_remove -- the nodes without a key below them are freed, only the surviving ancestors are hashed -- and then loses one more key WITH A
 * WITNESS: dst_stree_apply writes the empty leaf to it and returns the path and the root after the write, dst_rescue_verify_writes checks them as
 * a client that holds only the root would, and dst_stree_compact frees the nodes of the emptied key without changing the root.  dst_stree_get
 * reads the key's leaf before and after.  C99, the header and libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_remove examples/merkle_remove.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_remove <k> <m> [device, default 0; -1 = on the host, no GPU]
 *
 * Key i (i = 0 .. k - 1) is ((i + 1) * 0x9E3779B97F4A7C15) mod 2^63 and its leaf is (2i + 1, 2i + 2), as in merkle_sparse.c; keys 0 .. m - 1 are
 * removed, key m is deleted with a witness; m < k. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

#define DEPTH 63u

static void print_element(const uint8_t* e) { int i; for (i = 15; i >= 0; i--) printf("%02x", e[i]); }
static void print_root(const char* label, const uint8_t* root) { printf("%s ", label); print_element(root); printf(" "); print_element(root + 16); printf("\n"); }
static void print_info(const char* label, const dst_stree_info_t* info) {
    printf("%s: %llu keys in %llu stored nodes, %llu digests\n", label, (unsigned long long)info->keys, (unsigned long long)info->nodes, (unsigned long long)info->last_digests);
}

int main(int argc, char** argv) {
    unsigned long long i, k, m;
    uint64_t *keys, key, removed = 0, compacted = 0;
    int device, rc, b;
    uint8_t *leaves, path[(DEPTH + 1) * 32], root[32], root_before[32], root_after[32], computed[32], empty[32] = {0}, leaf[32], stored = 0;
    int64_t first_bad = 0;
    uint32_t why = 0;
    dst_stree* tree = NULL;
    dst_stree_info_t info;
    if (argc < 3) { fprintf(stderr, "usage: %s <k> <m> [device | -1 for the host]\n", argv[0]); return 2; }
    k = strtoull(argv[1], NULL, 10);
    m = strtoull(argv[2], NULL, 10);
    device = argc > 3 ? atoi(argv[3]) : 0;
    if (k < 1 || k > (1ull << 24) || m >= k) { fprintf(stderr, "1 <= k <= 2^24 and m < k\n"); return 2; }
    keys = (uint64_t*)malloc((size_t)k * sizeof(uint64_t));
    leaves = (uint8_t*)calloc((size_t)k, 32);
    if (!keys || !leaves) { fprintf(stderr, "out of memory\n"); return 2; }
    for (i = 0; i < k; i++) {                                   /* leaf i = (2i + 1, 2i + 2), little-endian */
        unsigned long long v0 = 2 * i + 1, v1 = 2 * i + 2;
        keys[i] = ((i + 1) * 0x9E3779B97F4A7C15ull) & ((1ull << DEPTH) - 1);
        for (b = 0; b < 8; b++) { leaves[32 * i + b] = (uint8_t)(v0 >> (8 * b)); leaves[32 * i + 16 + b] = (uint8_t)(v1 >> (8 * b)); }
    }
    key = keys[m];
    rc = dst_stree_create(device, DEPTH, NULL, &tree);          /* the empty leaf is (0, 0) */
    if (rc != DST_OK) { fprintf(stderr, "dst_stree_create: %d %s\n", rc, dst_stree_last_error(NULL)); return 1; }
    rc = dst_stree_set(tree, keys, leaves, (size_t)k);
    if (rc == DST_OK) rc = dst_stree_root(tree, root);
    if (rc == DST_OK) rc = dst_stree_info(tree, &info);
    if (rc == DST_OK) { print_root("root", root); print_info("set", &info); }

    if (rc == DST_OK) rc = dst_stree_remove(tree, keys, (size_t)m, &removed);                      /* keys 0 .. m - 1 leave, and their nodes */
    if (rc == DST_OK) rc = dst_stree_root(tree, root_before);
    if (rc == DST_OK) rc = dst_stree_info(tree, &info);
    if (rc == DST_OK) { print_root("root after remove", root_before); printf("%llu removed\n", (unsigned long long)removed); print_info("remove", &info); }

    if (rc == DST_OK) rc = dst_stree_apply(tree, &key, empty, 1, path, root_after);                /* key m <- the empty leaf, with its witness */
    if (rc == DST_OK) {
        rc = dst_rescue_verify_writes(device, root_before, path, DEPTH + 1, &key, empty, root_after, 1, &first_bad, &why, computed, NULL);
        if (rc != DST_OK) { fprintf(stderr, "dst_rescue_verify_writes: %d %s\n", rc, dst_rtree_last_error(NULL)); dst_stree_destroy(tree); return 1; }
        print_root("root after the witnessed deletion", root_after);
        printf("witness: first_bad %lld why %u, the root follows: %s\n", (long long)first_bad, (unsigned)why, memcmp(computed, root_after, 32) == 0 ? "yes" : "no");
    }
    if (rc == DST_OK) rc = dst_stree_get(tree, &key, 1, leaf, &stored);
    if (rc == DST_OK) rc = dst_stree_info(tree, &info);
    if (rc == DST_OK) printf("before compact: %llu keys in %llu stored nodes, the key is %s and its leaf is %s\n", (unsigned long long)info.keys, (unsigned long long)info.nodes,
                             stored ? "stored" : "not stored", memcmp(leaf, empty, 32) == 0 ? "empty" : "not empty");

    if (rc == DST_OK) rc = dst_stree_compact(tree, &compacted);                                    /* the emptied key's nodes are freed */
    if (rc == DST_OK) rc = dst_stree_root(tree, root);
    if (rc == DST_OK) rc = dst_stree_get(tree, &key, 1, leaf, &stored);
    if (rc == DST_OK) rc = dst_stree_info(tree, &info);
    if (rc != DST_OK) { fprintf(stderr, "dst_stree: %d %s\n", rc, dst_stree_last_error(tree)); dst_stree_destroy(tree); return 1; }
    print_root("root after compact", root);
    printf("%llu compacted\n", (unsigned long long)compacted);
    print_info("compact", &info);
    printf("after compact: the key is %s and its leaf is %s\n", stored ? "stored" : "not stored", memcmp(leaf, empty, 32) == 0 ? "empty" : "not empty");
    dst_stree_destroy(tree);
    free(keys); free(leaves);
    return 0;
}
