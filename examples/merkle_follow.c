/* "following writes with held paths": a client holds the root of a tree and the authentication paths of three leaves of its own.  Somebody else
 * owns the tree and applies two batches of ordered writes to it (dst_rtree_apply), which return one witness per write.  The client never sees the
 * tree: with ONE dst_rescue_refresh_paths per batch it checks the witnesses, moves its root forward and turns its three paths into its paths under
 * the new root -- in place.  Here the owner's side runs first and every handle that could open a path again is destroyed before the client starts;
 * at the end the client's paths are compared with the paths the tree reported before it went.  The batches write to a held leaf, to the sibling
 * of a held leaf, and to one key twice.  C99, the header and libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_follow examples/merkle_follow.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_follow [device, default 0; -1 = on the host, no GPU]
 *
 * 16 leaves, leaf i = (i + 1, 2 i + 1); the client holds leaves 3, 9 and 12.  Write j of batch b has the value (100 (b + 1) + j, 100 (b + 1) + 50 + j). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

#define K 4
#define N (K + 1)                 /* nodes of a path */
#define HELD 3
#define BATCHES 2
#define MOST 6                    /* writes of the longer batch */

static void print_element(const uint8_t* e) { int i; for (i = 15; i >= 0; i--) printf("%02x", e[i]); }
static void print_node(const uint8_t* node) { print_element(node); printf(" "); print_element(node + 16); printf("\n"); }
static void put_node(uint8_t* node, unsigned v0, unsigned v1) {
    memset(node, 0, 32);
    node[0] = (uint8_t)v0; node[1] = (uint8_t)(v0 >> 8); node[16] = (uint8_t)v1; node[17] = (uint8_t)(v1 >> 8);
}

int main(int argc, char** argv) {
    static const uint64_t held[HELD] = {3, 9, 12};
    static const uint64_t writes[BATCHES][MOST] = {{3, 2, 8, 3, 13, 0}, {9, 8, 8, 12, 13, 0}};      /* a held leaf, its sibling, a key twice */
    static const size_t counts[BATCHES] = {5, 6};
    static uint8_t leaves[32 << K], new_leaves[BATCHES][32 * MOST], witnesses[BATCHES][32 * N * MOST], roots[BATCHES][32 * MOST];
    static uint8_t mine[32 * N * HELD], theirs[32 * N * HELD];
    uint8_t root[32], next_root[32];
    int64_t first_bad = 0;
    uint32_t why = 0;
    size_t total = 0;
    unsigned i, j, b;
    int rc, device = argc > 1 ? atoi(argv[1]) : 0;
    dst_rtree* tree = NULL;
    /* ---- the owner of the tree ---- */
    for (i = 0; i < (1u << K); i++) put_node(leaves + 32 * i, i + 1, 2 * i + 1);
    rc = dst_rtree_build(device, leaves, K, &tree);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_build: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    rc = dst_rtree_root(tree, root);                                          /* what the client starts from: the root and its three paths */
    if (rc == DST_OK) rc = dst_rtree_paths(tree, held, HELD, mine);
    for (b = 0; b < BATCHES && rc == DST_OK; b++) {
        for (j = 0; j < counts[b]; j++) put_node(new_leaves[b] + 32 * j, 100 * (b + 1) + j, 100 * (b + 1) + 50 + j);
        rc = dst_rtree_apply(tree, writes[b], new_leaves[b], counts[b], witnesses[b], roots[b]);
    }
    if (rc == DST_OK) rc = dst_rtree_paths(tree, held, HELD, theirs);         /* kept for the comparison at the end only */
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree: %d %s\n", rc, dst_rtree_last_error(tree)); dst_rtree_destroy(tree); return 1; }
    dst_rtree_destroy(tree);
    /* ---- the client: a root, three paths and the witnesses; no tree from here on ---- */
    printf("root before "); print_node(root);
    for (b = 0; b < BATCHES; b++) {
        rc = dst_rescue_refresh_paths(device, root, witnesses[b], N, writes[b], new_leaves[b], roots[b], counts[b], held, mine, HELD, mine, &first_bad, &why, next_root, NULL);
        if (rc != DST_OK) { fprintf(stderr, "dst_rescue_refresh_paths: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
        if (first_bad != -1 || why != DST_PATH_OK) { fprintf(stderr, "batch %u: write %ld does not verify: %u\n", b, (long)first_bad, (unsigned)why); return 1; }
        memcpy(root, next_root, 32);
        printf("batch %u: %lu writes followed, root ", b, (unsigned long)counts[b]); print_node(root);
        total += counts[b];
    }
    for (i = 0; i < HELD; i++)
        for (j = 0; j < N; j++) { printf("leaf %lu node %u ", (unsigned long)held[i], j); print_node(mine + 32 * (N * i + j)); }
    if (memcmp(mine, theirs, sizeof mine)) { fprintf(stderr, "the refreshed paths are not the tree's paths\n"); return 1; }
    rc = dst_rescue_verify_paths(device, root, mine, N, held, NULL, HELD, &first_bad, &why, NULL);      /* and they open under the root the client computed */
    if (rc != DST_OK || first_bad != -1) { fprintf(stderr, "dst_rescue_verify_paths: %d, path %ld: %u\n", rc, (long)first_bad, (unsigned)why); return 1; }
    printf("%d held paths of %d nodes equal the tree's after %lu writes\n", HELD, N, (unsigned long)total);
    return 0;
}
