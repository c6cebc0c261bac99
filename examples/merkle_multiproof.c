/* "one proof for many leaves": builds the counter tree of merkle_verify.c (leaf i = (2i + 1, 2i + 2)) over 2^k leaves, takes ONE multiproof of a
 * set of leaves with dst_rtree_multiproof -- the leaves and only those sibling nodes that cannot be recomputed from them, every node once, where
 * dst_rtree_paths ships a whole path per leaf -- and then does what a client that holds nothing but the root does with it: checks it with
 * dst_rescue_verify_multiproof, which hashes every ancestor the paths share once, sees a tampered node rejected, and expands it with
 * dst_rescue_multiproof_paths into the full authentication paths that dst_rescue_path_tapes turns into the secret tapes of smpath.n / pmpath.n.
 * The expanded paths are compared with dst_rtree_paths' byte for byte.  C99, the header and libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_multiproof examples/merkle_multiproof.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_multiproof <k: 1..26> <candidates: 1..100000> [device, default 0; -1 = on the host, no GPU]
 *
 * The set is the distinct values of (7 j^2 + 3 j + 1) mod 2^k for j < candidates, in ascending order.  Exit status 0 when everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

static int ascending(const void* a, const void* b) {
    const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
    return x < y ? -1 : x > y;
}

int main(int argc, char** argv) {
    unsigned k, n;
    unsigned long long i, leaves_n;
    unsigned long j, candidates;
    size_t count = 0, num_nodes = 0;
    int device, rc, b, ok = 0;
    uint8_t *leaves, *set_leaves, *nodes, *paths, *expanded, root[32], got[32];
    uint64_t *indices, digests = 0;
    dst_rtree* tree = NULL;
    if (argc < 3) { fprintf(stderr, "usage: %s <k: 1..26> <candidates: 1..100000> [device | -1 for the host]\n", argv[0]); return 2; }
    k = (unsigned)strtoul(argv[1], NULL, 10);
    candidates = strtoul(argv[2], NULL, 10);
    device = argc > 3 ? atoi(argv[3]) : 0;
    if (k < 1 || k > 26 || candidates < 1 || candidates > 100000) { fprintf(stderr, "k must be 1..26, candidates 1..100000\n"); return 2; }
    n = k + 1;
    leaves_n = 1ull << k;
    leaves = (uint8_t*)calloc((size_t)leaves_n, 32);
    indices = (uint64_t*)calloc(candidates, sizeof(uint64_t));
    if (!leaves || !indices) { fprintf(stderr, "out of memory\n"); return 2; }
    for (i = 0; i < leaves_n; i++) {                            /* leaf i = (2i + 1, 2i + 2), little-endian */
        unsigned long long v0 = 2 * i + 1, v1 = 2 * i + 2;
        for (b = 0; b < 8; b++) { leaves[32 * i + b] = (uint8_t)(v0 >> (8 * b)); leaves[32 * i + 16 + b] = (uint8_t)(v1 >> (8 * b)); }
    }
    for (j = 0; j < candidates; j++) indices[j] = (7ull * j * j + 3ull * j + 1) & (leaves_n - 1);
    qsort(indices, candidates, sizeof(uint64_t), ascending);
    for (j = 0; j < candidates; j++) if (count == 0 || indices[count - 1] != indices[j]) indices[count++] = indices[j];      /* a multiproof is of DISTINCT leaves */
    rc = dst_rtree_build(device, leaves, k, &tree);
    free(leaves);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_build: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    /* the tree's side: the size query, the multiproof, and -- for the comparison at the end only -- the full paths */
    rc = dst_rtree_multiproof(tree, indices, count, NULL, NULL, 0, &num_nodes);
    set_leaves = (uint8_t*)calloc(count, 32);
    nodes = (uint8_t*)calloc(num_nodes + 1, 32);
    paths = (uint8_t*)calloc(count * n, 32);
    expanded = (uint8_t*)calloc(count * n, 32);
    if (!set_leaves || !nodes || !paths || !expanded) { fprintf(stderr, "out of memory\n"); return 2; }
    if (rc == DST_OK) rc = dst_rtree_multiproof(tree, indices, count, set_leaves, nodes, num_nodes, &num_nodes);
    if (rc == DST_OK) rc = dst_rtree_paths(tree, indices, count, paths);
    if (rc == DST_OK) rc = dst_rtree_root(tree, root);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree: %d %s\n", rc, dst_rtree_last_error(tree)); dst_rtree_destroy(tree); return 1; }
    dst_rtree_destroy(tree);
    printf("%lu leaves of 2^%u: multiproof %lu bytes against %lu bytes of paths\n", (unsigned long)count, k, (unsigned long)(32 * (count + num_nodes)), (unsigned long)(32 * count * n));
    /* from here on: no tree.  What a client that holds `root` does with (indices, set_leaves, nodes) */
    rc = dst_rescue_verify_multiproof(device, root, n, indices, set_leaves, count, nodes, num_nodes, &ok, NULL);
    if (rc == DST_OK) rc = dst_rescue_multiproof_root(device, n, indices, set_leaves, count, nodes, num_nodes, got, &digests, NULL);
    if (rc != DST_OK) { fprintf(stderr, "dst_rescue_verify_multiproof: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    if (!ok || memcmp(got, root, 32)) { fprintf(stderr, "the multiproof does not resolve to the root\n"); return 1; }
    printf("verified against the root alone: %lu digests against %lu\n", (unsigned long)digests, (unsigned long)(count * k));
    set_leaves[0] ^= 1;                                         /* one flipped bit: not an error, ok = 0 */
    rc = dst_rescue_verify_multiproof(device, root, n, indices, set_leaves, count, nodes, num_nodes, &ok, NULL);
    set_leaves[0] ^= 1;
    if (rc == DST_OK && !ok && num_nodes) {
        nodes[32 * (num_nodes - 1) + 16] ^= 1;
        rc = dst_rescue_verify_multiproof(device, root, n, indices, set_leaves, count, nodes, num_nodes, &ok, NULL);
        nodes[32 * (num_nodes - 1) + 16] ^= 1;
    }
    if (rc != DST_OK) { fprintf(stderr, "dst_rescue_verify_multiproof: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    if (ok) { fprintf(stderr, "a tampered multiproof was accepted\n"); return 1; }
    printf("a tampered node is rejected\n");
    rc = dst_rescue_multiproof_paths(device, n, indices, set_leaves, count, nodes, num_nodes, expanded, got, NULL);
    if (rc != DST_OK) { fprintf(stderr, "dst_rescue_multiproof_paths: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    if (memcmp(got, root, 32) || memcmp(expanded, paths, 32 * count * n)) { fprintf(stderr, "the expanded paths differ from dst_rtree_paths'\n"); return 1; }
    printf("the expanded paths equal dst_rtree_paths'\n");
    free(set_leaves); free(nodes); free(paths); free(expanded); free(indices);
    return 0;
}
