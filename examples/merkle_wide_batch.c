/* "one proof for a batch of hash-derived keys, and a tree that survives a restart": a wide-key sparse Rescue Merkle tree (dst_wtree_*, depth 127)
 * with the keys of examples/merkle_wide.c -- key i is the first element of dst_rescue_digest_many over (i, 1, 2, 3) masked to 127 bits, its leaf
 * (2i + 1, 2i + 2).  ONE dst_wtree_set inserts k keys.  Three members and three keys that were never inserted are opened by ONE
 * dst_wtree_multiproof in the COMPACT form: the siblings that are empty subtrees are a bit each, not 32 bytes.  A client that holds the root and
 * the table of empty subtrees it computed itself (dst_rescue_empty_nodes) checks all six -- membership and absence -- with
 * dst_rescue_verify_multiproof_w, which hashes no parent of two empty subtrees.  The tree is then saved to a file (dst_wtree_save), loaded from
 * it with the audit (dst_wtree_load), and the loaded tree gives the same proof.  C99, the header and libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_wide_batch examples/merkle_wide_batch.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_wide_batch <k> <file> [device, default 0; -1 = on the host, no GPU] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

#define DEPTH 127u
#define NODES (DEPTH + 1u)
#define ASKED 6u

static void print_element(const uint8_t* e) { int i; for (i = 15; i >= 0; i--) printf("%02x", e[i]); }
static void put_u64(uint8_t* at, unsigned long long v) { int b; for (b = 0; b < 8; b++) at[b] = (uint8_t)(v >> (8 * b)); }

/* the compact proof of the ASKED keys: leaves (ASKED * 32), *nodes (allocated here), bits (*bits, allocated here) */
static int take_proof(const dst_wtree* tree, const uint8_t* ask, uint8_t* leaves, uint8_t** nodes, uint8_t** bits, size_t* shipped, size_t* supplied) {
    uint8_t probe = 0;
    int rc = dst_wtree_multiproof(tree, ask, ASKED, NULL, NULL, 0, shipped, &probe, supplied);      /* size query of the compact form */
    if (rc != DST_OK) return rc;
    *nodes = (uint8_t*)malloc(32 * (*shipped + 1));
    *bits = (uint8_t*)malloc((*supplied + 7) / 8 + 1);
    if (!*nodes || !*bits) return DST_ERR_HIP;
    return dst_wtree_multiproof(tree, ask, ASKED, leaves, *nodes, *shipped, shipped, *bits, supplied);
}

int main(int argc, char** argv) {
    unsigned long long i, k;
    uint64_t digests = 0, plain_digests = 0;
    int device, rc, ok = 0;
    uint8_t *in, *hashed, *keys, *leaves, *nodes = NULL, *bits = NULL, *nodes2 = NULL, *bits2 = NULL, *blob, *back;
    uint8_t ask[ASKED * 16], got[ASKED * 32], got2[ASKED * 32], empties[NODES * 32], root[32], root2[32], own[32];
    size_t shipped = 0, supplied = 0, shipped2 = 0, supplied2 = 0, plain_nodes = 0, len = 0;
    dst_wtree *tree = NULL, *loaded = NULL;
    dst_stree_info_t info;
    FILE* f;
    if (argc < 3) { fprintf(stderr, "usage: %s <k> <file> [device | -1 for the host]\n", argv[0]); return 2; }
    k = strtoull(argv[1], NULL, 10);
    device = argc > 3 ? atoi(argv[3]) : 0;
    if (k < 3 || k > (1ull << 20)) { fprintf(stderr, "3 <= k <= 2^20\n"); return 2; }
    in = (uint8_t*)calloc((size_t)(k + 3), 64);
    hashed = (uint8_t*)malloc((size_t)(k + 3) * 32);
    keys = (uint8_t*)malloc((size_t)(k + 3) * 16);
    leaves = (uint8_t*)calloc((size_t)k, 32);
    if (!in || !hashed || !keys || !leaves) { fprintf(stderr, "out of memory\n"); return 2; }
    for (i = 0; i < k + 3; i++) { put_u64(in + 64 * i, i); in[64 * i + 16] = 1; in[64 * i + 32] = 2; in[64 * i + 48] = 3; }
    rc = dst_rescue_digest_many(device, in, (size_t)(k + 3), hashed);
    if (rc != DST_OK) { fprintf(stderr, "dst_rescue_digest_many: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    for (i = 0; i < k + 3; i++) { memcpy(keys + 16 * i, hashed + 32 * i, 16); keys[16 * i + 15] &= 0x7f; }    /* one element, masked to 127 bits */
    for (i = 0; i < k; i++) { put_u64(leaves + 32 * i, 2 * i + 1); put_u64(leaves + 32 * i + 16, 2 * i + 2); }
    rc = dst_wtree_create(device, DEPTH, NULL, &tree);
    if (rc != DST_OK) { fprintf(stderr, "dst_wtree_create: %d %s\n", rc, dst_wtree_last_error(NULL)); return 1; }
    /* three members -- the first, the middle, the last -- and the three keys behind them, which are not inserted */
    memcpy(ask, keys, 16); memcpy(ask + 16, keys + 16 * (k / 2), 16); memcpy(ask + 32, keys + 16 * (k - 1), 16); memcpy(ask + 48, keys + 16 * k, 48);
    rc = dst_wtree_set(tree, keys, leaves, (size_t)k);
    if (rc == DST_OK) rc = dst_wtree_root(tree, root);
    if (rc == DST_OK) rc = dst_wtree_info(tree, &info);
    if (rc == DST_OK) rc = take_proof(tree, ask, got, &nodes, &bits, &shipped, &supplied);
    if (rc == DST_OK) rc = dst_wtree_save(tree, NULL, 0, &len);
    if (rc != DST_OK) { fprintf(stderr, "dst_wtree: %d %s\n", rc, dst_wtree_last_error(tree)); dst_wtree_destroy(tree); return 1; }
    blob = (uint8_t*)malloc(len);
    back = (uint8_t*)malloc(len);
    if (!blob || !back) { fprintf(stderr, "out of memory\n"); dst_wtree_destroy(tree); return 2; }
    rc = dst_wtree_save(tree, blob, len, &len);
    if (rc != DST_OK) { fprintf(stderr, "dst_wtree_save: %d %s\n", rc, dst_wtree_last_error(tree)); dst_wtree_destroy(tree); return 1; }
    dst_wtree_destroy(tree);
    /* a client that holds the root alone: the table of empty subtrees is its own; members show their leaves, the others the empty leaf (0, 0) */
    rc = dst_rescue_empty_nodes(NULL, NODES, empties);
    if (rc == DST_OK) rc = dst_rescue_multiproof_size_w(NODES, ask, ASKED, &plain_nodes, &plain_digests);
    if (rc == DST_OK) rc = dst_rescue_verify_multiproof_w(device, root, NODES, ask, got, ASKED, nodes, shipped, bits, empties, &ok, NULL);
    if (rc == DST_OK) rc = dst_rescue_multiproof_root_w(device, NODES, ask, got, ASKED, nodes, shipped, bits, empties, own, &digests, NULL);
    if (rc != DST_OK) { fprintf(stderr, "dst_rescue_multiproof: %d %s\n", rc, dst_rtree_last_error(NULL)); return 1; }
    if (!ok || memcmp(own, root, 32) != 0) { fprintf(stderr, "the proof does not resolve to the root\n"); return 1; }
    if (memcmp(got, leaves, 32) != 0 || memcmp(got + 64, leaves + 32 * (k - 1), 32) != 0 || memcmp(got + 96, empties + 32 * DEPTH, 32) != 0) { fprintf(stderr, "a leaf is not what was set\n"); return 1; }
    got[0] ^= 1;                                                                                              /* another leaf for the first member */
    rc = dst_rescue_verify_multiproof_w(device, root, NODES, ask, got, ASKED, nodes, shipped, bits, empties, &ok, NULL);
    if (rc != DST_OK || ok) { fprintf(stderr, "a changed leaf verified\n"); return 1; }
    got[0] ^= 1;
    /* the restart: the bytes go to a file and come back; load checks their shape and, asked to, every stored parent */
    f = fopen(argv[2], "wb");
    if (!f || fwrite(blob, 1, len, f) != len || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    f = fopen(argv[2], "rb");
    if (!f || fread(back, 1, len, f) != len) { fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
    fclose(f);
    rc = dst_wtree_load(device, back, len, 1, &loaded);
    if (rc != DST_OK) { fprintf(stderr, "dst_wtree_load: %d %s\n", rc, dst_wtree_last_error(NULL)); return 1; }
    rc = dst_wtree_root(loaded, root2);
    if (rc == DST_OK) rc = take_proof(loaded, ask, got2, &nodes2, &bits2, &shipped2, &supplied2);
    if (rc != DST_OK) { fprintf(stderr, "dst_wtree: %d %s\n", rc, dst_wtree_last_error(loaded)); dst_wtree_destroy(loaded); return 1; }
    dst_wtree_destroy(loaded);
    if (memcmp(root, root2, 32) != 0 || shipped2 != shipped || supplied2 != supplied || memcmp(got, got2, sizeof got) != 0 || memcmp(nodes, nodes2, 32 * shipped) != 0 ||
        memcmp(bits, bits2, (supplied + 7) / 8) != 0) { fprintf(stderr, "the loaded tree gives another proof\n"); return 1; }
    printf("root "); print_element(root); printf(" "); print_element(root + 16); printf("\n");
    printf("%llu keys of 127 bits in %llu stored nodes\n", (unsigned long long)info.keys, (unsigned long long)info.nodes);
    printf("%u keys asked, 3 members and 3 absent: %lu supplied nodes, %lu of them stored; the compact proof has %lu bytes, the plain one %lu, six paths %lu\n", ASKED, (unsigned long)supplied,
           (unsigned long)shipped, (unsigned long)(32 * ASKED + 32 * shipped + (supplied + 7) / 8), (unsigned long)(32 * ASKED + 32 * plain_nodes), (unsigned long)(32 * ASKED * NODES));
    printf("verified against the root alone with %llu digests; the plain proof takes %llu, six paths %u; a changed leaf is rejected\n", (unsigned long long)digests, (unsigned long long)plain_digests, ASKED * DEPTH);
    printf("saved %lu bytes, loaded with audit: root ", (unsigned long)len); print_element(root2); printf(" "); print_element(root2 + 16); printf(", the same proof\n");
    free(in); free(hashed); free(keys); free(leaves); free(nodes); free(bits); free(nodes2); free(bits2); free(blob); free(back);
    return 0;
}
