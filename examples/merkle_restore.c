/* "a tree that survives a restart": a Rescue Merkle tree is built once, saved to a file with dst_rtree_save and destroyed; dst_rtree_load brings
 * it back WITHOUT hashing it again and, because the file is not trusted, with the audit -- one launch that checks every parent against its
 * children.  The restored tree has the same root and opens the same path.  Then one bit of one node is flipped in the file: the load with audit
 * refuses it and names the node, while dst_rtree_audit on the tree loaded without audit gives the position as a number.  C99, the header and
 * libdistaff_hip.so only.
 *
 *   cc -std=c99 -I include -o merkle_restore examples/merkle_restore.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./merkle_restore <log_leaves> <file> [device, default 0; -1 = on the host, no GPU]
 *
 * Leaf i is (2i + 1, 2i + 2); the path shown is that of the last leaf; the node changed in the file is heap position 3, so its parent,
 * node 1, is the first parent that no longer is the digest of its children. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

static void print_element(const uint8_t* e) { int i; for (i = 15; i >= 0; i--) printf("%02x", e[i]); }
static void print_node(const char* label, const uint8_t* node) { printf("%s ", label); print_element(node); printf(" "); print_element(node + 16); printf("\n"); }

static int write_file(const char* name, const uint8_t* p, size_t len) {
    FILE* f = fopen(name, "wb");
    size_t done = f ? fwrite(p, 1, len, f) : 0;
    return f && fclose(f) == 0 && done == len ? 0 : -1;
}
static int read_file(const char* name, uint8_t* p, size_t len) {
    FILE* f = fopen(name, "rb");
    size_t done = f ? fread(p, 1, len, f) : 0;
    if (f) fclose(f);
    return done == len ? 0 : -1;
}

int main(int argc, char** argv) {
    unsigned long long i, n;
    unsigned log_leaves;
    int device, rc, b, status = 1;
    uint8_t *leaves = NULL, *blob = NULL, root[32], root_again[32], path[27 * 32], path_again[27 * 32];
    size_t len = 0, path_bytes;
    int64_t first_bad = 0;
    dst_rtree* tree = NULL;
    if (argc < 3) { fprintf(stderr, "usage: %s <log_leaves> <file> [device | -1 for the host]\n", argv[0]); return 2; }
    log_leaves = (unsigned)atoi(argv[1]);
    device = argc > 3 ? atoi(argv[3]) : 0;
    if (log_leaves < 2 || log_leaves > 24) { fprintf(stderr, "2 <= log_leaves <= 24\n"); return 2; }
    n = 1ull << log_leaves;
    path_bytes = (size_t)(log_leaves + 1) * 32;
    leaves = (uint8_t*)calloc((size_t)n, 32);
    if (!leaves) { fprintf(stderr, "out of memory\n"); goto done; }
    for (i = 0; i < n; i++) {                                   /* leaf i = (2i + 1, 2i + 2), little-endian */
        unsigned long long v0 = 2 * i + 1, v1 = 2 * i + 2;
        for (b = 0; b < 8; b++) { leaves[32 * i + b] = (uint8_t)(v0 >> (8 * b)); leaves[32 * i + 16 + b] = (uint8_t)(v1 >> (8 * b)); }
    }
    rc = dst_rtree_build(device, leaves, log_leaves, &tree);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_build: %d %s\n", rc, dst_rtree_last_error(NULL)); goto done; }
    rc = dst_rtree_root(tree, root);
    if (rc == DST_OK) rc = dst_rtree_path(tree, n - 1, path);
    if (rc == DST_OK) rc = dst_rtree_save(tree, NULL, 0, &len);                                     /* the size query */
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree: %d %s\n", rc, dst_rtree_last_error(tree)); goto done; }
    blob = (uint8_t*)malloc(len);
    if (!blob) { fprintf(stderr, "out of memory\n"); goto done; }
    rc = dst_rtree_save(tree, blob, len, &len);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_save: %d %s\n", rc, dst_rtree_last_error(tree)); goto done; }
    dst_rtree_destroy(tree);                                                                        /* the "restart" */
    tree = NULL;
    if (write_file(argv[2], blob, len) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); goto done; }
    print_node("root", root);
    printf("saved %llu nodes in %llu bytes\n", 2 * n - 1, (unsigned long long)len);

    memset(blob, 0, len);
    if (read_file(argv[2], blob, len) != 0) { fprintf(stderr, "cannot read %s\n", argv[2]); goto done; }
    rc = dst_rtree_load(device, blob, len, 1, &tree);                                               /* nothing is built; every parent is checked */
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_load: %d %s\n", rc, dst_rtree_last_error(NULL)); goto done; }
    rc = dst_rtree_root(tree, root_again);
    if (rc == DST_OK) rc = dst_rtree_path(tree, n - 1, path_again);
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree: %d %s\n", rc, dst_rtree_last_error(tree)); goto done; }
    print_node("root after the restart", root_again);
    printf("the same root: %s, the same path of leaf %llu: %s\n", memcmp(root, root_again, 32) == 0 ? "yes" : "no", n - 1,
           memcmp(path, path_again, path_bytes) == 0 ? "yes" : "no");
    dst_rtree_destroy(tree);
    tree = NULL;

    blob[64 + 2 * 32] ^= 1;                                                                         /* one bit of node 3, in the file */
    if (write_file(argv[2], blob, len) != 0 || read_file(argv[2], blob, len) != 0) { fprintf(stderr, "cannot rewrite %s\n", argv[2]); goto done; }
    rc = dst_rtree_load(device, blob, len, 1, &tree);
    printf("load of the changed file with audit: %s, tree %s: %s\n", rc == DST_ERR_ARG ? "DST_ERR_ARG" : rc == DST_OK ? "DST_OK" : "another error",
           tree ? "handed out" : "NULL", dst_rtree_last_error(NULL));
    if (tree) goto done;
    rc = dst_rtree_load(device, blob, len, 0, &tree);                                               /* believed as it is ... */
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_load: %d %s\n", rc, dst_rtree_last_error(NULL)); goto done; }
    rc = dst_rtree_audit(tree, &first_bad, NULL);                                                   /* ... and then found out */
    if (rc != DST_OK) { fprintf(stderr, "dst_rtree_audit: %d %s\n", rc, dst_rtree_last_error(tree)); goto done; }
    printf("loaded without audit, then audited: first bad node %lld\n", (long long)first_bad);
    status = 0;
done:                                                                                               /* every way out frees what it holds */
    dst_rtree_destroy(tree);
    free(leaves);
    free(blob);
    return status;
}
