// The saved form of a Rescue Merkle tree (dst_rtree_save / dst_rtree_load, dst_stree_save / dst_stree_load, dst_wtree_save / dst_wtree_load;
// include/distaff_hip.h has the layout):
// the header, and the parser that takes UNTRUSTED bytes -- every length, count and prefix is checked here, before anything is allocated, and a
// sparse blob is admitted only with a shape that dst_stree_create + dst_stree_set could have made.  Free of HIP and of field arithmetic (an
// element is compared with p as two 64-bit halves), as is host/stree_levels.h, whose 128-bit comparisons it takes, so
// tests/sparse_host/tree_blob_check.cpp and tree_blob_wide_check.cpp compile it alone, with sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "stree_levels.h"

#define TBLOB_MAGIC "DSTTREE1"                           // 8 bytes; the last one is the version digit
#define TBLOB_HEADER 64u                                 // magic 8, kind 4, depth 4, empty leaf 32, keys 8, stored nodes 8
#define TBLOB_DENSE 1u
#define TBLOB_SPARSE 2u
#define TBLOB_WIDE 3u                                    // a sparse tree with 16-byte prefixes (dst_wtree_*), depth 1 .. 127
#define TBLOB_DENSE_MAX_DEPTH 26u
#define TBLOB_SPARSE_MAX_DEPTH 63u
#define TBLOB_WIDE_MAX_DEPTH 127u
#define TBLOB_MAX_NODES 0xFFFFFFFFull                    // a sparse tree stores fewer nodes than this (STREE_NEW: flat positions are 32 bits)

inline uint32_t tblob_u32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t tblob_u64(const uint8_t* p) { return (uint64_t)tblob_u32(p) | (uint64_t)tblob_u32(p + 4) << 32; }
inline void tblob_put_u32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
inline void tblob_put_u64(uint8_t* p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
// a stored prefix of `width` = 8 or 16 bytes, little-endian, as the two halves the comparisons of host/stree_levels.h take
inline stree_wide tblob_prefix(const uint8_t* p, size_t width) { return stree_wide{tblob_u64(p), width == 16 ? tblob_u64(p + 8) : 0}; }
// `elems` little-endian 128-bit values, all below p = 2^128 - 45 * 2^40 + 1 = 0xFFFFFFFF_FFFFFFFF_FFFFD300_00000001
inline bool tblob_below_p(const uint8_t* p, uint64_t elems) {
    for (uint64_t i = 0; i < elems; i++)
        if (tblob_u64(p + 16 * i + 8) == ~(uint64_t)0 && tblob_u64(p + 16 * i) >= 0xFFFFD30000000001ull) return false;
    return true;
}
inline void tblob_put_header(uint8_t* out, uint32_t kind, uint32_t depth, const uint8_t* empty /* 32 bytes, or nullptr: zero */, uint64_t keys, uint64_t nodes) {
    memcpy(out, TBLOB_MAGIC, 8);
    tblob_put_u32(out + 8, kind); tblob_put_u32(out + 12, depth);
    if (empty) memcpy(out + 16, empty, 32); else memset(out + 16, 0, 32);
    tblob_put_u64(out + 48, keys); tblob_put_u64(out + 56, nodes);
}
inline uint64_t tblob_dense_bytes(uint32_t log_leaves) { return TBLOB_HEADER + 32 * (((uint64_t)2 << log_leaves) - 1); }
inline uint64_t tblob_sparse_bytes(uint32_t depth, uint64_t nodes) { return TBLOB_HEADER + 8 * ((uint64_t)depth + 1) + 40 * nodes; }
inline uint64_t tblob_wide_bytes(uint32_t depth, uint64_t nodes) { return TBLOB_HEADER + 8 * ((uint64_t)depth + 1) + 48 * nodes; }

// what a checked blob holds: pointers into it (of any alignment)
struct tblob_view {
    uint32_t kind = 0, depth = 0;
    const uint8_t* empty = nullptr;                      // 32 bytes
    uint64_t keys = 0, nodes = 0;
    const uint8_t* counts = nullptr;                     // sparse: depth + 1 lengths, the leaf level first
    const uint8_t* prefixes = nullptr;                   // sparse: `nodes` prefixes of 8 bytes (wide: 16), level by level in that order
    const uint8_t* values = nullptr;                     // `nodes` nodes of 32 bytes
};

// nullptr when `blob` is a well-formed tree of `kind`, else what is wrong with it
inline const char* tblob_parse(const uint8_t* blob, size_t len, uint32_t kind, tblob_view& v) {
    if (!blob || len < TBLOB_HEADER) return "the blob is shorter than its header";
    if (memcmp(blob, TBLOB_MAGIC, 7) != 0) return "not a saved tree (wrong magic)";
    if (blob[7] != (uint8_t)TBLOB_MAGIC[7]) return "a saved tree of another version";
    v.kind = tblob_u32(blob + 8); v.depth = tblob_u32(blob + 12);
    v.empty = blob + 16;
    v.keys = tblob_u64(blob + 48); v.nodes = tblob_u64(blob + 56);
    if (v.kind != kind) {                                // per loader, what it says to each other kind; the loaders of kinds 1 and 2 do not know kind 3
        const bool known = v.kind == TBLOB_DENSE || v.kind == TBLOB_SPARSE;
        switch (kind) {
        case TBLOB_DENSE: return known ? "a sparse tree, not a dense one" : "unknown kind of tree";
        case TBLOB_SPARSE: return known ? "a dense tree, not a sparse one" : "unknown kind of tree";
        default: return v.kind == TBLOB_DENSE ? "a dense tree, not a wide sparse one" : v.kind == TBLOB_SPARSE ? "a sparse tree of 8-byte keys, not a wide one" : "unknown kind of tree";
        }
    }
    if (kind == TBLOB_DENSE) {
        if (v.depth < 1 || v.depth > TBLOB_DENSE_MAX_DEPTH) return "log_leaves outside 1 .. 26";
        for (int i = 0; i < 32; i++) if (v.empty[i]) return "a dense tree has no empty leaf";
        if (v.keys != (uint64_t)1 << v.depth || v.nodes != ((uint64_t)2 << v.depth) - 1) return "the counts disagree with log_leaves";
        if (len < tblob_dense_bytes(v.depth)) return "the blob is truncated";
        if (len > tblob_dense_bytes(v.depth)) return "bytes after the end of the tree";
        v.values = blob + TBLOB_HEADER;
        if (!tblob_below_p(v.values, 2 * v.nodes)) return "a node element is not below the modulus";
        return nullptr;
    }
    const uint32_t D = v.depth;
    const size_t W = kind == TBLOB_WIDE ? 16 : 8;        // bytes per prefix
    const uint64_t bytes = kind == TBLOB_WIDE ? tblob_wide_bytes(D, v.nodes) : tblob_sparse_bytes(D, v.nodes);
    if (kind == TBLOB_WIDE && (D < 1 || D > TBLOB_WIDE_MAX_DEPTH)) return "depth outside 1 .. 127";
    if (kind == TBLOB_SPARSE && (D < 1 || D > TBLOB_SPARSE_MAX_DEPTH)) return "depth outside 1 .. 63";
    if (!tblob_below_p(v.empty, 2)) return "an element of the empty leaf is not below the modulus";
    if (v.nodes >= TBLOB_MAX_NODES) return "more than 2^32 - 2 stored nodes";
    if (len < bytes) return "the blob is truncated";
    if (len > bytes) return "bytes after the end of the tree";
    v.counts = blob + TBLOB_HEADER;
    v.prefixes = v.counts + 8 * ((size_t)D + 1);
    v.values = v.prefixes + W * v.nodes;
    uint64_t sum = 0;
    for (uint32_t k = 0; k <= D; k++) {                  // run k is level D - k
        const uint64_t c = tblob_u64(v.counts + 8 * k);
        if (c > v.nodes - sum) return "the level counts disagree with the number of stored nodes";
        sum += c;
    }
    if (sum != v.nodes) return "the level counts disagree with the number of stored nodes";
    if (tblob_u64(v.counts) != v.keys) return "the key count disagrees with the leaf level";
    if (tblob_u64(v.counts + 8 * (size_t)D) > 1) return "more than one root";
    const uint8_t *child = nullptr, *run = v.prefixes;   // the level below, and this one
    uint64_t child_cnt = 0;
    for (uint32_t k = 0; k <= D; k++) {
        const uint32_t l = D - k;
        const uint64_t cnt = tblob_u64(v.counts + 8 * k);
        for (uint64_t i = 0; i < cnt; i++) {             // the whole prefix is compared: both halves of a wide one
            const stree_wide q = tblob_prefix(run + W * i, W);
            if (l < 8 * W && (q >> l) != stree_wide{0, 0}) return "a prefix is not below 2^level";
            if (i && tblob_prefix(run + W * (i - 1), W) == q) return "a prefix is stored twice on its level";
            if (i && tblob_prefix(run + W * (i - 1), W) > q) return "the prefixes of a level do not ascend";
        }
        if (k) {                                         // exactly the distinct prefix >> 1 of the level below, which ascends
            uint64_t at = 0;
            for (uint64_t i = 0; i < child_cnt; i++) {
                const stree_wide q = tblob_prefix(child + W * i, W) >> 1u;
                if (at && tblob_prefix(run + W * (at - 1), W) == q) continue;
                if (at == cnt) return "a level lacks the parent of a stored node";
                const stree_wide have = tblob_prefix(run + W * at, W);
                if (have < q) return "a level stores a node with nothing below it";
                if (have > q) return "a level lacks the parent of a stored node";
                at++;
            }
            if (at != cnt) return "a level stores a node with nothing below it";
        }
        child = run; child_cnt = cnt;
        run += W * cnt;
    }
    if (!tblob_below_p(v.values, 2 * v.nodes)) return "a node element is not below the modulus";
    return nullptr;
}
