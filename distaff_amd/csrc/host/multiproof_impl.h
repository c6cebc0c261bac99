// dst_rescue_multiproof_size, dst_rtree_multiproof / dst_stree_multiproof and the tree-less dst_rescue_multiproof_root / dst_rescue_verify_multiproof /
// dst_rescue_multiproof_paths: the plan of host/multiproof_plan.h run where the caller says.  Included by api.hip alone, after stree_impl.h and
// path_verify_impl.h, whose conventions these calls keep: the tree-less ones file errors with dst_rtree_last_error(NULL), device < 0 is the host
// with one thread and no HIP call, and everything but an element that is not below p is refused before anything is queued.  The _w forms
// (16-byte indices, n <= 128) and dst_wtree_multiproof run the same plan over stree_wide positions, with the compact form's known-empty nodes.
#pragma once
#include "multiproof_plan.h"
#include "path_verify_impl.h"
#include "stree_impl.h"

static_assert(MP_MAX_DEPTH + 1 == PV_MAX_NODES && MP_MAX_DEPTH == STREE_MAX_DEPTH, "a multiproof covers the paths of 2 .. 64 nodes");
static const char* const MP_NOT_BELOW_P = "an element of the leaves or nodes is not below the modulus";

int dst_rescue_multiproof_size(uint32_t n, const uint64_t* indices, size_t count, size_t* num_nodes, uint64_t* digests) {
    if (!num_nodes || !digests || (!indices && count)) return pv_fail(DST_ERR_ARG, "null pointer");
    *num_nodes = 0; *digests = 0;
    if (const char* why = pv_check_shape(n, indices, count)) return pv_fail(DST_ERR_ARG, why);
    if (count == 0) return DST_OK;
    try {
        mp_plan p;
        if (const char* why = mp_plan_make(n - 1, indices, count, 0, p)) return pv_fail(DST_ERR_ARG, why);
        *num_nodes = (size_t)p.sizes.nodes; *digests = p.sizes.digests;
    } catch (const std::bad_alloc&) { return pv_fail(DST_ERR_HIP, "out of host memory"); }
    return DST_OK;
}

// ---- the tree side: the leaves of the set and the supplied nodes, gathered out of a tree ---------------------------------------------------------
// what the two calls share before they read a node: DST_OK with *num_nodes = M and p.slevel / p.spos in the order of `nodes`; *gather = whether the
// caller asked for more than the size
template <class T, class Fail>
static int mp_tree_enter(const T* t, uint32_t depth, const uint64_t* indices, size_t count, const uint8_t* leaves, const uint8_t* nodes, size_t cap_nodes, size_t* num_nodes, mp_plan& p,
                         bool* gather, Fail fail) {
    *gather = false;
    if (!num_nodes || (!indices && count)) return fail(t, DST_ERR_ARG, "null pointer");
    *num_nodes = 0;
    if (count == 0) return DST_OK;
    if (const char* why = pv_check_shape(depth + 1, indices, count)) return fail(t, DST_ERR_ARG, why);
    if (const char* why = mp_plan_make(depth, indices, count, MP_SUPPLIED, p)) return fail(t, DST_ERR_ARG, why);
    *num_nodes = (size_t)p.sizes.nodes;
    if (!nodes) return DST_OK;                                             // size query
    if (!leaves) return fail(t, DST_ERR_ARG, "null pointer");
    if (cap_nodes < p.sizes.nodes) return fail(t, DST_ERR_ARG, "node buffer too small");
    *gather = true;
    return DST_OK;
}
// on a device tree: one upload of the positions, one gather launch, one copy back -- [count leaves][M nodes] -- whatever count is
int dst_rtree_multiproof(const dst_rtree* t, const uint64_t* indices, size_t count, uint8_t* leaves, uint8_t* nodes, size_t cap_nodes, size_t* num_nodes) {
    if (int r = rt_enter(t)) return r;
    try {
        mp_plan p;
        bool gather;
        if (int r = mp_tree_enter(t, t->log_leaves, indices, count, leaves, nodes, cap_nodes, num_nodes, p, &gather, rt_fail)) return r;
        if (!gather) return DST_OK;
        const size_t M = p.inputs() - count, m = p.inputs();
        std::vector<uint32_t> where(m);                                    // node-array positions: (l, q) sits at 2^l + q
        for (size_t i = 0; i < count; i++) where[i] = (uint32_t)(((uint64_t)1 << t->log_leaves) + indices[i]);
        for (size_t j = 0; j < M; j++) where[count + j] = (uint32_t)(((uint64_t)1 << p.slevel[j]) + p.spos[j]);
        if (t->device < 0) {
            for (size_t s = 0; s < m; s++) memcpy(s < count ? leaves + 32 * s : nodes + 32 * (s - count), t->host.data() + 2 * (size_t)where[s], 32);
            return DST_OK;
        }
        std::vector<uint8_t> back(32 * m);
        if (int r = rtree_stage(t, 36 * m)) return r;                      // [m nodes][m positions]
        uint32_t* d_where = reinterpret_cast<uint32_t*>(t->stage + 32 * m);
        RT_HIP(t->err, hipMemcpyAsync(d_where, where.data(), 4 * m, hipMemcpyHostToDevice, t->stream));
        if (k_rescue_tree_gather(t->stream, t->dev, d_where, reinterpret_cast<fe*>(t->stage), m)) return rt_fail(t, DST_ERR_HIP, "rescue_tree_gather_kernel: launch failed");
        RT_HIP(t->err, hipMemcpyAsync(back.data(), t->stage, 32 * m, hipMemcpyDeviceToHost, t->stream));
        RT_HIP(t->err, hipStreamSynchronize(t->stream));
        memcpy(leaves, back.data(), 32 * count);
        if (M) memcpy(nodes, back.data() + 32 * count, 32 * M);
    } catch (const std::bad_alloc&) { return rt_fail(t, DST_ERR_HIP, "out of host memory"); }
    return DST_OK;
}
// the same on a sparse tree: a leaf or a sibling that is not stored is the E_l of its level, so absent keys are proven by the same call.  On a
// device tree one upload of the (prefix, level) pairs, one lookup launch, one copy back
int dst_stree_multiproof(const dst_stree* t, const uint64_t* indices, size_t count, uint8_t* leaves, uint8_t* nodes, size_t cap_nodes, size_t* num_nodes) {
    if (int r = st_enter(t)) return r;
    try {
        mp_plan p;
        bool gather;
        if (int r = mp_tree_enter(t, t->depth, indices, count, leaves, nodes, cap_nodes, num_nodes, p, &gather, st_fail)) return r;
        if (!gather) return DST_OK;
        const size_t M = p.inputs() - count, m = p.inputs();
        if (t->device < 0) {
            for (size_t s = 0; s < m; s++) {
                const uint32_t level = s < count ? t->depth : p.slevel[s - count];
                const uint64_t prefix = s < count ? indices[s] : p.spos[s - count];
                const size_t start = t->shape.start[level], pos = stree_find(t->shape.pref.data() + start, t->shape.cnt[level], prefix);
                memcpy(s < count ? leaves + 32 * s : nodes + 32 * (s - count), pos != STREE_ABSENT ? &t->host[2 * (start + pos)] : t->empties + 2 * level, 32);
            }
            return DST_OK;
        }
        std::vector<uint8_t> up(12 * m), back(32 * m);                     // [m prefixes][m levels]
        memcpy(up.data(), indices, 8 * count);
        if (M) memcpy(up.data() + 8 * count, p.spos.data(), 8 * M);
        for (size_t s = 0; s < m; s++) { const uint32_t level = s < count ? t->depth : p.slevel[s - count]; memcpy(up.data() + 8 * m + 4 * s, &level, 4); }
        if (int r = rtree_stage(t, 44 * m)) return r;                      // [m nodes][m prefixes][m levels]
        const uint64_t* d_prefix = reinterpret_cast<const uint64_t*>(t->stage + 32 * m);
        RT_HIP(t->err, hipMemcpyAsync(t->stage + 32 * m, up.data(), 12 * m, hipMemcpyHostToDevice, t->stream));
        if (k_rescue_stree_lookup(t->stream, t->dev_nodes(), t->dev_pref(), t->dev_levels(), t->dev_empties(), d_prefix, reinterpret_cast<const uint32_t*>(d_prefix + m),
                                  reinterpret_cast<fe*>(t->stage), m))
            return st_fail(t, DST_ERR_HIP, "rescue_stree_lookup_kernel: launch failed");
        RT_HIP(t->err, hipMemcpyAsync(back.data(), t->stage, 32 * m, hipMemcpyDeviceToHost, t->stream));
        RT_HIP(t->err, hipStreamSynchronize(t->stream));
        memcpy(leaves, back.data(), 32 * count);
        if (M) memcpy(nodes, back.data() + 32 * count, 32 * M);
    } catch (const std::bad_alloc&) { return st_fail(t, DST_ERR_HIP, "out of host memory"); }
    return DST_OK;
}

// ---- the wide tree side: plain (every supplied node) or compact (the stored ones and a bit for each that is not) ----------------------------------
// 16-byte little-endian indices at any alignment, copied into u128; the plan reads the same bytes as stree_wide
struct mp_wide_indices {
    std::vector<u128> v;
    const stree_wide* wide() const { return reinterpret_cast<const stree_wide*>(v.data()); }
};
// Every asked node -- the count leaves, then the M supplied nodes in plan order -- is located in its level's list: flat position or STREE_NEW.  A
// device tree does that in one launch over all m = count + M nodes and leaves the positions on the device; a second launch packs the stored ones,
// which alone come back.  What is not stored never crosses the bus: the host has every E_l.  A tree without nodes launches nothing.
int dst_wtree_multiproof(const dst_wtree* t, const uint8_t* keys, size_t count, uint8_t* leaves, uint8_t* nodes, size_t cap_nodes, size_t* num_nodes, uint8_t* absent_bits, size_t* total) {
    if (int r = st_enter(t)) return r;
    if (!num_nodes || (!keys && count)) return st_fail(t, DST_ERR_ARG, "null pointer");
    *num_nodes = 0;
    if (total) *total = 0;
    if (count == 0) return DST_OK;
    if ((uint64_t)count >= ((uint64_t)1 << 31)) return st_fail(t, DST_ERR_ARG, "2^31 paths or more");
    try {
        mp_wide_indices k;
        k.v.resize(count);
        memcpy(k.v.data(), keys, 16 * count);
        if (const char* why = pv_check_shape_of<u128>(t->depth + 1, k.v.data(), count)) return st_fail(t, DST_ERR_ARG, why);
        mp_plan_t<stree_wide> p;
        if (const char* why = mp_plan_make(t->depth, k.wide(), count, MP_SUPPLIED, p)) return st_fail(t, DST_ERR_ARG, why);
        const size_t M = (size_t)p.sizes.nodes, m = count + M, D = t->depth;
        if (!absent_bits) {                                                // the plain form: its size needs no look at the tree
            if (!nodes) { *num_nodes = M; if (total) *total = M; return DST_OK; }
            if (!leaves) return st_fail(t, DST_ERR_ARG, "null pointer");
            if (cap_nodes < M) return st_fail(t, DST_ERR_ARG, "node buffer too small");
        } else if (nodes && !leaves) return st_fail(t, DST_ERR_ARG, "null pointer");
        std::vector<uint32_t> flat(m, STREE_NEW), level(m, (uint32_t)D);
        for (size_t j = 0; j < M; j++) level[count + j] = p.slevel[j];
        auto prefix = [&](size_t s) { u128 q = 0; if (s < count) q = k.v[s]; else memcpy(&q, &p.spos[s - count], 16); return q; };
        const bool launch = t->device >= 0 && t->shape.total() != 0;
        const size_t blocks = (m + RESCUE_LOCATE_BLOCK - 1) / RESCUE_LOCATE_BLOCK;
        const size_t o_prefix = 32 * m, o_level = o_prefix + 16 * m, o_flat = o_level + 4 * m, o_rank = o_flat + 4 * m, o_totals = o_rank + 4 * m;      // [packed nodes][prefixes][levels][flat][rank][totals]
        if (launch) {
            std::vector<uint8_t> up(20 * m);
            memcpy(up.data(), keys, 16 * count);
            if (M) memcpy(up.data() + 16 * count, p.spos.data(), 16 * M);
            memcpy(up.data() + 16 * m, level.data(), 4 * m);
            if (int r = rtree_stage(t, o_totals + 4 * blocks)) return r;
            RT_HIP(t->err, hipMemcpyAsync(t->stage + o_prefix, up.data(), 20 * m, hipMemcpyHostToDevice, t->stream));
            if (k_rescue_stree_locate(t->stream, t->dev_pref(), t->dev_levels(), reinterpret_cast<const stree_wide*>(t->stage + o_prefix), reinterpret_cast<const uint32_t*>(t->stage + o_level),
                                      reinterpret_cast<uint32_t*>(t->stage + o_flat), reinterpret_cast<uint32_t*>(t->stage + o_rank), reinterpret_cast<uint32_t*>(t->stage + o_totals), m))
                return st_fail(t, DST_ERR_HIP, "rescue_stree_locate_kernel: launch failed");
            RT_HIP(t->err, hipMemcpyAsync(flat.data(), t->stage + o_flat, 4 * m, hipMemcpyDeviceToHost, t->stream));
            RT_HIP(t->err, hipStreamSynchronize(t->stream));
        } else if (t->device < 0) {
            for (size_t s = 0; s < m; s++) {
                const size_t start = t->shape.start[level[s]], pos = stree_find(t->shape.pref.data() + start, t->shape.cnt[level[s]], prefix(s));
                if (pos != STREE_ABSENT) flat[s] = (uint32_t)(start + pos);
            }
        }
        size_t stored = 0, S = 0;                                          // among all m nodes, among the supplied ones
        for (size_t s = 0; s < m; s++) { if (flat[s] != STREE_NEW) { stored++; if (s >= count) S++; } }
        if (total) *total = M;
        if (absent_bits) {
            *num_nodes = S;
            if (!nodes) return DST_OK;                                     // size query
            if (cap_nodes < S) { *num_nodes = 0; if (total) *total = 0; return st_fail(t, DST_ERR_ARG, "node buffer too small"); }
        } else *num_nodes = M;
        std::vector<uint8_t> back;
        const uint8_t* from = nullptr;                                     // the stored nodes, packed in the order of s
        if (launch && stored) {
            back.resize(32 * stored);
            if (k_rescue_stree_pack(t->stream, t->dev_nodes(), reinterpret_cast<const uint32_t*>(t->stage + o_flat), reinterpret_cast<const uint32_t*>(t->stage + o_rank),
                                    reinterpret_cast<const uint32_t*>(t->stage + o_totals), reinterpret_cast<fe*>(t->stage), m))
                return st_fail(t, DST_ERR_HIP, "rescue_stree_pack_kernel: launch failed");
            RT_HIP(t->err, hipMemcpyAsync(back.data(), t->stage, 32 * stored, hipMemcpyDeviceToHost, t->stream));
            RT_HIP(t->err, hipStreamSynchronize(t->stream));
            from = back.data();
        }
        if (absent_bits) memset(absent_bits, 0, (M + 7) / 8);
        uint8_t* to = nodes;
        for (size_t s = 0; s < m; s++) {
            const bool has = flat[s] != STREE_NEW;
            const uint8_t* value = !has ? reinterpret_cast<const uint8_t*>(t->empties + 2 * (size_t)level[s]) : from ? from : reinterpret_cast<const uint8_t*>(&t->host[2 * (size_t)flat[s]]);
            if (has && from) from += 32;
            if (s < count) { memcpy(leaves + 32 * s, value, 32); continue; }
            if (!has && absent_bits) { absent_bits[(s - count) >> 3] |= (uint8_t)(1u << ((s - count) & 7)); continue; }
            memcpy(to, value, 32); to += 32;
        }
    } catch (const std::bad_alloc&) { return st_fail(t, DST_ERR_HIP, "out of host memory"); }
    return DST_OK;
}

// ---- without a tree: every ancestor the paths share is hashed once ------------------------------------------------------------------------------
static thread_local uint32_t g_mp_levels = 0;                             // dst_rescue_multiproof_last_levels
// the pool on the host: [leaves | nodes | the table of the compact form] are in place and below p; one rescue_digest_many_host call per level that
// has a job, over all of its jobs, whose results are consecutive pool nodes
template <class P>
static void mp_hash_host(const mp_plan_t<P>& p, std::vector<u128>& pool) {
    size_t most = 0;
    for (uint32_t l = 0; l < p.depth; l++) most = std::max(most, p.jcnt[l]);
    std::vector<u128> in(4 * most);
    for (uint32_t l = p.depth; l-- > 0;) {
        if (p.jcnt[l] == 0) continue;
        const uint32_t* jobs = p.jobs.data() + 3 * p.joff[l];
        for (size_t g = 0; g < p.jcnt[l]; g++) {
            memcpy(&in[4 * g], &pool[2 * (size_t)jobs[3 * g]], 32);
            memcpy(&in[4 * g + 2], &pool[2 * (size_t)jobs[3 * g + 1]], 32);
        }
        rescue_digest_many_host(in.data(), p.jcnt[l], &pool[2 * (size_t)jobs[2]]);
    }
}
// ... and on a device.  p = [job lists][path node indices][leaves][nodes][table] -- one upload; the pool begins at the leaves and goes on behind
// the upload -- then [paths][bad]; one level launch per level that has a job and, for the expansion, one gather launch between two events; one
// synchronisation; one copy back, from the root -- the last node of the pool: the caller has dealt with a plan without jobs -- to `bad`.
// back = [root][paths]
template <class P>
static int mp_hash_device(int device, const mp_plan_t<P>& p, const uint8_t* leaves, const uint8_t* nodes, const uint8_t* empties, bool expand, std::vector<uint8_t>& back, double* ms) {
    const size_t count = p.count, S = p.shipped, W = expand ? p.where.size() : 0;
    const size_t o_where = 4 * p.jobs.size(), o_pool = (o_where + 4 * W + 15) & ~(size_t)15, up_bytes = o_pool + 32 * p.inputs();
    const size_t o_root = o_pool + 32 * (p.pool() - 1), o_paths = o_root + 32, o_bad = o_paths + 32 * W, total = o_bad + 4;
    std::vector<uint8_t> up(up_bytes);                                     // the last host allocations: nothing is queued yet
    back.resize(total - o_root);
    memcpy(up.data(), p.jobs.data(), o_where);
    if (W) memcpy(up.data() + o_where, p.where.data(), 4 * W);
    memcpy(up.data() + o_pool, leaves, 32 * count);
    if (S) memcpy(up.data() + o_pool + 32 * count, nodes, 32 * S);
    if (p.table) memcpy(up.data() + o_pool + 32 * (count + S), empties, 32 * p.table);
    rt_scratch h;
    RT_HIP(g_rtree_error, hipSetDevice(device));
    RT_HIP(g_rtree_error, hipStreamCreateWithFlags(&h.s, hipStreamNonBlocking));
    RT_HIP(g_rtree_error, hipEventCreate(&h.ev[0]));
    RT_HIP(g_rtree_error, hipEventCreate(&h.ev[1]));
    RT_HIP(g_rtree_error, hipMalloc((void**)&h.p, total));
    fe* const pool = reinterpret_cast<fe*>(h.p + o_pool);
    const uint32_t* d_jobs = reinterpret_cast<const uint32_t*>(h.p);
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(h.p + o_bad);
    RT_HIP(g_rtree_error, hipMemsetAsync(d_bad, 0, 4, h.s));
    RT_HIP(g_rtree_error, hipMemcpyAsync(h.p, up.data(), up_bytes, hipMemcpyHostToDevice, h.s));
    RT_HIP(g_rtree_error, hipEventRecord(h.ev[0], h.s));
    for (uint32_t l = p.depth; l-- > 0;)
        if (p.jcnt[l] && k_rescue_multiproof_level(h.s, pool, d_jobs + 3 * p.joff[l], p.jcnt[l], (uint32_t)p.inputs(), d_bad)) return pv_fail(DST_ERR_HIP, "rescue_multiproof_level_kernel: launch failed");
    if (W && k_rescue_tree_gather(h.s, pool, reinterpret_cast<const uint32_t*>(h.p + o_where), reinterpret_cast<fe*>(h.p + o_paths), W))
        return pv_fail(DST_ERR_HIP, "rescue_tree_gather_kernel: launch failed");
    RT_HIP(g_rtree_error, hipEventRecord(h.ev[1], h.s));
    RT_HIP(g_rtree_error, hipMemcpyAsync(back.data(), h.p + o_root, total - o_root, hipMemcpyDeviceToHost, h.s));
    RT_HIP(g_rtree_error, hipStreamSynchronize(h.s));
    float f = 0;
    RT_HIP(g_rtree_error, hipEventElapsedTime(&f, h.ev[0], h.ev[1]));
    *ms = f;
    uint32_t bad = 0;
    memcpy(&bad, back.data() + (o_bad - o_root), 4);
    if (bad) return pv_fail(DST_ERR_ARG, MP_NOT_BELOW_P);
    back.resize(o_bad - o_root);
    return DST_OK;
}
// what the calls share: the argument checks, the plan, the hashing.  K = the indices as the shape check reads them (uint64_t, u128), P = the same
// bytes as the plan reads them (uint64_t, stree_wide).  root, paths (may be nullptr: no expansion), digests and ms (may be nullptr) are written
// only when everything holds.  absent_bits / empties: the compact form of the _w calls, nullptr otherwise
template <class K, class P>
static int mp_run(int device, uint32_t n, const K* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, const uint8_t* absent_bits, const uint8_t* empties,
                  uint8_t* paths, uint8_t* root, uint64_t* digests, double* ms) {
    static_assert(sizeof(K) == sizeof(P), "the plan reads the indices as they are");
    if (count == 0) return pv_fail(DST_ERR_ARG, "a multiproof of no leaf proves nothing");
    if (!indices || !leaves || (!nodes && num_nodes)) return pv_fail(DST_ERR_ARG, "null pointer");
    if (const char* why = pv_check_shape_of<K>(n, indices, count)) return pv_fail(DST_ERR_ARG, why);
    if (absent_bits && !empties) return pv_fail(DST_ERR_ARG, "absent_bits without empties: the compact form needs the table of empty subtrees");
    if (!absent_bits && empties) return pv_fail(DST_ERR_ARG, "empties without absent_bits: the plain form takes no table");
    if (empties && !all_below_p(empties, 2 * (size_t)n)) return pv_fail(DST_ERR_ARG, "an element of empties is not below the modulus");
    double device_ms = 0;
    try {
        mp_plan_t<P> p;
        std::vector<uint8_t> leaf_empty;
        if (absent_bits) {                                                 // by value: a leaf that equals E_D is an empty subtree whoever stored it
            leaf_empty.resize(count);
            for (size_t i = 0; i < count; i++) leaf_empty[i] = pv_same(leaves + 32 * i, empties + 32 * (size_t)(n - 1));
        }
        if (const char* why = mp_plan_make(n - 1, reinterpret_cast<const P*>(indices), count, MP_JOBS | (paths ? MP_WHERE : 0u), p, absent_bits, absent_bits ? leaf_empty.data() : nullptr))
            return pv_fail(DST_ERR_ARG, why);
        if (num_nodes != p.shipped)
            return pv_fail(DST_ERR_ARG, absent_bits ? "num_nodes is not the number of supplied nodes of these indices less the bits set in absent_bits"
                                                    : "num_nodes is not the number of supplied nodes of these indices");
        const size_t S = p.shipped;
        if (device < 0 || p.sizes.digests == 0) {                          // nothing to hash: the root is E_0, and nothing is queued anywhere
            if (!all_below_p(leaves, 2 * count) || !all_below_p(nodes, 2 * S)) return pv_fail(DST_ERR_ARG, MP_NOT_BELOW_P);
            std::vector<u128> pool(2 * p.pool());                          // the caller's buffers need only byte alignment
            memcpy(pool.data(), leaves, 32 * count);
            if (S) memcpy(pool.data() + 2 * count, nodes, 32 * S);
            if (p.table) memcpy(pool.data() + 2 * (count + S), empties, 32 * p.table);
            mp_hash_host(p, pool);
            for (size_t s = 0; s < p.where.size(); s++) memcpy(paths + 32 * s, &pool[2 * (size_t)p.where[s]], 32);
            memcpy(root, &pool[2 * (size_t)p.root], 32);
        } else {
            std::vector<uint8_t> back;
            if (int r = mp_hash_device(device, p, leaves, nodes, empties, paths != nullptr, back, &device_ms)) return r;
            memcpy(root, back.data(), 32);
            if (paths) memcpy(paths, back.data() + 32, 32 * p.where.size());
        }
        if (digests) *digests = p.sizes.digests;
        g_mp_levels = p.levels;
    } catch (const std::bad_alloc&) { return pv_fail(DST_ERR_HIP, "out of host memory"); }
    if (ms) *ms = device_ms;
    return DST_OK;
}
template <class K, class P>
static int mp_root(int device, uint32_t n, const K* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, const uint8_t* absent_bits, const uint8_t* empties,
                   uint8_t root[32], uint64_t* digests, double* device_ms) {
    if (device_ms) *device_ms = 0;
    if (!root) return pv_fail(DST_ERR_ARG, "null pointer");
    return mp_run<K, P>(device, n, indices, leaves, count, nodes, num_nodes, absent_bits, empties, nullptr, root, digests, device_ms);
}
template <class K, class P>
static int mp_verify(int device, const uint8_t root[32], uint32_t n, const K* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, const uint8_t* absent_bits,
                     const uint8_t* empties, int* ok, double* device_ms) {
    if (device_ms) *device_ms = 0;
    if (!ok || !root) return pv_fail(DST_ERR_ARG, "null pointer");
    *ok = 0;
    uint8_t own[32];
    if (int r = mp_run<K, P>(device, n, indices, leaves, count, nodes, num_nodes, absent_bits, empties, nullptr, own, nullptr, device_ms)) return r;
    *ok = pv_same(own, root) ? 1 : 0;
    return DST_OK;
}
template <class K, class P>
static int mp_paths(int device, uint32_t n, const K* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, const uint8_t* absent_bits, const uint8_t* empties,
                    uint8_t* paths, uint8_t root[32], double* device_ms) {
    if (device_ms) *device_ms = 0;
    if (!paths || !root) return pv_fail(DST_ERR_ARG, "null pointer");
    return mp_run<K, P>(device, n, indices, leaves, count, nodes, num_nodes, absent_bits, empties, paths, root, nullptr, device_ms);
}

int dst_rescue_multiproof_root(int device, uint32_t n, const uint64_t* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, uint8_t root[32],
                               uint64_t* digests, double* device_ms) {
    return mp_root<uint64_t, uint64_t>(device, n, indices, leaves, count, nodes, num_nodes, nullptr, nullptr, root, digests, device_ms);
}
int dst_rescue_verify_multiproof(int device, const uint8_t root[32], uint32_t n, const uint64_t* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes,
                                 int* ok, double* device_ms) {
    return mp_verify<uint64_t, uint64_t>(device, root, n, indices, leaves, count, nodes, num_nodes, nullptr, nullptr, ok, device_ms);
}
int dst_rescue_multiproof_paths(int device, uint32_t n, const uint64_t* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, uint8_t* paths,
                                uint8_t root[32], double* device_ms) {
    return mp_paths<uint64_t, uint64_t>(device, n, indices, leaves, count, nodes, num_nodes, nullptr, nullptr, paths, root, device_ms);
}

// ---- the same calls over 16-byte indices (n <= 128), plain or compact ----------------------------------------------------------------------------
int dst_rescue_empty_nodes(const uint8_t empty_leaf[32], uint32_t n, uint8_t* out) {
    if (!out) return pv_fail(DST_ERR_ARG, "null pointer");
    if (n < PV_MIN_NODES || n > PV_WIDE_MAX_NODES) return pv_fail(DST_ERR_ARG, "a path has 2 .. 128 nodes");
    if (empty_leaf && !all_below_p(empty_leaf, 2)) return pv_fail(DST_ERR_ARG, "an element of the empty leaf is not below the modulus");
    u128 e[2 * PV_WIDE_MAX_NODES] = {0};
    if (empty_leaf) memcpy(e + 2 * (size_t)(n - 1), empty_leaf, 32);
    for (uint32_t l = n - 1; l-- > 0;) {                                   // E_l = digest(E_{l+1}, E_{l+1}), as dst_wtree_create
        const u128 in[4] = {e[2 * l + 2], e[2 * l + 3], e[2 * l + 2], e[2 * l + 3]};
        rescue_digest_many_host(in, 1, e + 2 * l);
    }
    memcpy(out, e, 32 * (size_t)n);
    return DST_OK;
}
int dst_rescue_multiproof_size_w(uint32_t n, const uint8_t* indices, size_t count, size_t* num_nodes, uint64_t* digests) {
    if (!num_nodes || !digests || (!indices && count)) return pv_fail(DST_ERR_ARG, "null pointer");
    *num_nodes = 0; *digests = 0;
    const pv_wide_indices w(indices, count);
    if (w.code) return w.code;
    if (const char* why = pv_check_shape_of<u128>(n, w.p, count)) return pv_fail(DST_ERR_ARG, why);
    if (count == 0) return DST_OK;
    try {
        mp_plan_t<stree_wide> p;
        if (const char* why = mp_plan_make(n - 1, reinterpret_cast<const stree_wide*>(w.p), count, 0, p)) return pv_fail(DST_ERR_ARG, why);
        *num_nodes = (size_t)p.sizes.nodes; *digests = p.sizes.digests;
    } catch (const std::bad_alloc&) { return pv_fail(DST_ERR_HIP, "out of host memory"); }
    return DST_OK;
}
int dst_rescue_multiproof_root_w(int device, uint32_t n, const uint8_t* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, const uint8_t* absent_bits,
                                 const uint8_t* empties, uint8_t root[32], uint64_t* digests, double* device_ms) {
    if (device_ms) *device_ms = 0;
    const pv_wide_indices w(indices, count);
    return w.code ? w.code : mp_root<u128, stree_wide>(device, n, w.p, leaves, count, nodes, num_nodes, absent_bits, empties, root, digests, device_ms);
}
int dst_rescue_verify_multiproof_w(int device, const uint8_t root[32], uint32_t n, const uint8_t* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes,
                                   const uint8_t* absent_bits, const uint8_t* empties, int* ok, double* device_ms) {
    if (device_ms) *device_ms = 0;
    const pv_wide_indices w(indices, count);
    return w.code ? w.code : mp_verify<u128, stree_wide>(device, root, n, w.p, leaves, count, nodes, num_nodes, absent_bits, empties, ok, device_ms);
}
int dst_rescue_multiproof_paths_w(int device, uint32_t n, const uint8_t* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, const uint8_t* absent_bits,
                                  const uint8_t* empties, uint8_t* paths, uint8_t root[32], double* device_ms) {
    if (device_ms) *device_ms = 0;
    const pv_wide_indices w(indices, count);
    return w.code ? w.code : mp_paths<u128, stree_wide>(device, n, w.p, leaves, count, nodes, num_nodes, absent_bits, empties, paths, root, device_ms);
}
uint32_t dst_rescue_multiproof_last_levels(void) { return g_mp_levels; }
