// dst_rescue_multiproof_size, dst_rtree_multiproof / dst_stree_multiproof and the tree-less dst_rescue_multiproof_root / dst_rescue_verify_multiproof /
// dst_rescue_multiproof_paths: the plan of host/multiproof_plan.h run where the caller says.  Included by api.hip alone, after stree_impl.h and
// path_verify_impl.h, whose conventions these calls keep: the tree-less ones file errors with dst_rtree_last_error(NULL), device < 0 is the host
// with one thread and no HIP call, and everything but an element that is not below p is refused before anything is queued.
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

// ---- without a tree: every ancestor the paths share is hashed once ------------------------------------------------------------------------------
// the pool on the host: [leaves | nodes] are in place and below p; one rescue_digest_many_host call per level over all of its jobs, whose results
// are consecutive pool nodes
static void mp_hash_host(const mp_plan& p, std::vector<u128>& pool) {
    size_t most = 0;
    for (uint32_t l = 0; l < p.depth; l++) most = std::max(most, p.jcnt[l]);
    std::vector<u128> in(4 * most);
    for (uint32_t l = p.depth; l-- > 0;) {
        const uint32_t* jobs = p.jobs.data() + 3 * p.joff[l];
        for (size_t g = 0; g < p.jcnt[l]; g++) {
            memcpy(&in[4 * g], &pool[2 * (size_t)jobs[3 * g]], 32);
            memcpy(&in[4 * g + 2], &pool[2 * (size_t)jobs[3 * g + 1]], 32);
        }
        rescue_digest_many_host(in.data(), p.jcnt[l], &pool[2 * (size_t)jobs[2]]);
    }
}
// ... and on a device.  p = [job lists][path node indices][leaves][nodes] -- one upload; the pool begins at the leaves and goes on behind the
// upload -- then [paths][bad]; at most `depth` level launches and, for the expansion, one gather launch between two events; one synchronisation;
// one copy back, from the root -- the last node of the pool -- to `bad`.  back = [root][paths]
static int mp_hash_device(int device, const mp_plan& p, const uint8_t* leaves, const uint8_t* nodes, bool expand, std::vector<uint8_t>& back, double* ms) {
    const size_t count = p.count, M = p.inputs() - count, W = expand ? p.where.size() : 0;
    const size_t o_where = 4 * p.jobs.size(), o_pool = (o_where + 4 * W + 15) & ~(size_t)15, up_bytes = o_pool + 32 * p.inputs();
    const size_t o_root = o_pool + 32 * (p.pool() - 1), o_paths = o_root + 32, o_bad = o_paths + 32 * W, total = o_bad + 4;
    std::vector<uint8_t> up(up_bytes);                                     // the last host allocations: nothing is queued yet
    back.resize(total - o_root);
    memcpy(up.data(), p.jobs.data(), o_where);
    if (W) memcpy(up.data() + o_where, p.where.data(), 4 * W);
    memcpy(up.data() + o_pool, leaves, 32 * count);
    if (M) memcpy(up.data() + o_pool + 32 * count, nodes, 32 * M);
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
        if (k_rescue_multiproof_level(h.s, pool, d_jobs + 3 * p.joff[l], p.jcnt[l], (uint32_t)p.inputs(), d_bad)) return pv_fail(DST_ERR_HIP, "rescue_multiproof_level_kernel: launch failed");
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
// what the three calls share: the argument checks, the plan, the hashing.  root, paths (may be nullptr: no expansion), digests and ms (may be
// nullptr) are written only when everything holds
static int mp_run(int device, uint32_t n, const uint64_t* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, uint8_t* paths, uint8_t* root,
                  uint64_t* digests, double* ms) {
    if (count == 0) return pv_fail(DST_ERR_ARG, "a multiproof of no leaf proves nothing");
    if (!indices || !leaves || (!nodes && num_nodes)) return pv_fail(DST_ERR_ARG, "null pointer");
    if (const char* why = pv_check_shape(n, indices, count)) return pv_fail(DST_ERR_ARG, why);
    double device_ms = 0;
    try {
        mp_plan p;
        if (const char* why = mp_plan_make(n - 1, indices, count, MP_JOBS | (paths ? MP_WHERE : 0u), p)) return pv_fail(DST_ERR_ARG, why);
        if (num_nodes != p.sizes.nodes) return pv_fail(DST_ERR_ARG, "num_nodes is not the number of supplied nodes of these indices");
        if (device < 0) {
            if (!all_below_p(leaves, 2 * count) || !all_below_p(nodes, 2 * num_nodes)) return pv_fail(DST_ERR_ARG, MP_NOT_BELOW_P);
            std::vector<u128> pool(2 * p.pool());                          // the caller's buffers need only byte alignment
            memcpy(pool.data(), leaves, 32 * count);
            if (num_nodes) memcpy(pool.data() + 2 * count, nodes, 32 * num_nodes);
            mp_hash_host(p, pool);
            for (size_t s = 0; s < p.where.size(); s++) memcpy(paths + 32 * s, &pool[2 * (size_t)p.where[s]], 32);
            memcpy(root, &pool[2 * (p.pool() - 1)], 32);
        } else {
            std::vector<uint8_t> back;
            if (int r = mp_hash_device(device, p, leaves, nodes, paths != nullptr, back, &device_ms)) return r;
            memcpy(root, back.data(), 32);
            if (paths) memcpy(paths, back.data() + 32, 32 * p.where.size());
        }
        if (digests) *digests = p.sizes.digests;
    } catch (const std::bad_alloc&) { return pv_fail(DST_ERR_HIP, "out of host memory"); }
    if (ms) *ms = device_ms;
    return DST_OK;
}

int dst_rescue_multiproof_root(int device, uint32_t n, const uint64_t* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, uint8_t root[32],
                               uint64_t* digests, double* device_ms) {
    if (device_ms) *device_ms = 0;
    if (!root) return pv_fail(DST_ERR_ARG, "null pointer");
    return mp_run(device, n, indices, leaves, count, nodes, num_nodes, nullptr, root, digests, device_ms);
}
int dst_rescue_verify_multiproof(int device, const uint8_t root[32], uint32_t n, const uint64_t* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes,
                                 int* ok, double* device_ms) {
    if (device_ms) *device_ms = 0;
    if (!ok || !root) return pv_fail(DST_ERR_ARG, "null pointer");
    *ok = 0;
    uint8_t own[32];
    if (int r = mp_run(device, n, indices, leaves, count, nodes, num_nodes, nullptr, own, nullptr, device_ms)) return r;
    *ok = pv_same(own, root) ? 1 : 0;
    return DST_OK;
}
int dst_rescue_multiproof_paths(int device, uint32_t n, const uint64_t* indices, const uint8_t* leaves, size_t count, const uint8_t* nodes, size_t num_nodes, uint8_t* paths,
                                uint8_t root[32], double* device_ms) {
    if (device_ms) *device_ms = 0;
    if (!paths || !root) return pv_fail(DST_ERR_ARG, "null pointer");
    return mp_run(device, n, indices, leaves, count, nodes, num_nodes, paths, root, nullptr, device_ms);
}
