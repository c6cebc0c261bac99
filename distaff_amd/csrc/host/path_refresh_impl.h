// dst_rescue_refresh_paths: the witnesses of ordered writes turn the paths a client holds into its paths under the new root -- without a tree.
// Included by api.hip alone, after path_verify_impl.h, whose checks, chains and conventions these calls keep: the writes are verified exactly as
// dst_rescue_verify_writes verifies them (pv_decide_writes decides), errors are filed with dst_rtree_last_error(NULL).  What is new is that the
// chains of the written leaves leave their nodes behind (k_rescue_path_chains, path_roots_host with `mid`) and that the plan of host/path_refresh.h
// gathers them into the held paths.  out_paths is written on the host, after the verdict: all of it, or nothing.  Stated once over the index type K.
#pragma once
#include "path_refresh.h"
#include "path_verify_impl.h"

static thread_local double g_refresh_gather_ms = 0;                        // dst_rescue_refresh_last_gather_ms
struct pr_event {                                                          // the event between the two launches
    hipEvent_t e = nullptr;
    ~pr_event() { if (e) hipEventDestroy(e); }
};

// the refreshed node (j, k) on the host: see rescue_path_refresh_kernel
static const uint8_t* pr_node(const uint8_t* held_paths, const int32_t* sel, const uint8_t* leaves, const u128* mid, size_t count, uint32_t n, size_t j, uint32_t k) {
    const int32_t s = sel[(size_t)n * j + k];
    if (s < 0) return held_paths + 32 * ((size_t)n * j + k);
    return k <= 1 ? leaves + 32 * (size_t)s : (const uint8_t*)(mid + 2 * ((size_t)(k - 2) * count + (size_t)s));
}

// p = [paths][new leaves][held paths][indices][sel] -- one upload -- then [refreshed paths][bad][roots] -- one copy back -- and the chain nodes behind
// the roots, which stay on the device.  ONE chain launch and one gather launch between two events, a third between them for the gather's own time;
// one synchronisation.  down = [refreshed paths][16 bytes that begin with bad][roots 2 * count]
template <class K>
static int refresh_device(int device, const uint8_t* paths, uint32_t n, const K* indices, const uint8_t* leaves, size_t count, const uint8_t* held_paths, size_t held,
                          const int32_t* sel, std::vector<uint8_t>& down, double* ms) {
    const size_t b_paths = 32 * (size_t)n * count, b_held = 32 * (size_t)n * held, b_roots = 64 * count, b_down = b_held + 16 + b_roots;
    const size_t o_leaves = b_paths, o_held = o_leaves + 32 * count, o_idx = o_held + b_held, o_sel = o_idx + sizeof(K) * count, up_bytes = o_sel + 4 * (size_t)n * held;
    const size_t o_out = (up_bytes + 15) & ~(size_t)15, o_bad = o_out + b_held, o_roots = o_bad + 16, total = o_roots + b_roots + 32 * (size_t)(n - 2) * count;
    std::vector<uint8_t> up(up_bytes);                                     // the last host allocations: nothing is queued yet
    down.resize(b_down);
    memcpy(up.data(), paths, b_paths);
    memcpy(up.data() + o_leaves, leaves, 32 * count);
    memcpy(up.data() + o_held, held_paths, b_held);
    memcpy(up.data() + o_idx, indices, sizeof(K) * count);
    memcpy(up.data() + o_sel, sel, 4 * (size_t)n * held);
    rt_scratch h;
    pr_event between;
    RT_HIP(g_rtree_error, hipSetDevice(device));
    RT_HIP(g_rtree_error, hipStreamCreateWithFlags(&h.s, hipStreamNonBlocking));
    RT_HIP(g_rtree_error, hipEventCreate(&h.ev[0]));
    RT_HIP(g_rtree_error, hipEventCreate(&h.ev[1]));
    RT_HIP(g_rtree_error, hipEventCreate(&between.e));
    RT_HIP(g_rtree_error, hipMalloc((void**)&h.p, total));
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(h.p + o_bad);
    const fe* d_leaves = reinterpret_cast<const fe*>(h.p + o_leaves);
    fe* d_roots = reinterpret_cast<fe*>(h.p + o_roots);
    RT_HIP(g_rtree_error, hipMemsetAsync(d_bad, 0, 16, h.s));
    RT_HIP(g_rtree_error, hipMemcpyAsync(h.p, up.data(), up_bytes, hipMemcpyHostToDevice, h.s));
    RT_HIP(g_rtree_error, hipEventRecord(h.ev[0], h.s));
    typedef typename std::conditional<sizeof(K) == 8, uint64_t, stree_wide>::type dev_key;
    if (k_rescue_path_chains(h.s, reinterpret_cast<const fe*>(h.p), n, reinterpret_cast<const dev_key*>(h.p + o_idx), count, d_leaves, d_roots, d_bad))
        return pv_fail(DST_ERR_HIP, "rescue_path_root_kernel: launch failed");
    RT_HIP(g_rtree_error, hipEventRecord(between.e, h.s));
    if (k_rescue_path_refresh(h.s, reinterpret_cast<const fe*>(h.p + o_held), reinterpret_cast<const int32_t*>(h.p + o_sel), d_leaves, d_roots + 4 * count, count, n, held,
                              reinterpret_cast<fe*>(h.p + o_out), d_bad))
        return pv_fail(DST_ERR_HIP, "rescue_path_refresh_kernel: launch failed");
    RT_HIP(g_rtree_error, hipEventRecord(h.ev[1], h.s));
    RT_HIP(g_rtree_error, hipMemcpyAsync(down.data(), h.p + o_out, b_down, hipMemcpyDeviceToHost, h.s));
    RT_HIP(g_rtree_error, hipStreamSynchronize(h.s));
    float f = 0;
    RT_HIP(g_rtree_error, hipEventElapsedTime(&f, h.ev[0], h.ev[1]));
    *ms = f;
    RT_HIP(g_rtree_error, hipEventElapsedTime(&f, between.e, h.ev[1]));
    g_refresh_gather_ms = f;
    uint32_t bad = 0;
    memcpy(&bad, down.data() + b_held, 4);
    if (bad) return pv_fail(DST_ERR_ARG, PV_NOT_BELOW_P);
    return DST_OK;
}

template <class K>
static int pr_refresh_paths(int device, const uint8_t root_before[32], const uint8_t* paths, uint32_t n, const K* indices, const uint8_t* leaves, const uint8_t* roots, size_t count,
                            const K* held_indices, const uint8_t* held_paths, size_t held, uint8_t* out_paths, int64_t* first_bad, uint32_t* why, uint8_t root_after[32],
                            double* device_ms) {
    g_refresh_gather_ms = 0;
    if (held == 0) return pv_verify_writes(device, root_before, paths, n, indices, leaves, roots, count, first_bad, why, root_after, device_ms);
    if (device_ms) *device_ms = 0;
    if (!first_bad || !why || !root_before || ((!paths || !indices || !leaves) && count) || !held_indices || !held_paths || !out_paths) return pv_fail(DST_ERR_ARG, "null pointer");
    *first_bad = -1; *why = DST_PATH_OK;
    if (const char* w = pv_check_shape_of<K>(n, indices, count)) return pv_fail(DST_ERR_ARG, w);
    if (const char* w = pv_check_shape_of<K>(n, held_indices, held)) return pv_fail(DST_ERR_ARG, w);
    if (!all_below_p(root_before, 2) || (roots && count && !all_below_p(roots, 2 * count))) return pv_fail(DST_ERR_ARG, PV_NOT_BELOW_P);      // what the host compares
    const size_t b_held = 32 * (size_t)n * held;
    if (count == 0) {                                                      // no write: the paths and the state stay
        if (!all_below_p(held_paths, 2 * (size_t)n * held)) return pv_fail(DST_ERR_ARG, PV_NOT_BELOW_P);
        memmove(out_paths, held_paths, b_held);
        if (root_after) memcpy(root_after, root_before, 32);
        return DST_OK;
    }
    double ms = 0;
    try {
        std::vector<int32_t> sel((size_t)n * held);
        pr_plan(n, indices, count, held_indices, held, sel.data());
        std::vector<u128> chain, mid;                                      // host: the 2 * count roots, the nodes of the written leaves' chains
        std::vector<uint8_t> down;                                         // device: the refreshed paths and the roots
        if (device < 0) {
            if (!all_below_p(paths, 2 * (size_t)n * count) || !all_below_p(leaves, 2 * count) || !all_below_p(held_paths, 2 * (size_t)n * held))
                return pv_fail(DST_ERR_ARG, PV_NOT_BELOW_P);
            chain.assign(4 * count, 0); mid.assign(2 * (size_t)(n - 2) * count + 2, 0);
            path_roots_host(paths, n, indices, count, leaves, RESCUE_PATH_BOTH, chain.data(), mid.data());
        } else if (int r = refresh_device(device, paths, n, indices, leaves, count, held_paths, held, sel.data(), down, &ms)) return r;
        const uint8_t* own = device < 0 ? (const uint8_t*)chain.data() : down.data() + 32 * (size_t)n * held + 16;
        const pv_verdict v = pv_decide_writes(own, own + 32 * count, root_before, roots, count, root_after);
        *first_bad = v.first_bad; *why = v.why;
        if (device_ms) *device_ms = ms;
        if (v.first_bad >= 0) return DST_OK;                               // nothing is written from witnesses that do not hold
        if (device >= 0) memcpy(out_paths, down.data(), b_held);
        else
            for (size_t j = 0; j < held; j++)                              // node by node: out_paths may be held_paths itself
                for (uint32_t k = 0; k < n; k++) memmove(out_paths + 32 * ((size_t)n * j + k), pr_node(held_paths, sel.data(), leaves, mid.data(), count, n, j, k), 32);
    } catch (const std::bad_alloc&) { return pv_fail(DST_ERR_HIP, "out of host memory"); }
    return DST_OK;
}

int dst_rescue_refresh_paths(int device, const uint8_t root_before[32], const uint8_t* paths, uint32_t n, const uint64_t* indices, const uint8_t* leaves, const uint8_t* roots, size_t count,
                             const uint64_t* held_indices, const uint8_t* held_paths, size_t held, uint8_t* out_paths, int64_t* first_bad, uint32_t* why, uint8_t root_after[32],
                             double* device_ms) {
    return pr_refresh_paths(device, root_before, paths, n, indices, leaves, roots, count, held_indices, held_paths, held, out_paths, first_bad, why, root_after, device_ms);
}
double dst_rescue_refresh_last_gather_ms(void) { return g_refresh_gather_ms; }
int dst_rescue_refresh_paths_w(int device, const uint8_t root_before[32], const uint8_t* paths, uint32_t n, const uint8_t* indices, const uint8_t* leaves, const uint8_t* roots, size_t count,
                               const uint8_t* held_indices, const uint8_t* held_paths, size_t held, uint8_t* out_paths, int64_t* first_bad, uint32_t* why, uint8_t root_after[32],
                               double* device_ms) {
    if (device_ms) *device_ms = 0;
    const pv_wide_indices w(indices, count), hw(held_indices, held);
    if (w.code || hw.code) return w.code ? w.code : hw.code;
    return pr_refresh_paths(device, root_before, paths, n, w.p, leaves, roots, count, hw.p, held_paths, held, out_paths, first_bad, why, root_after, device_ms);
}
