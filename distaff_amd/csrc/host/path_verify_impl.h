// dst_rescue_path_roots / dst_rescue_verify_paths / dst_rescue_verify_writes: compute_merkle_root (src/examples/merkle.rs:112-145) of many paths at
// once and the verdicts of host/path_verify.h over the roots.  Included by api.hip alone, after rtree_impl.h, whose conventions these calls keep: no
// tree, no context; errors are filed with dst_rtree_last_error(NULL), as dst_rescue_path_tapes files them.  Each call is stated once over the index
// type K -- uint64_t (n <= 64) and u128 (the _w calls, n <= 128; the kernels read the same 16 bytes as stree_wide) -- the entry points follow at the end.
#pragma once
#include "path_verify.h"
#include "rtree_impl.h"
#include "stree_levels.h"

static_assert(PV_OK == DST_PATH_OK && PV_BAD_LEAF == DST_PATH_BAD_LEAF && PV_BAD_ROOT == DST_PATH_BAD_ROOT && PV_BAD_NEXT_ROOT == DST_PATH_BAD_NEXT_ROOT,
              "host/path_verify.h states the values of `why` for itself: they are the header's");
static int pv_fail(int code, const char* why) { g_rtree_error = why; return code; }
static const char* const PV_NOT_BELOW_P = "an element of the paths, leaves or roots is not below the modulus";

// the chains of `count` paths on the host: one level of ALL chains per rescue_digest_many_host call, so that its two-at-a-time form runs on full
// groups.  out = 2 elements per chain, in the order of k_rescue_path_roots.  The caller has checked that every element is below p.  mid (or
// nullptr; RESCUE_PATH_BOTH) receives what k_rescue_path_chains stores: the substitute-leaf chain of path i after level k at mid[k - 1][i], k <= n - 2
template <class K>
static void path_roots_host(const uint8_t* paths, uint32_t n, const K* indices, size_t count, const uint8_t* leaves, uint32_t mode, u128* out, u128* mid = nullptr) {
    const size_t chains = mode == RESCUE_PATH_BOTH ? 2 * count : count;
    std::vector<u128> in(4 * chains);
    for (size_t c = 0; c < chains; c++) {                                  // the running value starts as the leaf
        const size_t i = c < count ? c : c - count;
        memcpy(out + 2 * c, (mode == RESCUE_PATH_ALT || c >= count) ? leaves + 32 * i : paths + 32 * (size_t)n * i, 32);
    }
    for (uint32_t k = 1; k < n; k++) {
        for (size_t c = 0; c < chains; c++) {
            const size_t i = c < count ? c : c - count;
            const size_t right = (size_t)(indices[i] >> (k - 1)) & 1;              // the running node is the right child: the sibling goes first
            memcpy(in.data() + 4 * c + 2 * right, out + 2 * c, 32);
            memcpy(in.data() + 4 * c + 2 * (1 - right), paths + 32 * ((size_t)n * i + k), 32);
        }
        rescue_digest_many_host(in.data(), chains, out);
        if (mid && k + 1 < n)
            memcpy(mid + 2 * (size_t)(k - 1) * count, out + 2 * count, 32 * count);
    }
}

// p = [paths][substitute leaves][indices] -- one upload -- then [roots][bad] -- one copy back; ONE launch between two events; one synchronisation
template <class K>
static int path_roots_device(int device, const uint8_t* paths, uint32_t n, const K* indices, size_t count, const uint8_t* leaves, uint32_t mode, u128* out, double* ms) {
    const size_t chains = mode == RESCUE_PATH_BOTH ? 2 * count : count;
    const size_t o_alt = 32 * (size_t)n * count, o_idx = o_alt + (leaves ? 32 * count : 0), up_bytes = o_idx + sizeof(K) * count;
    const size_t o_out = (up_bytes + 15) & ~(size_t)15, o_bad = o_out + 32 * chains, total = o_bad + 4;
    std::vector<uint8_t> up(up_bytes), down(32 * chains + 4);              // the last host allocations: nothing is queued yet
    memcpy(up.data(), paths, o_alt);
    if (leaves) memcpy(up.data() + o_alt, leaves, 32 * count);
    memcpy(up.data() + o_idx, indices, sizeof(K) * count);
    rt_scratch h;
    RT_HIP(g_rtree_error, hipSetDevice(device));
    RT_HIP(g_rtree_error, hipStreamCreateWithFlags(&h.s, hipStreamNonBlocking));
    RT_HIP(g_rtree_error, hipEventCreate(&h.ev[0]));
    RT_HIP(g_rtree_error, hipEventCreate(&h.ev[1]));
    RT_HIP(g_rtree_error, hipMalloc((void**)&h.p, total));
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(h.p + o_bad);
    RT_HIP(g_rtree_error, hipMemsetAsync(d_bad, 0, 4, h.s));
    RT_HIP(g_rtree_error, hipMemcpyAsync(h.p, up.data(), up_bytes, hipMemcpyHostToDevice, h.s));
    RT_HIP(g_rtree_error, hipEventRecord(h.ev[0], h.s));
    typedef typename std::conditional<sizeof(K) == 8, uint64_t, stree_wide>::type dev_key;
    if (k_rescue_path_roots(h.s, reinterpret_cast<const fe*>(h.p), n, reinterpret_cast<const dev_key*>(h.p + o_idx), count, leaves ? reinterpret_cast<const fe*>(h.p + o_alt) : nullptr, mode,
                            reinterpret_cast<fe*>(h.p + o_out), d_bad))
        return pv_fail(DST_ERR_HIP, "rescue_path_root_kernel: launch failed");
    RT_HIP(g_rtree_error, hipEventRecord(h.ev[1], h.s));
    RT_HIP(g_rtree_error, hipMemcpyAsync(down.data(), h.p + o_out, 32 * chains + 4, hipMemcpyDeviceToHost, h.s));
    RT_HIP(g_rtree_error, hipStreamSynchronize(h.s));
    float f = 0;
    RT_HIP(g_rtree_error, hipEventElapsedTime(&f, h.ev[0], h.ev[1]));
    *ms = f;
    uint32_t bad = 0;
    memcpy(&bad, down.data() + 32 * chains, 4);
    if (bad) return pv_fail(DST_ERR_ARG, PV_NOT_BELOW_P);
    memcpy(out, down.data(), 32 * chains);
    return DST_OK;
}

// what the three calls share: the argument checks of host/path_verify.h, then the chains of `mode` -> out (2 elements per chain); count >= 1.  The
// host checks what only the host reads -- the first nodes of the paths when substitute leaves alone are hashed -- and, on the host path, everything.
template <class K>
static int path_roots_run(int device, const uint8_t* paths, uint32_t n, const K* indices, size_t count, const uint8_t* leaves, uint32_t mode, std::vector<u128>& out, double* ms) {
    if (const char* why = pv_check_shape_of<K>(n, indices, count)) return pv_fail(DST_ERR_ARG, why);
    double device_ms = 0;
    try {
        out.assign(2 * (mode == RESCUE_PATH_BOTH ? 2 * count : count), 0);
        if (device < 0) {
            if (!all_below_p(paths, 2 * (size_t)n * count) || (leaves && !all_below_p(leaves, 2 * count))) return pv_fail(DST_ERR_ARG, PV_NOT_BELOW_P);
            path_roots_host(paths, n, indices, count, leaves, mode, out.data());
        } else {
            if (mode == RESCUE_PATH_ALT)
                for (size_t i = 0; i < count; i++) if (!all_below_p(paths + 32 * (size_t)n * i, 2)) return pv_fail(DST_ERR_ARG, PV_NOT_BELOW_P);
            if (int r = path_roots_device(device, paths, n, indices, count, leaves, mode, out.data(), &device_ms)) return r;
        }
    } catch (const std::bad_alloc&) { return pv_fail(DST_ERR_HIP, "out of host memory"); }
    if (ms) *ms = device_ms;
    return DST_OK;
}

template <class K>
static int pv_path_roots(int device, const uint8_t* paths, uint32_t n, const K* indices, size_t count, const uint8_t* leaves, uint8_t* roots, double* device_ms) {
    if (device_ms) *device_ms = 0;
    if ((!paths || !indices || !roots) && count) return pv_fail(DST_ERR_ARG, "null pointer");
    if (count == 0) { const char* why = pv_check_shape_of<K>(n, nullptr, 0); return why ? pv_fail(DST_ERR_ARG, why) : DST_OK; }
    std::vector<u128> out;
    if (int r = path_roots_run(device, paths, n, indices, count, leaves, leaves ? RESCUE_PATH_ALT : RESCUE_PATH_OWN, out, device_ms)) return r;
    memcpy(roots, out.data(), 32 * count);
    return DST_OK;
}

template <class K>
static int pv_verify_paths(int device, const uint8_t root[32], const uint8_t* paths, uint32_t n, const K* indices, const uint8_t* leaves, size_t count, int64_t* first_bad,
                           uint32_t* why, double* device_ms) {
    if (device_ms) *device_ms = 0;
    if (!first_bad || !why || !root || ((!paths || !indices) && count)) return pv_fail(DST_ERR_ARG, "null pointer");
    *first_bad = -1; *why = DST_PATH_OK;
    if (count == 0) { const char* w = pv_check_shape_of<K>(n, nullptr, 0); return w ? pv_fail(DST_ERR_ARG, w) : DST_OK; }
    if (!all_below_p(root, 2) || (leaves && !all_below_p(leaves, 2 * count))) return pv_fail(DST_ERR_ARG, PV_NOT_BELOW_P);      // what the host compares
    std::vector<u128> out;
    if (int r = path_roots_run(device, paths, n, indices, count, nullptr, RESCUE_PATH_OWN, out, device_ms)) return r;
    const pv_verdict v = pv_decide_paths((const uint8_t*)out.data(), root, paths, n, leaves, count);
    *first_bad = v.first_bad; *why = v.why;
    return DST_OK;
}

template <class K>
static int pv_verify_writes(int device, const uint8_t root_before[32], const uint8_t* paths, uint32_t n, const K* indices, const uint8_t* leaves, const uint8_t* roots, size_t count,
                            int64_t* first_bad, uint32_t* why, uint8_t root_after[32], double* device_ms) {
    if (device_ms) *device_ms = 0;
    if (!first_bad || !why || !root_before || ((!paths || !indices || !leaves) && count)) return pv_fail(DST_ERR_ARG, "null pointer");
    *first_bad = -1; *why = DST_PATH_OK;
    if (const char* w = count ? nullptr : pv_check_shape_of<K>(n, nullptr, 0)) return pv_fail(DST_ERR_ARG, w);
    if (!all_below_p(root_before, 2) || (roots && count && !all_below_p(roots, 2 * count))) return pv_fail(DST_ERR_ARG, PV_NOT_BELOW_P);      // what the host compares
    std::vector<u128> out;
    if (count) { if (int r = path_roots_run(device, paths, n, indices, count, leaves, RESCUE_PATH_BOTH, out, device_ms)) return r; }
    const uint8_t* own = (const uint8_t*)out.data();
    const pv_verdict v = pv_decide_writes(own, own + 32 * count, root_before, roots, count, root_after);
    *first_bad = v.first_bad; *why = v.why;
    return DST_OK;
}

int dst_rescue_path_roots(int device, const uint8_t* paths, uint32_t n, const uint64_t* indices, size_t count, const uint8_t* leaves, uint8_t* roots, double* device_ms) {
    return pv_path_roots(device, paths, n, indices, count, leaves, roots, device_ms);
}
int dst_rescue_verify_paths(int device, const uint8_t root[32], const uint8_t* paths, uint32_t n, const uint64_t* indices, const uint8_t* leaves, size_t count, int64_t* first_bad,
                            uint32_t* why, double* device_ms) {
    return pv_verify_paths(device, root, paths, n, indices, leaves, count, first_bad, why, device_ms);
}
int dst_rescue_verify_writes(int device, const uint8_t root_before[32], const uint8_t* paths, uint32_t n, const uint64_t* indices, const uint8_t* leaves, const uint8_t* roots, size_t count,
                             int64_t* first_bad, uint32_t* why, uint8_t root_after[32], double* device_ms) {
    return pv_verify_writes(device, root_before, paths, n, indices, leaves, roots, count, first_bad, why, root_after, device_ms);
}

// the same calls over 16-byte little-endian indices at any alignment: copied into u128 first.  A count the calls refuse anyway (2^31 or more) is
// refused before the copy
struct pv_wide_indices {
    std::vector<u128> v;
    const u128* p = nullptr;
    int code = DST_OK;
    pv_wide_indices(const uint8_t* indices, size_t count) {
        if (!indices || count == 0) return;
        if ((uint64_t)count >= ((uint64_t)1 << 31)) { code = pv_fail(DST_ERR_ARG, "2^31 paths or more"); return; }
        try { v.resize(count); memcpy(v.data(), indices, 16 * count); p = v.data(); } catch (const std::bad_alloc&) { code = pv_fail(DST_ERR_HIP, "out of host memory"); }
    }
};
int dst_rescue_path_roots_w(int device, const uint8_t* paths, uint32_t n, const uint8_t* indices, size_t count, const uint8_t* leaves, uint8_t* roots, double* device_ms) {
    if (device_ms) *device_ms = 0;
    const pv_wide_indices w(indices, count);
    return w.code ? w.code : pv_path_roots(device, paths, n, w.p, count, leaves, roots, device_ms);
}
int dst_rescue_verify_paths_w(int device, const uint8_t root[32], const uint8_t* paths, uint32_t n, const uint8_t* indices, const uint8_t* leaves, size_t count, int64_t* first_bad,
                              uint32_t* why, double* device_ms) {
    if (device_ms) *device_ms = 0;
    const pv_wide_indices w(indices, count);
    return w.code ? w.code : pv_verify_paths(device, root, paths, n, w.p, leaves, count, first_bad, why, device_ms);
}
int dst_rescue_verify_writes_w(int device, const uint8_t root_before[32], const uint8_t* paths, uint32_t n, const uint8_t* indices, const uint8_t* leaves, const uint8_t* roots, size_t count,
                               int64_t* first_bad, uint32_t* why, uint8_t root_after[32], double* device_ms) {
    if (device_ms) *device_ms = 0;
    const pv_wide_indices w(indices, count);
    return w.code ? w.code : pv_verify_writes(device, root_before, paths, n, w.p, leaves, roots, count, first_bad, why, root_after, device_ms);
}
int dst_rescue_path_tapes_w(const uint8_t* paths, uint32_t n, const uint8_t* indices, size_t count, uint32_t what, uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each) {
    if (count > ((size_t)1 << 40)) { g_rtree_error = "too many indices"; return DST_ERR_ARG; }
    std::vector<u128> v;
    try { if (indices && count) { v.resize(count); memcpy(v.data(), indices, 16 * count); } } catch (const std::bad_alloc&) { g_rtree_error = "out of host memory"; return DST_ERR_HIP; }
    return path_tapes<u128>(paths, n, indices && count ? v.data() : nullptr, count, what, tape_a, tape_b, cap_elems_each, elems_each);
}
