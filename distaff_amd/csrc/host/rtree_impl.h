// Rescue digests and Rescue Merkle trees behind dst_rescue_digest_many / dst_rtree_* (kernels_hash.hip and rescue_dev.h on the device,
// host_rescue.h on the host): the implementation, included by api.hip alone.  Host code, and no prover context: a device tree owns its stream.
#pragma once
#include <algorithm>
#include <memory>
#include "../ctx.h"
#include "../host_rescue.h"
#include "tree_sequence.h"
#include "tree_blob.h"

struct dst_rtree {
    int device = -1;                      // < 0: the nodes live in `host`
    uint32_t log_leaves = 0;
    fe* dev = nullptr;                    // node array on the device: 2 elements per node, nodes[1] = root, nodes[leaves ..) = the leaves
    std::vector<u128> host;
    double device_ms = 0;                 // events around the level launches of the build
    double update_ms = 0;                 // ... and of the last dst_rtree_update / dst_rtree_apply
    bool broken = false;                  // a HIP error inside dst_rtree_update: the nodes are in an unknown state, only destroy / last_error remain
    // what the build, the updates and the openings of a device tree run on: rtree_stage creates the stream and the events with the build and
    // grows the staging buffer as calls need it (openings of a const tree too, hence mutable); they live as long as the tree
    mutable hipStream_t stream = nullptr;
    mutable hipEvent_t ev[2] = {nullptr, nullptr};
    mutable uint8_t* stage = nullptr; mutable size_t stage_bytes = 0;
    mutable std::string err;
    ~dst_rtree() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (dev) hipFree(dev);
        if (stage) hipFree(stage);
        for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
        if (stream) hipStreamDestroy(stream);
    }
};
static thread_local std::string g_rtree_error;         // error of the calling thread's last failed call without a tree (dst_rtree_last_error(NULL))
#define RT_HIP(errstr, expr)                                                                                              \
    do {                                                                                                                   \
        hipError_t _e = (expr);                                                                                            \
        if (_e != hipSuccess) { (errstr) = std::string(#expr) + ": " + hipGetErrorString(_e); return DST_ERR_HIP; }       \
    } while (0)
// how every call on a tree begins, and how it files an error
static int rt_enter(const dst_rtree* t) { return !t ? DST_ERR_ARG : t->broken ? DST_ERR_STATE : DST_OK; }
static int rt_fail(const dst_rtree* t, int code, const char* why) { t->err = why; return code; }
static bool all_below_p(const uint8_t* p, size_t elems) {
    for (size_t i = 0; i < elems; i++) { u128 v; memcpy(&v, p + 16 * i, 16); if (v >= FIELD_P) return false; }
    return true;
}
static bool all_leaf_indices(const dst_rtree* t, const uint64_t* indices, size_t count) {
    for (size_t i = 0; i < count; i++) if (indices[i] >> t->log_leaves) return false;
    return true;
}
struct rt_scratch {                                    // the stream and the device buffer of a call without a tree
    hipStream_t s = nullptr; uint8_t* p = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};             // around the launch, where the call reports device milliseconds
    ~rt_scratch() { if (p) hipFree(p); for (hipEvent_t e : ev) if (e) hipEventDestroy(e); if (s) hipStreamDestroy(s); }
};

// utils::hasher::digest (src/utils/hasher.rs:12)
int dst_rescue_digest_many(int device, const uint8_t* in, size_t count, uint8_t* out) {
    if ((!in || !out) && count) return DST_ERR_ARG;
    if (count == 0) return DST_OK;
    if (count > ((size_t)1 << 32)) return DST_ERR_ARG;
    if (device < 0) {
        if (!all_below_p(in, 4 * count)) { g_rtree_error = "an input element is not below the modulus"; return DST_ERR_ARG; }
        try {
            std::vector<u128> v(4 * count), d(2 * count);                  // the caller's buffers need only byte alignment
            memcpy(v.data(), in, 64 * count);
            rescue_digest_many_host(v.data(), count, d.data());
            memcpy(out, d.data(), 32 * count);
        } catch (const std::bad_alloc&) { g_rtree_error = "out of host memory"; return DST_ERR_HIP; }
        return DST_OK;
    }
    rt_scratch h;                                                          // p = [count inputs][count digests][bad]
    RT_HIP(g_rtree_error, hipSetDevice(device));
    RT_HIP(g_rtree_error, hipStreamCreateWithFlags(&h.s, hipStreamNonBlocking));
    RT_HIP(g_rtree_error, hipMalloc((void**)&h.p, count * 96 + 4));
    fe *d_in = reinterpret_cast<fe*>(h.p), *d_out = d_in + 4 * count;
    uint32_t *d_bad = reinterpret_cast<uint32_t*>(h.p + count * 96), bad = 0;
    RT_HIP(g_rtree_error, hipMemsetAsync(d_bad, 0, 4, h.s));
    RT_HIP(g_rtree_error, hipMemcpyAsync(d_in, in, count * 64, hipMemcpyHostToDevice, h.s));
    if (k_rescue_digests(h.s, d_in, d_out, count, d_bad)) { g_rtree_error = "rescue_digest_kernel: launch failed"; return DST_ERR_HIP; }
    RT_HIP(g_rtree_error, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, h.s));
    RT_HIP(g_rtree_error, hipMemcpyAsync(out, d_out, count * 32, hipMemcpyDeviceToHost, h.s));
    RT_HIP(g_rtree_error, hipStreamSynchronize(h.s));
    if (bad) { g_rtree_error = "an input element is not below the modulus"; return DST_ERR_ARG; }
    return DST_OK;
}

// selects the tree's device; its stream and events on the first call, and at least `bytes` of device staging (T: dst_rtree, dst_stree)
template <class T>
static int rtree_stage(const T* t, size_t bytes) {
    RT_HIP(t->err, hipSetDevice(t->device));
    if (!t->stream) RT_HIP(t->err, hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    if (!t->ev[0]) RT_HIP(t->err, hipEventCreate(&t->ev[0]));
    if (!t->ev[1]) RT_HIP(t->err, hipEventCreate(&t->ev[1]));
    if (bytes > t->stage_bytes) {
        if (t->stage) { hipFree(t->stage); t->stage = nullptr; t->stage_bytes = 0; }
        RT_HIP(t->err, hipMalloc((void**)&t->stage, bytes));
        t->stage_bytes = bytes;
    }
    return DST_OK;
}
// ev[0] .. ev[1] of the stream, which has been synchronised
template <class T>
static int rtree_elapsed(const T* t, double* ms) {
    float f = 0;
    RT_HIP(t->err, hipEventElapsedTime(&f, t->ev[0], t->ev[1]));
    *ms = f;
    return DST_OK;
}

static int rtree_build_device(dst_rtree* t, const uint8_t* leaves) {
    const size_t n = (size_t)1 << t->log_leaves;
    if (int r = rtree_stage(t, 4)) return r;                                                // the flag of a leaf element >= p
    uint32_t *d_bad = reinterpret_cast<uint32_t*>(t->stage), bad = 0;
    RT_HIP(t->err, hipMalloc((void**)&t->dev, 64 * n));
    RT_HIP(t->err, hipMemsetAsync(d_bad, 0, 4, t->stream));
    RT_HIP(t->err, hipMemsetAsync(t->dev, 0, 32, t->stream));                               // nodes[0] is not part of the tree
    RT_HIP(t->err, hipMemcpyAsync(t->dev + 2 * n, leaves, 32 * n, hipMemcpyHostToDevice, t->stream));
    RT_HIP(t->err, hipEventRecord(t->ev[0], t->stream));
    if (k_rescue_tree(t->stream, t->dev, n, d_bad)) return rt_fail(t, DST_ERR_HIP, "rescue_tree_level_kernel: launch failed");
    RT_HIP(t->err, hipEventRecord(t->ev[1], t->stream));
    RT_HIP(t->err, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, t->stream));
    RT_HIP(t->err, hipStreamSynchronize(t->stream));
    if (int r = rtree_elapsed(t, &t->device_ms)) return r;
    return bad ? rt_fail(t, DST_ERR_ARG, "a leaf element is not below the modulus") : DST_OK;
}
// the tree whose paths smpath / pmpath authenticate: parent = digest(l0, l1, r0, r1) (src/examples/merkle.rs:112-145)
int dst_rtree_build(int device, const uint8_t* leaves, uint32_t log_leaves, dst_rtree** out) {
    if (out) *out = nullptr;
    if (!leaves || !out || log_leaves < 1 || log_leaves > 26) { g_rtree_error = "invalid argument (1 <= log_leaves <= 26)"; return DST_ERR_ARG; }
    const size_t n = (size_t)1 << log_leaves;
    std::unique_ptr<dst_rtree> t(new (std::nothrow) dst_rtree);
    if (!t) { g_rtree_error = "out of host memory"; return DST_ERR_HIP; }
    t->device = device < 0 ? -1 : device; t->log_leaves = log_leaves;
    int r = DST_OK;
    if (device >= 0) r = rtree_build_device(t.get(), leaves);
    else if (!all_below_p(leaves, 2 * n)) r = rt_fail(t.get(), DST_ERR_ARG, "a leaf element is not below the modulus");
    else {
        try { t->host.assign(4 * n, 0); } catch (const std::bad_alloc&) { g_rtree_error = "out of host memory"; return DST_ERR_HIP; }
        memcpy(t->host.data() + 2 * n, leaves, 32 * n);
        rescue_tree_host(t->host.data(), n);
    }
    if (r != DST_OK) { g_rtree_error = t->err; return r; }
    *out = t.release();
    return DST_OK;
}
void dst_rtree_destroy(dst_rtree* t) { delete t; }
const char* dst_rtree_last_error(const dst_rtree* t) { return t ? t->err.c_str() : g_rtree_error.c_str(); }
int dst_rtree_build_ms(const dst_rtree* t, double* device_ms) {
    if (int r = rt_enter(t)) return r;
    if (!device_ms) return rt_fail(t, DST_ERR_ARG, "null pointer");
    *device_ms = t->device_ms;
    return DST_OK;
}
int dst_rtree_update_ms(const dst_rtree* t, double* device_ms) {
    if (int r = rt_enter(t)) return r;
    if (!device_ms) return rt_fail(t, DST_ERR_ARG, "null pointer");
    *device_ms = t->update_ms;
    return DST_OK;
}
int dst_rtree_read_nodes(const dst_rtree* t, uint64_t first, uint64_t count, uint8_t* out) {
    if (int r = rt_enter(t)) return r;
    if (!out && count) return rt_fail(t, DST_ERR_ARG, "null pointer");
    const uint64_t total = (uint64_t)2 << t->log_leaves;
    if (first > total || count > total - first) return rt_fail(t, DST_ERR_ARG, "node range past the end of the node array");
    if (count == 0) return DST_OK;
    if (t->device < 0) { memcpy(out, t->host.data() + 2 * first, 32 * count); return DST_OK; }
    RT_HIP(t->err, hipSetDevice(t->device));
    RT_HIP(t->err, hipMemcpy(out, t->dev + 2 * first, 32 * count, hipMemcpyDeviceToHost));
    return DST_OK;
}
int dst_rtree_root(const dst_rtree* t, uint8_t root[32]) {
    if (int r = rt_enter(t)) return r;
    if (!root) return rt_fail(t, DST_ERR_ARG, "null pointer");
    return dst_rtree_read_nodes(t, 1, 1, root);
}

// ---- updates in place ------------------------------------------------------------------------------------------------------------------
// the dirty parents of an update, in the form k_rescue_tree_update and rescue_tree_update_host take: level l (2^l parents, l < log_leaves)
// has cnt[l] of them, their node-array positions sorted at lists[off[l] ..); a level that is dirty as a whole (and so every level above it)
// has cnt[l] == 2^l and no list
struct rtree_dirty {
    std::vector<uint32_t> lists;
    size_t off[27] = {0}, cnt[27] = {0};
};
static rtree_dirty rtree_dirty_levels(std::vector<uint32_t> cur /* the leaf indices: sorted, distinct */, uint32_t log_leaves) {
    rtree_dirty d;
    for (uint32_t l = log_leaves; l-- > 0;) {                    // dirty parents of level l = unique(index >> (log_leaves - l))
        for (auto& v : cur) v >>= 1;
        cur.erase(std::unique(cur.begin(), cur.end()), cur.end());
        d.cnt[l] = cur.size();
        if (d.cnt[l] == ((size_t)1 << l)) continue;
        d.off[l] = d.lists.size();
        for (uint32_t v : cur) d.lists.push_back(((uint32_t)1 << l) + v);
    }
    return d;
}
// staging: the new leaves as given, their node positions, then the dirty lists -- `up`, one upload; nothing here allocates host memory
static int rtree_update_device(dst_rtree* t, const std::vector<uint8_t>& up, size_t count, const rtree_dirty& d) {
    if (int r = rtree_stage(t, up.size())) return r;
    const uint32_t* d_words = reinterpret_cast<const uint32_t*>(t->stage + 32 * count);
    RT_HIP(t->err, hipMemcpyAsync(t->stage, up.data(), up.size(), hipMemcpyHostToDevice, t->stream));
    if (k_rescue_tree_scatter(t->stream, t->dev, d_words, reinterpret_cast<const fe*>(t->stage), count)) return rt_fail(t, DST_ERR_HIP, "rescue_tree_scatter_kernel: launch failed");
    RT_HIP(t->err, hipEventRecord(t->ev[0], t->stream));
    if (k_rescue_tree_update(t->stream, t->dev, t->log_leaves, d_words + count, d.off, d.cnt)) return rt_fail(t, DST_ERR_HIP, "rescue_tree_update_kernel: launch failed");
    RT_HIP(t->err, hipEventRecord(t->ev[1], t->stream));
    RT_HIP(t->err, hipStreamSynchronize(t->stream));
    return rtree_elapsed(t, &t->update_ms);
}
// a tree is not frozen: replaces leaves and recomputes their ancestors, the nodes that src/examples/merkle.rs:98-145 would read on the
// way from any of these leaves to the root
int dst_rtree_update(dst_rtree* t, const uint64_t* indices, const uint8_t* leaves, size_t count) {
    if (int r = rt_enter(t)) return r;
    if (count == 0) return DST_OK;
    if (!indices || !leaves) return rt_fail(t, DST_ERR_ARG, "null pointer");
    const size_t n = (size_t)1 << t->log_leaves;
    if (count > n) return rt_fail(t, DST_ERR_ARG, "a leaf index is repeated");
    if (!all_leaf_indices(t, indices, count)) return rt_fail(t, DST_ERR_ARG, "leaf index past the end");
    try {
        // everything is checked and every host buffer allocated here, before the first node changes: O(count log count)
        std::vector<uint32_t> sorted(indices, indices + count);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return rt_fail(t, DST_ERR_ARG, "a leaf index is repeated");
        if (!all_below_p(leaves, 2 * count)) return rt_fail(t, DST_ERR_ARG, "a leaf element is not below the modulus");
        const rtree_dirty d = rtree_dirty_levels(std::move(sorted), t->log_leaves);
        if (t->device < 0) {
            std::vector<u128> scratch(6 * count);                  // no level has more dirty parents than there are new leaves
            for (size_t i = 0; i < count; i++) memcpy(t->host.data() + 2 * (n + indices[i]), leaves + 32 * i, 32);
            rescue_tree_update_host(t->host.data(), t->log_leaves, d.lists.data(), d.off, d.cnt, scratch.data());
            return DST_OK;
        }
        std::vector<uint32_t> where(count);
        for (size_t i = 0; i < count; i++) where[i] = (uint32_t)(n + indices[i]);
        std::vector<uint8_t> up(36 * count + 4 * d.lists.size());
        memcpy(up.data(), leaves, 32 * count);
        memcpy(up.data() + 32 * count, where.data(), 4 * count);
        memcpy(up.data() + 36 * count, d.lists.data(), 4 * d.lists.size());
        const int r = rtree_update_device(t, up, count, d);
        if (r != DST_OK) { t->broken = true; t->err += "; the update did not complete, the tree is unusable"; }
        return r;
    } catch (const std::bad_alloc&) { return rt_fail(t, DST_ERR_HIP, "out of host memory"); }      // thrown before anything was queued
}

// ---- openings --------------------------------------------------------------------------------------------------------------------------
// the paths of `count` leaves, (log_leaves + 1) nodes each -> out: on a device tree one upload of the positions, one gather launch, one copy back
static int rtree_paths(const dst_rtree* t, const uint64_t* indices, size_t count, uint8_t* out) {
    const size_t n = t->log_leaves + 1, m = count * n;
    if (count > ((size_t)1 << 40)) return rt_fail(t, DST_ERR_ARG, "too many indices");
    if (!all_leaf_indices(t, indices, count)) return rt_fail(t, DST_ERR_ARG, "leaf index past the end");
    if (count == 0) return DST_OK;
    uint64_t pos[27];
    if (t->device < 0) {
        for (size_t i = 0; i < count; i++) {
            rescue_path_positions(t->log_leaves, indices[i], pos);
            for (size_t k = 0; k < n; k++) memcpy(out + 32 * (i * n + k), t->host.data() + 2 * pos[k], 32);
        }
        return DST_OK;
    }
    try {
        std::vector<uint32_t> where(m);
        for (size_t i = 0; i < count; i++) {
            rescue_path_positions(t->log_leaves, indices[i], pos);
            for (size_t k = 0; k < n; k++) where[i * n + k] = (uint32_t)pos[k];
        }
        if (int r = rtree_stage(t, 36 * m)) return r;                 // [m nodes][m positions]
        uint32_t* d_where = reinterpret_cast<uint32_t*>(t->stage + 32 * m);
        RT_HIP(t->err, hipMemcpyAsync(d_where, where.data(), 4 * m, hipMemcpyHostToDevice, t->stream));
        if (k_rescue_tree_gather(t->stream, t->dev, d_where, reinterpret_cast<fe*>(t->stage), m)) return rt_fail(t, DST_ERR_HIP, "rescue_tree_gather_kernel: launch failed");
        RT_HIP(t->err, hipMemcpyAsync(out, t->stage, 32 * m, hipMemcpyDeviceToHost, t->stream));
        RT_HIP(t->err, hipStreamSynchronize(t->stream));
    } catch (const std::bad_alloc&) { return rt_fail(t, DST_ERR_HIP, "out of host memory"); }
    return DST_OK;
}
int dst_rtree_paths(const dst_rtree* t, const uint64_t* indices, size_t count, uint8_t* paths) {
    if (int r = rt_enter(t)) return r;
    if ((!indices || !paths) && count) return rt_fail(t, DST_ERR_ARG, "null pointer");
    return rtree_paths(t, indices, count, paths);
}
int dst_rtree_path(const dst_rtree* t, uint64_t index, uint8_t* path) {
    if (int r = rt_enter(t)) return r;
    if (!path) return rt_fail(t, DST_ERR_ARG, "null pointer");
    return rtree_paths(t, &index, 1, path);
}
// the tapes of `count` paths of n nodes each, `each` elements per tape and path (dense and sparse trees; K: uint64_t, or u128 for the wide ones)
template <class K>
static void tapes_from_paths(const u128* paths, size_t n, const K* indices, size_t count, uint32_t what, size_t each, uint8_t* tape_a, uint8_t* tape_b) {
    std::vector<u128> a, b;
    for (size_t i = 0; i < count; i++) {
        rescue_tapes(paths + 2 * n * i, n, indices[i], what, a, b);
        memcpy(tape_a + 16 * each * i, a.data(), 16 * each); memcpy(tape_b + 16 * each * i, b.data(), 16 * each);
    }
}
// generate_program_inputs (src/examples/merkle.rs:63-94) for `count` leaves; `size_name`: what the entry calls its size output
static int rtree_tapes(const dst_rtree* t, const uint64_t* indices, size_t count, uint32_t what, uint8_t* tape_a, uint8_t* tape_b, size_t cap_each, size_t* each_out,
                       const char* size_name) {
    if (int r = rt_enter(t)) return r;
    if (!each_out || what < 1 || what > 3) { t->err = std::string(size_name) + " missing, or what outside 1..3"; return DST_ERR_ARG; }
    if (!indices && count) return rt_fail(t, DST_ERR_ARG, "null pointer");
    const size_t n = t->log_leaves + 1;
    const size_t each = ((what & 1u) ? 2 * n - 1 : 0) + ((what & 2u) ? n - 1 : 0);
    *each_out = each;
    if (!tape_a && !tape_b)                                                                // size query
        return all_leaf_indices(t, indices, count) ? DST_OK : rt_fail(t, DST_ERR_ARG, "leaf index past the end");
    if (!tape_a || !tape_b || cap_each < each) return rt_fail(t, DST_ERR_ARG, "tape buffers missing or too small");
    try {
        std::vector<u128> paths(2 * n * count);
        if (int r = rtree_paths(t, indices, count, (uint8_t*)paths.data())) return r;
        tapes_from_paths(paths.data(), n, indices, count, what, each, tape_a, tape_b);
    } catch (const std::bad_alloc&) { return rt_fail(t, DST_ERR_HIP, "out of host memory"); }
    return DST_OK;
}
// generate_program_inputs over paths the caller holds (the witnesses of dst_rtree_apply / dst_stree_apply / dst_wtree_apply, or anyone's): no tree,
// no device.  K: uint64_t (n <= 64) or u128 (dst_rescue_path_tapes_w, n <= 128)
template <class K>
static int path_tapes(const uint8_t* paths, uint32_t n, const K* indices, size_t count, uint32_t what, uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each) {
    if (!elems_each || what < 1 || what > 3) { g_rtree_error = "elems_each missing, or what outside 1..3"; return DST_ERR_ARG; }
    if (n < 2 || n > 8 * sizeof(K)) { g_rtree_error = sizeof(K) == 8 ? "a path has 2 .. 64 nodes" : "a path has 2 .. 128 nodes"; return DST_ERR_ARG; }
    if (!indices && count) { g_rtree_error = "null pointer"; return DST_ERR_ARG; }
    if (count > ((size_t)1 << 40)) { g_rtree_error = "too many indices"; return DST_ERR_ARG; }
    const size_t each = ((what & 1u) ? 2 * (size_t)n - 1 : 0) + ((what & 2u) ? (size_t)n - 1 : 0);
    *elems_each = each;
    for (size_t i = 0; i < count; i++) if (indices[i] >> (n - 1)) { g_rtree_error = "leaf index past the end"; return DST_ERR_ARG; }
    if (!tape_a && !tape_b) return DST_OK;                                                 // size query
    if (!tape_a || !tape_b || cap_elems_each < each) { g_rtree_error = "tape buffers missing or too small"; return DST_ERR_ARG; }
    if (count == 0) return DST_OK;
    if (!paths) { g_rtree_error = "null pointer"; return DST_ERR_ARG; }
    if (!all_below_p(paths, 2 * (size_t)n * count)) { g_rtree_error = "a path element is not below the modulus"; return DST_ERR_ARG; }
    try {
        std::vector<u128> v(2 * (size_t)n * count);                                        // the caller's buffer needs only byte alignment
        memcpy(v.data(), paths, 32 * (size_t)n * count);
        tapes_from_paths(v.data(), n, indices, count, what, each, tape_a, tape_b);
    } catch (const std::bad_alloc&) { g_rtree_error = "out of host memory"; return DST_ERR_HIP; }
    return DST_OK;
}
int dst_rescue_path_tapes(const uint8_t* paths, uint32_t n, const uint64_t* indices, size_t count, uint32_t what, uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each) {
    return path_tapes(paths, n, indices, count, what, tape_a, tape_b, cap_elems_each, elems_each);
}
int dst_rtree_tapes(const dst_rtree* t, uint64_t index, uint32_t what, uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems, size_t* elems) {
    return rtree_tapes(t, &index, 1, what, tape_a, tape_b, cap_elems, elems, "elems");
}
int dst_rtree_tapes_many(const dst_rtree* t, const uint64_t* indices, size_t count, uint32_t what, uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each) {
    return rtree_tapes(t, indices, count, what, tape_a, tape_b, cap_elems_each, elems_each, "elems_each");
}

// ---- ordered writes (tree_sequence.h) --------------------------------------------------------------------------------------------------
// the level launches of an apply on a device tree (T: dst_rtree, dst_stree): `nodes` is the tree before the call, `empties` a sparse tree's E_l
// (nullptr: dense), spos the node-array positions of p's touched nodes when their last versions are to be written into `nodes` (dense), empty
// otherwise.  Staging: [the leaves = the versions of level D][indices][source words][spos][the touched nodes' last operations] -- one upload --
// [the versions of level D - 1]: the levels take the two version areas by turns; then [paths].  The last versions of level l + 1 go into the node
// array behind the launch of level l, which reads that level's nodes as they were.  One synchronisation; ms: events around the launches.
// The level kernel reads bit k - 1 of a 64-bit index word.  16-byte indices (Key = u128, the wide sparse trees) are staged as two arrays, all
// low halves and then all high halves; the launches of path nodes k > 64 get the high halves, k - 64, and the paths moved up by 64 nodes, which
// is the same bit, the same sibling and the same slot of the path.
template <class T, class Key>
static int tseq_run_device(const T* t, fe* nodes, const u128* empties, const tseq_plan_t<Key>& p, const std::vector<uint32_t>& spos, const Key* indices, const uint8_t* leaves,
                           uint8_t* paths, uint8_t* roots, double* ms) {
    const size_t K = p.count, D = p.depth, n = D + 1, S = spos.size(), W = sizeof(Key) / 8;
    const size_t o_idx = 32 * K, o_src = o_idx + 8 * W * K, o_pos = o_src + 4 * K * n, o_from = o_pos + 4 * S, up_bytes = o_from + 4 * S;
    const size_t o_other = (up_bytes + 15) & ~(size_t)15, o_paths = o_other + 32 * K, total = o_paths + (paths ? 32 * K * n : 0);
    std::vector<uint8_t> up(up_bytes);                                // the last host allocation: nothing is queued yet
    memcpy(up.data(), leaves, 32 * K);
    for (size_t w = 0; w < W; w++)
        for (size_t i = 0; i < K; i++) { const uint64_t half = (uint64_t)(indices[i] >> (32 * w) >> (32 * w)); memcpy(up.data() + o_idx + 8 * (w * K + i), &half, 8); }
    memcpy(up.data() + o_src, p.src.data(), 4 * K * n);
    if (S) { memcpy(up.data() + o_pos, spos.data(), 4 * S); memcpy(up.data() + o_from, p.tlast.data(), 4 * S); }
    if (int r = rtree_stage(t, total)) return r;
    uint8_t* st = t->stage;
    fe* const ver[2] = {reinterpret_cast<fe*>(st), reinterpret_cast<fe*>(st + o_other)};             // level l: ver[(D - l) & 1]
    const uint64_t* d_idx = reinterpret_cast<const uint64_t*>(st + o_idx);
    const uint32_t *d_src = reinterpret_cast<const uint32_t*>(st + o_src), *d_pos = reinterpret_cast<const uint32_t*>(st + o_pos), *d_from = reinterpret_cast<const uint32_t*>(st + o_from);
    fe* d_paths = paths ? reinterpret_cast<fe*>(st + o_paths) : nullptr;
    static const u128 none[2] = {0, 0};
    auto scatter = [&](size_t l) {                                     // level l's last versions -> nodes
        return S && k_rescue_tree_scatter_from(t->stream, nodes, d_pos + p.toff[l], ver[(D - l) & 1], d_from + p.toff[l], p.tcnt[l]);
    };
    RT_HIP(t->err, hipMemcpyAsync(st, up.data(), up_bytes, hipMemcpyHostToDevice, t->stream));
    RT_HIP(t->err, hipEventRecord(t->ev[0], t->stream));
    for (size_t l = D; l-- > 0;) {
        const uint32_t k = (uint32_t)(D - l), high = k > 64 ? 64u : 0u;
        if (k_rescue_seq_level(t->stream, nodes, ver[(k - 1) & 1], ver[k & 1], d_src + k * K, k == 1 ? d_src : nullptr, d_idx + (high ? K : 0), d_paths ? d_paths + 2 * high : nullptr, K, k - high,
                               (uint32_t)n,
                               reinterpret_cast<const fe*>(empties ? empties + 2 * (l + 1) : none))) { t->err = "rescue_seq_level_kernel: launch failed"; return DST_ERR_HIP; }
        if (scatter(l + 1)) { t->err = "rescue_tree_scatter_from_kernel: launch failed"; return DST_ERR_HIP; }
    }
    if (scatter(0)) { t->err = "rescue_tree_scatter_from_kernel: launch failed"; return DST_ERR_HIP; }
    RT_HIP(t->err, hipEventRecord(t->ev[1], t->stream));
    if (paths) RT_HIP(t->err, hipMemcpyAsync(paths, d_paths, 32 * K * n, hipMemcpyDeviceToHost, t->stream));
    if (roots) RT_HIP(t->err, hipMemcpyAsync(roots, ver[D & 1], 32 * K, hipMemcpyDeviceToHost, t->stream));
    RT_HIP(t->err, hipStreamSynchronize(t->stream));
    return rtree_elapsed(t, ms);
}
// operations (indices[i], leaves[i]) applied in order, indices may repeat: paths[i] opens indices[i] in the tree as operations 0 .. i-1 left it,
// roots[i] is the root after operation i; afterwards the tree is the one built from the final leaves
int dst_rtree_apply(dst_rtree* t, const uint64_t* indices, const uint8_t* leaves, size_t count, uint8_t* paths, uint8_t* roots) {
    if (int r = rt_enter(t)) return r;
    if (count == 0) return DST_OK;
    if (!indices || !leaves) return rt_fail(t, DST_ERR_ARG, "null pointer");
    if (count >= ((size_t)1 << 31)) return rt_fail(t, DST_ERR_ARG, "2^31 operations or more");
    if (!all_leaf_indices(t, indices, count)) return rt_fail(t, DST_ERR_ARG, "leaf index past the end");
    if (!all_below_p(leaves, 2 * count)) return rt_fail(t, DST_ERR_ARG, "a leaf element is not below the modulus");
    const size_t n = t->log_leaves + 1;
    if (t->device < 0) {                                               // one after the other: open, update, root
        for (size_t i = 0; i < count; i++) {
            if (paths) { if (int r = rtree_paths(t, indices + i, 1, paths + 32 * n * i)) return r; }
            if (int r = dst_rtree_update(t, indices + i, leaves + 32 * i, 1)) return r;
            if (roots) memcpy(roots + 32 * i, t->host.data() + 2, 32);
        }
        return DST_OK;
    }
    try {
        const tseq_plan p = tseq_plan_make(t->log_leaves, indices, count, [](uint32_t l, uint64_t q) { return (uint32_t)(((uint64_t)1 << l) + q); });
        std::vector<uint32_t> spos(p.touched());
        for (uint32_t l = 0; l <= t->log_leaves; l++)
            for (size_t j = p.toff[l]; j < p.toff[l] + p.tcnt[l]; j++) spos[j] = (uint32_t)(((uint64_t)1 << l) + p.tpref[j]);
        const int r = tseq_run_device(t, t->dev, nullptr, p, spos, indices, leaves, paths, roots, &t->update_ms);
        if (r != DST_OK) { t->broken = true; t->err += "; the sequence did not complete, the tree is unusable"; }
        return r;
    } catch (const std::bad_alloc&) { return rt_fail(t, DST_ERR_HIP, "out of host memory"); }      // thrown before anything was queued
}

// ---- save, load, audit (tree_blob.h has the saved form and the parser of untrusted bytes) ------------------------------------------------------
// the saved tree: the header and the nodes of heap positions 1 and up, as dst_rtree_read_nodes returns them
int dst_rtree_save(const dst_rtree* t, uint8_t* out, size_t cap, size_t* len) {
    if (int r = rt_enter(t)) return r;
    if (!len) return rt_fail(t, DST_ERR_ARG, "null pointer");
    const uint64_t nodes = ((uint64_t)2 << t->log_leaves) - 1;
    *len = (size_t)tblob_dense_bytes(t->log_leaves);
    if (!out) return DST_OK;                                                                // size query
    if (cap < *len) return rt_fail(t, DST_ERR_ARG, "the buffer is smaller than the saved tree");
    tblob_put_header(out, TBLOB_DENSE, t->log_leaves, nullptr, (uint64_t)1 << t->log_leaves, nodes);
    return dst_rtree_read_nodes(t, 1, nodes, out + TBLOB_HEADER);
}
// the first parent in [1, leaves) that is not the digest of its children: *key = its heap position, all ones when there is none
static int rtree_audit_run(const dst_rtree* t, uint64_t* key, double* ms) {
    const size_t n = (size_t)1 << t->log_leaves;
    *key = ~(uint64_t)0; *ms = 0;
    if (t->device < 0) {
        const size_t chunk = 1024;                                                          // ascending positions: the first chunk with a bad parent ends the walk
        std::vector<u128> d(2 * std::min(chunk, n));
        for (size_t p = 1; p < n; p += chunk) {
            const size_t m = std::min(chunk, n - p);
            rescue_digest_many_host(t->host.data() + 4 * p, m, d.data());                   // the children of p are the nodes 2p, 2p + 1: four elements at 4p
            for (size_t i = 0; i < m; i++) if (memcmp(&d[2 * i], &t->host[2 * (p + i)], 32) != 0) { *key = p + i; return DST_OK; }
        }
        return DST_OK;
    }
    if (int r = rtree_stage(t, 8)) return r;
    unsigned long long* d_key = reinterpret_cast<unsigned long long*>(t->stage);
    RT_HIP(t->err, hipMemsetAsync(d_key, 0xFF, 8, t->stream));
    RT_HIP(t->err, hipEventRecord(t->ev[0], t->stream));
    if (k_rescue_tree_audit(t->stream, t->dev, n, d_key)) return rt_fail(t, DST_ERR_HIP, "rescue_tree_audit_kernel: launch failed");
    RT_HIP(t->err, hipEventRecord(t->ev[1], t->stream));
    RT_HIP(t->err, hipMemcpyAsync(key, d_key, 8, hipMemcpyDeviceToHost, t->stream));
    RT_HIP(t->err, hipStreamSynchronize(t->stream));
    return rtree_elapsed(t, ms);
}
// the tree is only read: an error here leaves it usable
int dst_rtree_audit(const dst_rtree* t, int64_t* first_bad, double* device_ms) {
    if (int r = rt_enter(t)) return r;
    if (!first_bad) return rt_fail(t, DST_ERR_ARG, "null pointer");
    uint64_t key = 0;
    double ms = 0;
    try {
        if (int r = rtree_audit_run(t, &key, &ms)) return r;
    } catch (const std::bad_alloc&) { return rt_fail(t, DST_ERR_HIP, "out of host memory"); }
    *first_bad = key == ~(uint64_t)0 ? -1 : (int64_t)key;
    if (device_ms) *device_ms = ms;
    return DST_OK;
}
// a tree from its saved form: nothing is hashed -- one allocation, one upload -- unless the caller asks for the audit
int dst_rtree_load(int device, const uint8_t* blob, size_t len, uint32_t audit, dst_rtree** out) {
    if (out) *out = nullptr;
    if (!blob || !out) { g_rtree_error = "null pointer"; return DST_ERR_ARG; }
    tblob_view v;
    if (const char* why = tblob_parse(blob, len, TBLOB_DENSE, v)) { g_rtree_error = why; return DST_ERR_ARG; }
    std::unique_ptr<dst_rtree> t(new (std::nothrow) dst_rtree);
    if (!t) { g_rtree_error = "out of host memory"; return DST_ERR_HIP; }
    t->device = device < 0 ? -1 : device; t->log_leaves = v.depth;
    const size_t n = (size_t)1 << v.depth;
    auto upload = [&]() -> int {
        if (int r = rtree_stage(t.get(), 0)) return r;
        RT_HIP(t->err, hipMalloc((void**)&t->dev, 64 * n));
        RT_HIP(t->err, hipMemsetAsync(t->dev, 0, 32, t->stream));                           // nodes[0] is not part of the tree
        RT_HIP(t->err, hipMemcpyAsync(t->dev + 2, v.values, 32 * (2 * n - 1), hipMemcpyHostToDevice, t->stream));
        RT_HIP(t->err, hipStreamSynchronize(t->stream));
        return DST_OK;
    };
    try {
        if (device >= 0) { if (int r = upload()) { g_rtree_error = t->err; return r; } }
        else { t->host.assign(4 * n, 0); memcpy(t->host.data() + 2, v.values, 32 * (2 * n - 1)); }
        if (audit) {
            uint64_t key = 0;
            double ms = 0;
            if (int r = rtree_audit_run(t.get(), &key, &ms)) { g_rtree_error = t->err; return r; }
            if (key != ~(uint64_t)0) { g_rtree_error = "audit: node " + std::to_string(key) + " is not the digest of its children"; return DST_ERR_ARG; }
        }
    } catch (const std::bad_alloc&) { g_rtree_error = "out of host memory"; return DST_ERR_HIP; }
    *out = t.release();
    return DST_OK;
}
