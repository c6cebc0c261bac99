// Sparse Rescue Merkle trees behind dst_stree_* (8-byte keys, depth <= 63) and dst_wtree_* (16-byte keys, depth <= 127): the dense tree of rtree_impl.h over 2^depth leaves in which every leaf that was never set holds
// the tree's empty leaf, stored as the nodes with a set leaf below them only (host/stree_levels.h has the layout and the plans of a set and of
// a removal; the kernels are in kernels_hash.hip).  Included by api.hip after rtree_impl.h, whose stream / staging / error helpers it shares.
#pragma once
#include "rtree_impl.h"
#include "stree_levels.h"

// what the two key widths share: everything but the shape, the E_l and the layout of a device generation
struct stree_base {
    int device = -1;                      // < 0: the nodes live in `host`
    uint32_t depth = 0;
    std::vector<u128> host;               // the node values at the shape's flat positions, 2 elements per node
    uint8_t* dev = nullptr;               // one allocation per generation (stree_of)
    uint64_t last_digests = 0;
    double last_ms = 0;                   // events around the level launches of the last set / remove / compact
    bool broken = false;                  // a HIP error inside a call that changes the tree: only destroy / last_error remain
    mutable hipStream_t stream = nullptr;
    mutable hipEvent_t ev[2] = {nullptr, nullptr};
    mutable uint8_t* stage = nullptr; mutable size_t stage_bytes = 0;
    mutable std::string err;
    ~stree_base() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (dev) hipFree(dev);
        if (stage) hipFree(stage);
        for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
        if (stream) hipStreamDestroy(stream);
    }
};
// K = the key on the host: uint64_t (dst_stree, depth <= 63) or u128 (dst_wtree, depth <= 127); dev_key = the same bytes as the kernels read them.
// A device generation is [nodes 32 * total][empties 32 * L][levels 16 * L][prefixes sizeof(K) * total] with L = 8 * sizeof(K) levels at the most:
//   dst_stree  [nodes 32 * total][empties 32 * 64 ][levels 16 * 64 ][prefixes  8 * total]     40 * total + 3072 bytes
//   dst_wtree  [nodes 32 * total][empties 32 * 128][levels 16 * 128][prefixes 16 * total]     48 * total + 6144 bytes, the prefixes 16-byte aligned
template <class K, class DevKey> struct stree_of : stree_base {
    typedef K key;
    typedef DevKey dev_key;
    static_assert(sizeof(K) == sizeof(DevKey), "the device reads the host's keys as they are");
    static constexpr uint32_t max_depth = stree_max_depth<K>();
    static constexpr size_t L = max_depth + 1, empties_bytes = 32 * L, levels_bytes = 16 * L, head_bytes = empties_bytes + levels_bytes;
    static size_t generation_bytes(size_t total) { return (32 + sizeof(K)) * total + head_bytes; }
    u128 empties[2 * L] = {0};            // E_l, the value of an empty subtree of level l, at empties[2 l ..); E_depth = the empty leaf
    stree_shape_t<K> shape;               // every level's prefixes; of a device tree too: sets are planned on the host
    fe* dev_nodes() const { return reinterpret_cast<fe*>(dev); }
    fe* dev_empties() const { return reinterpret_cast<fe*>(dev + 32 * shape.total()); }
    uint64_t* dev_levels() const { return reinterpret_cast<uint64_t*>(dev + 32 * shape.total() + empties_bytes); }
    DevKey* dev_pref() const { return reinterpret_cast<DevKey*>(dev + 32 * shape.total() + head_bytes); }
};
struct dst_stree : stree_of<uint64_t, uint64_t> {
    static std::string& global_error() { static thread_local std::string e; return e; }      // dst_stree_last_error(NULL)
    static const char* depth_rule() { return "invalid argument (1 <= depth <= 63)"; }
};
struct dst_wtree : stree_of<u128, stree_wide> {
    static std::string& global_error() { static thread_local std::string e; return e; }      // dst_wtree_last_error(NULL)
    static const char* depth_rule() { return "invalid argument (1 <= depth <= 127)"; }
};
static int st_enter(const stree_base* t) { return !t ? DST_ERR_ARG : t->broken ? DST_ERR_STATE : DST_OK; }
static int st_fail(const stree_base* t, int code, const char* why) { t->err = why; return code; }
template <class T> static bool all_keys(const T* t, const typename T::key* indices, size_t count) {
    for (size_t i = 0; i < count; i++) if (indices[i] >> t->depth) return false;
    return true;
}
template <class T> static const typename T::dev_key* dev_keys(const typename T::key* k) { return reinterpret_cast<const typename T::dev_key*>(k); }
struct st_generation {                                 // a device allocation that is freed unless the plan completes
    uint8_t* p = nullptr;
    ~st_generation() { if (p) hipFree(p); }
};

// the plan on the device: the next generation's allocation, the uploads (prefixes and level table into the generation; new leaves, carry-over
// sources and dirty lists into the staging buffer), one carry-over launch, one scatter of the new leaves if there are any (a removal has none),
// one launch per level that has dirty parents, one synchronisation.  A generation without nodes (creation, the last key removed) launches nothing.
template <class T>
static int stree_apply_device(T* t, const stree_plan_t<typename T::key>& p, const uint8_t* leaves /* in the order of the sorted keys */, size_t count) {
    typedef typename T::key K;
    const stree_shape_t<K>& nx = p.next;
    const size_t total = nx.total(), D = t->depth;
    if (int r = rtree_stage(t, 32 * count + 4 * total + 4 * p.dirty.size() + 16)) return r;
    st_generation g;
    RT_HIP(t->err, hipMalloc((void**)&g.p, T::generation_bytes(total)));
    fe* nodes = reinterpret_cast<fe*>(g.p);
    uint64_t* levels = reinterpret_cast<uint64_t*>(g.p + 32 * total + T::empties_bytes);
    typename T::dev_key* pref = reinterpret_cast<typename T::dev_key*>(g.p + 32 * total + T::head_bytes);
    uint64_t lv[2 * T::L] = {0};
    for (size_t l = 0; l <= D; l++) { lv[2 * l] = nx.start[l]; lv[2 * l + 1] = nx.cnt[l]; }
    const fe* d_leaves = reinterpret_cast<const fe*>(t->stage);
    uint32_t *d_src = reinterpret_cast<uint32_t*>(t->stage + 32 * count), *d_dirty = d_src + total;
    RT_HIP(t->err, hipMemcpyAsync(g.p + 32 * total, t->empties, T::empties_bytes, hipMemcpyHostToDevice, t->stream));
    RT_HIP(t->err, hipMemcpyAsync(levels, lv, T::levels_bytes, hipMemcpyHostToDevice, t->stream));
    if (total) {
        RT_HIP(t->err, hipMemcpyAsync(pref, nx.pref.data(), sizeof(K) * total, hipMemcpyHostToDevice, t->stream));
        RT_HIP(t->err, hipMemcpyAsync(d_src, p.src.data(), 4 * total, hipMemcpyHostToDevice, t->stream));
    }
    if (count) RT_HIP(t->err, hipMemcpyAsync(t->stage, leaves, 32 * count, hipMemcpyHostToDevice, t->stream));
    if (!p.dirty.empty()) RT_HIP(t->err, hipMemcpyAsync(d_dirty, p.dirty.data(), 4 * p.dirty.size(), hipMemcpyHostToDevice, t->stream));
    if (total && k_rescue_stree_carry(t->stream, nodes, t->dev_nodes(), d_src, total)) return st_fail(t, DST_ERR_HIP, "rescue_stree_carry_kernel: launch failed");
    if (count && k_rescue_tree_scatter(t->stream, nodes, d_dirty + p.doff[D], d_leaves, count)) return st_fail(t, DST_ERR_HIP, "rescue_tree_scatter_kernel: launch failed");
    RT_HIP(t->err, hipEventRecord(t->ev[0], t->stream));
    for (size_t l = D; l-- > 0;) {
        if (p.dcnt[l] == 0) continue;
        const bool whole = p.dcnt[l] == nx.cnt[l];
        if (k_rescue_stree_level(t->stream, nodes, pref, whole ? nullptr : d_dirty + p.doff[l], p.dcnt[l], nx.start[l], nx.start[l + 1], nx.cnt[l + 1],
                                 reinterpret_cast<const fe*>(t->empties + 2 * (l + 1))))
            return st_fail(t, DST_ERR_HIP, "rescue_stree_level_kernel: launch failed");
    }
    RT_HIP(t->err, hipEventRecord(t->ev[1], t->stream));
    RT_HIP(t->err, hipStreamSynchronize(t->stream));
    if (int r = rtree_elapsed(t, &t->last_ms)) return r;
    if (t->dev) hipFree(t->dev);
    t->dev = g.p; g.p = nullptr;
    return DST_OK;
}
// ... and on the host: the same carry-over, the same lookups, rescue_digest_many_host over each level's dirty list
template <class T>
static void stree_apply_host(T* t, const stree_plan_t<typename T::key>& p, const uint8_t* leaves, size_t count) {
    const stree_shape_t<typename T::key>& nx = p.next;
    const size_t D = t->depth;
    size_t most = 0;                                                               // the longest dirty list of parents
    for (size_t l = 0; l < D; l++) most = std::max(most, p.dcnt[l]);
    std::vector<u128> nn(2 * nx.total()), in(4 * most), out(2 * most);
    for (size_t j = 0; j < nx.total(); j++) if (p.src[j] != STREE_NEW) memcpy(&nn[2 * j], &t->host[2 * (size_t)p.src[j]], 32);
    for (size_t i = 0; i < count; i++) memcpy(&nn[2 * (size_t)p.dirty[p.doff[D] + i]], leaves + 32 * i, 32);
    for (size_t l = D; l-- > 0;) {
        const uint32_t* list = p.dirty.data() + p.doff[l];
        const size_t m = p.dcnt[l], cstart = nx.start[l + 1];
        const u128* e = t->empties + 2 * (l + 1);
        if (m == 0) continue;
        for (size_t g = 0; g < m; g++) {
            size_t left, right;
            stree_children(nx.pref.data() + cstart, nx.cnt[l + 1], nx.pref[list[g]], left, right);
            memcpy(&in[4 * g], left != STREE_ABSENT ? &nn[2 * (cstart + left)] : e, 32);
            memcpy(&in[4 * g + 2], right != STREE_ABSENT ? &nn[2 * (cstart + right)] : e, 32);
        }
        rescue_digest_many_host(in.data(), m, out.data());
        for (size_t g = 0; g < m; g++) memcpy(&nn[2 * (size_t)list[g]], &out[2 * g], 32);
    }
    t->host.swap(nn);
}
// how set, remove and compact change a tree: the plan runs where the tree lives, then the tree takes the plan's shape.  Everything that can be
// refused has been refused before; a HIP error here leaves neither generation whole
template <class T>
static int stree_commit(T* t, stree_plan_t<typename T::key>& p, const uint8_t* leaves, size_t count, const char* what) {
    if (t->device < 0) stree_apply_host(t, p, leaves, count);
    else if (int r = stree_apply_device(t, p, leaves, count)) {
        t->broken = true; t->err += std::string("; the ") + what + " did not complete, the tree is unusable";
        return r;
    }
    t->shape = std::move(p.next);
    t->last_digests = p.digests;
    return DST_OK;
}
// `count` indices below 2^depth, sorted; false when one is repeated (the whole key is compared)
template <class K>
static bool sorted_distinct(const K* indices, size_t count, std::vector<K>& keys) {
    keys.assign(indices, indices + count);
    std::sort(keys.begin(), keys.end());
    return std::adjacent_find(keys.begin(), keys.end()) == keys.end();
}

// ---- the calls, each stated once for T = dst_stree and T = dst_wtree; the entry points of the C-ABI follow at the end ------------------------------
template <class T>
static int stree_create(int device, uint32_t depth, const uint8_t empty_leaf[32], T** out) {
    std::string& g_error = T::global_error();
    if (out) *out = nullptr;
    if (!out || depth < 1 || depth > T::max_depth) { g_error = T::depth_rule(); return DST_ERR_ARG; }
    if (empty_leaf && !all_below_p(empty_leaf, 2)) { g_error = "an element of the empty leaf is not below the modulus"; return DST_ERR_ARG; }
    std::unique_ptr<T> t(new (std::nothrow) T);
    if (!t) { g_error = "out of host memory"; return DST_ERR_HIP; }
    t->device = device < 0 ? -1 : device; t->depth = depth; t->shape.depth = depth;
    if (empty_leaf) memcpy(t->empties + 2 * depth, empty_leaf, 32);
    for (uint32_t l = depth; l-- > 0;) {                                           // E_l = digest(E_{l+1}, E_{l+1})
        const u128 in[4] = {t->empties[2 * l + 2], t->empties[2 * l + 3], t->empties[2 * l + 2], t->empties[2 * l + 3]};
        rescue_digest_many_host(in, 1, t->empties + 2 * l);
    }
    if (device >= 0) {                                                             // the generation of a tree without keys
        const int r = stree_apply_device(t.get(), stree_plan_set(t->shape, {}), nullptr, 0);
        if (r != DST_OK) { g_error = t->err; return r; }
        t->last_ms = 0;                                                            // nothing was launched
    }
    *out = t.release();
    return DST_OK;
}

template <class T>
static int stree_set(T* t, const typename T::key* indices, const uint8_t* leaves, size_t count) {
    typedef typename T::key K;
    if (int r = st_enter(t)) return r;
    if (count == 0) { t->last_digests = 0; t->last_ms = 0; return DST_OK; }
    if (!indices || !leaves) return st_fail(t, DST_ERR_ARG, "null pointer");
    if (count >= STREE_NEW || t->shape.total() + count * (t->depth + 1) >= STREE_NEW) return st_fail(t, DST_ERR_ARG, "more than 2^32 - 1 stored nodes");
    if (!all_keys(t, indices, count)) return st_fail(t, DST_ERR_ARG, "index past the end");
    try {
        // everything is checked and the whole plan made here, before anything is queued or a node changes
        std::vector<uint32_t> order(count);
        for (size_t i = 0; i < count; i++) order[i] = (uint32_t)i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return indices[a] < indices[b]; });
        std::vector<K> keys(count);
        for (size_t i = 0; i < count; i++) keys[i] = indices[order[i]];
        if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return st_fail(t, DST_ERR_ARG, "an index is repeated");
        if (!all_below_p(leaves, 2 * count)) return st_fail(t, DST_ERR_ARG, "a leaf element is not below the modulus");
        std::vector<uint8_t> sorted(32 * count);
        for (size_t i = 0; i < count; i++) memcpy(&sorted[32 * i], leaves + 32 * (size_t)order[i], 32);
        stree_plan_t<K> p = stree_plan_set(t->shape, std::move(keys));
        return stree_commit(t, p, sorted.data(), count, "set");
    } catch (const std::bad_alloc&) { return st_fail(t, DST_ERR_HIP, "out of host memory"); }      // thrown before anything was queued
}

// ---- deletion: the stored keys among the indices leave, and every node left without a key below it; what remains is the fresh tree of the
//      remaining keys.  The surviving ancestors of the removed keys are hashed again (stree_plan_remove), nothing else ------------------------
template <class T>
static int stree_remove(T* t, const typename T::key* indices, size_t count, uint64_t* removed) {
    typedef typename T::key K;
    if (int r = st_enter(t)) return r;
    if (!indices && count) return st_fail(t, DST_ERR_ARG, "null pointer");
    if (!all_keys(t, indices, count)) return st_fail(t, DST_ERR_ARG, "index past the end");
    try {
        std::vector<K> keys;
        if (!sorted_distinct(indices, count, keys)) return st_fail(t, DST_ERR_ARG, "an index is repeated");
        const size_t D = t->depth;
        const K* leaf_pref = t->shape.pref.data() + t->shape.start[D];
        const size_t leaf_cnt = t->shape.cnt[D];
        size_t at = 0;                                                             // the keys ascend: one walk along the leaf level
        keys.erase(std::remove_if(keys.begin(), keys.end(), [&](K k) { at = stree_advance(leaf_pref, leaf_cnt, at, k); return at == leaf_cnt || leaf_pref[at] != k; }), keys.end());
        if (removed) *removed = keys.size();
        if (keys.empty()) { t->last_digests = 0; t->last_ms = 0; return DST_OK; }
        stree_plan_t<K> p = stree_plan_remove(t->shape, std::move(keys));
        return stree_commit(t, p, nullptr, 0, "removal");
    } catch (const std::bad_alloc&) { return st_fail(t, DST_ERR_HIP, "out of host memory"); }
}
// the stored keys that hold the empty leaf leave: their ancestors are what they were (a stored empty side and an absent side hash alike), so
// nothing is hashed.  A device tree flags those leaves in one launch and sends a byte per stored key back; node values stay where they are
template <class T>
static int stree_compact(T* t, uint64_t* removed) {
    typedef typename T::key K;
    if (int r = st_enter(t)) return r;
    const size_t D = t->depth, m = t->shape.cnt[D], lstart = t->shape.start[D];
    try {
        std::vector<uint8_t> flags(m);
        if (t->device < 0) {
            for (size_t i = 0; i < m; i++) flags[i] = memcmp(&t->host[2 * (lstart + i)], t->empties + 2 * D, 32) == 0;
        } else if (m) {                                                            // the tree is only read: an error here leaves it usable
            if (int r = rtree_stage(t, m)) return r;
            if (k_rescue_stree_empty_leaves(t->stream, t->dev_nodes() + 2 * lstart, reinterpret_cast<const fe*>(t->empties + 2 * D), t->stage, m))
                return st_fail(t, DST_ERR_HIP, "rescue_stree_empty_leaves_kernel: launch failed");
            RT_HIP(t->err, hipMemcpyAsync(flags.data(), t->stage, m, hipMemcpyDeviceToHost, t->stream));
            RT_HIP(t->err, hipStreamSynchronize(t->stream));
        }
        std::vector<K> keys;
        for (size_t i = 0; i < m; i++) if (flags[i]) keys.push_back(t->shape.pref[lstart + i]);
        if (removed) *removed = keys.size();
        if (keys.empty()) { t->last_digests = 0; t->last_ms = 0; return DST_OK; }
        stree_plan_t<K> p = stree_plan_remove(t->shape, std::move(keys), false);
        return stree_commit(t, p, nullptr, 0, "compaction");
    } catch (const std::bad_alloc&) { return st_fail(t, DST_ERR_HIP, "out of host memory"); }
}
// the leaves alone, 32 bytes per index where a path is 32 * (depth + 1)
template <class T>
static int stree_get(const T* t, const typename T::key* indices, size_t count, uint8_t* leaves, uint8_t* stored) {
    typedef typename T::key K;
    if (int r = st_enter(t)) return r;
    if ((!indices || !leaves) && count) return st_fail(t, DST_ERR_ARG, "null pointer");
    if (count > ((size_t)1 << 40)) return st_fail(t, DST_ERR_ARG, "too many indices");
    if (!all_keys(t, indices, count)) return st_fail(t, DST_ERR_ARG, "index past the end");
    if (count == 0) return DST_OK;
    const size_t D = t->depth, m = t->shape.cnt[D], lstart = t->shape.start[D];
    if (t->device < 0) {
        for (size_t i = 0; i < count; i++) {
            const size_t pos = stree_find(t->shape.pref.data() + lstart, m, indices[i]);
            memcpy(leaves + 32 * i, pos != STREE_ABSENT ? &t->host[2 * (lstart + pos)] : t->empties + 2 * D, 32);
            if (stored) stored[i] = pos != STREE_ABSENT;
        }
        return DST_OK;
    }
    try {
        std::vector<uint8_t> back(stored ? 33 * count : 0);                        // one copy back: [count leaves][count flags]
        if (int r = rtree_stage(t, (33 + sizeof(K)) * count + sizeof(K))) return r;      // [count leaves][count flags, padded to a key][count indices]
        uint8_t* d_stored = t->stage + 32 * count;
        typename T::dev_key* d_idx = reinterpret_cast<typename T::dev_key*>(t->stage + 32 * count + ((count + sizeof(K) - 1) & ~(sizeof(K) - 1)));
        RT_HIP(t->err, hipMemcpyAsync(d_idx, indices, sizeof(K) * count, hipMemcpyHostToDevice, t->stream));
        if (k_rescue_stree_get(t->stream, t->dev_nodes(), t->dev_pref(), lstart, m, reinterpret_cast<const fe*>(t->empties + 2 * D), d_idx, reinterpret_cast<fe*>(t->stage), d_stored, count))
            return st_fail(t, DST_ERR_HIP, "rescue_stree_get_kernel: launch failed");
        RT_HIP(t->err, hipMemcpyAsync(stored ? back.data() : leaves, t->stage, stored ? 33 * count : 32 * count, hipMemcpyDeviceToHost, t->stream));
        RT_HIP(t->err, hipStreamSynchronize(t->stream));
        if (stored) { memcpy(leaves, back.data(), 32 * count); memcpy(stored, back.data() + 32 * count, count); }
    } catch (const std::bad_alloc&) { return st_fail(t, DST_ERR_HIP, "out of host memory"); }
    return DST_OK;
}

template <class T>
static int stree_read_level(const T* t, uint32_t level, uint64_t first, uint64_t count, void* prefixes /* count keys */, uint8_t* nodes, uint64_t* level_count) {
    if (int r = st_enter(t)) return r;
    if (level > t->depth) return st_fail(t, DST_ERR_ARG, "level past the leaf level");
    const size_t m = t->shape.cnt[level], at = t->shape.start[level] + first;
    if (level_count) *level_count = m;
    if (first > m || count > m - first) return st_fail(t, DST_ERR_ARG, "range past the end of the level");
    if (count == 0) return DST_OK;
    if (prefixes) memcpy(prefixes, t->shape.pref.data() + at, sizeof(typename T::key) * count);
    if (!nodes) return DST_OK;
    if (t->device < 0) { memcpy(nodes, t->host.data() + 2 * at, 32 * count); return DST_OK; }
    RT_HIP(t->err, hipSetDevice(t->device));
    RT_HIP(t->err, hipMemcpy(nodes, t->dev_nodes() + 2 * at, 32 * count, hipMemcpyDeviceToHost));
    return DST_OK;
}
template <class T>
static int stree_root(const T* t, uint8_t root[32]) {
    if (int r = st_enter(t)) return r;
    if (!root) return st_fail(t, DST_ERR_ARG, "null pointer");
    if (t->shape.cnt[0] == 0) { memcpy(root, t->empties, 32); return DST_OK; }     // no keys: E_0
    return stree_read_level(t, 0, 0, 1, nullptr, root, nullptr);
}
template <class T>
static int stree_info(const T* t, dst_stree_info_t* out) {
    if (int r = st_enter(t)) return r;
    if (!out) return st_fail(t, DST_ERR_ARG, "null pointer");
    out->depth = t->depth; out->device = t->device;
    out->keys = t->shape.cnt[t->depth]; out->nodes = t->shape.total();
    out->last_digests = t->last_digests; out->last_device_ms = t->last_ms;
    return DST_OK;
}

// ---- openings: any index below 2^depth, stored or not; a node that is not stored is the E_l of its level ------------------------------------
template <class T>
static int stree_paths(const T* t, const typename T::key* indices, size_t count, uint8_t* out) {
    typedef typename T::key K;
    const size_t n = t->depth + 1, m = count * n;
    if (count > ((size_t)1 << 40)) return st_fail(t, DST_ERR_ARG, "too many indices");
    if (!all_keys(t, indices, count)) return st_fail(t, DST_ERR_ARG, "index past the end");
    if (count == 0) return DST_OK;
    if (t->device < 0) {
        for (size_t s = 0; s < m; s++) {
            uint32_t level; K prefix;
            stree_path_slot(t->depth, indices[s / n], (uint32_t)(s % n), level, prefix);
            const size_t start = t->shape.start[level], pos = stree_find(t->shape.pref.data() + start, t->shape.cnt[level], prefix);
            memcpy(out + 32 * s, pos != STREE_ABSENT ? &t->host[2 * (start + pos)] : t->empties + 2 * level, 32);
        }
        return DST_OK;
    }
    if (int r = rtree_stage(t, 32 * m + sizeof(K) * count)) return r;             // [m nodes][count indices]
    typename T::dev_key* d_idx = reinterpret_cast<typename T::dev_key*>(t->stage + 32 * m);
    RT_HIP(t->err, hipMemcpyAsync(d_idx, indices, sizeof(K) * count, hipMemcpyHostToDevice, t->stream));
    if (k_rescue_stree_open(t->stream, t->dev_nodes(), t->dev_pref(), t->dev_levels(), t->dev_empties(), d_idx, reinterpret_cast<fe*>(t->stage), count, t->depth))
        return st_fail(t, DST_ERR_HIP, "rescue_stree_open_kernel: launch failed");
    RT_HIP(t->err, hipMemcpyAsync(out, t->stage, 32 * m, hipMemcpyDeviceToHost, t->stream));
    RT_HIP(t->err, hipStreamSynchronize(t->stream));
    return DST_OK;
}
template <class T>
static int stree_paths_call(const T* t, const typename T::key* indices, size_t count, uint8_t* paths) {
    if (int r = st_enter(t)) return r;
    if ((!indices || !paths) && count) return st_fail(t, DST_ERR_ARG, "null pointer");
    return stree_paths(t, indices, count, paths);
}
// dst_rtree_tapes_many with n = depth + 1
template <class T>
static int stree_tapes_many(const T* t, const typename T::key* indices, size_t count, uint32_t what, uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each) {
    if (int r = st_enter(t)) return r;
    if (!elems_each || what < 1 || what > 3) return st_fail(t, DST_ERR_ARG, "elems_each missing, or what outside 1..3");
    if (!indices && count) return st_fail(t, DST_ERR_ARG, "null pointer");
    const size_t n = t->depth + 1;
    const size_t each = ((what & 1u) ? 2 * n - 1 : 0) + ((what & 2u) ? n - 1 : 0);
    *elems_each = each;
    if (!tape_a && !tape_b)                                                                // size query
        return all_keys(t, indices, count) ? DST_OK : st_fail(t, DST_ERR_ARG, "index past the end");
    if (!tape_a || !tape_b || cap_elems_each < each) return st_fail(t, DST_ERR_ARG, "tape buffers missing or too small");
    try {
        std::vector<u128> paths(2 * n * count);
        if (int r = stree_paths(t, indices, count, (uint8_t*)paths.data())) return r;
        tapes_from_paths(paths.data(), n, indices, count, what, each, tape_a, tape_b);
    } catch (const std::bad_alloc&) { return st_fail(t, DST_ERR_HIP, "out of host memory"); }
    return DST_OK;
}

// ---- ordered writes (tree_sequence.h): dst_rtree_apply's semantics; a key that is not stored has the leaf E_depth --------------------------------
// On a device tree the witnesses are computed against the generation as it is (tseq_run_device: the level launches read it, nothing writes it),
// then the distinct keys with the value that stays go through dst_stree_set, which states the structure changes.  Source words hold flat
// positions below TSEQ_EMPTY, so such a tree may store at most 2^31 - 2 nodes.
template <class T>
static int stree_apply(T* t, const typename T::key* indices, const uint8_t* leaves, size_t count, uint8_t* paths, uint8_t* roots) {
    typedef typename T::key K;
    if (int r = st_enter(t)) return r;
    if (count == 0) return DST_OK;
    if (!indices || !leaves) return st_fail(t, DST_ERR_ARG, "null pointer");
    if (count >= ((size_t)1 << 31)) return st_fail(t, DST_ERR_ARG, "2^31 operations or more");
    if (t->shape.total() + count * (t->depth + 1) >= (t->device < 0 ? STREE_NEW : TSEQ_EMPTY)) return st_fail(t, DST_ERR_ARG, "too many stored nodes");
    if (!all_keys(t, indices, count)) return st_fail(t, DST_ERR_ARG, "index past the end");
    if (!all_below_p(leaves, 2 * count)) return st_fail(t, DST_ERR_ARG, "a leaf element is not below the modulus");
    const size_t D = t->depth, n = D + 1;
    if (t->device < 0) {                                               // one after the other: open, set, root
        uint64_t digests = 0;
        for (size_t i = 0; i < count; i++) {
            if (paths) { if (int r = stree_paths(t, indices + i, 1, paths + 32 * n * i)) return r; }
            if (int r = stree_set(t, indices + i, leaves + 32 * i, 1)) return r;
            if (roots) memcpy(roots + 32 * i, t->host.data() + 2 * t->shape.start[0], 32);
            digests += t->last_digests;
        }
        t->last_digests = digests;
        return DST_OK;
    }
    try {
        const stree_shape_t<K>& sh = t->shape;
        const tseq_plan_t<K> p = tseq_plan_make(t->depth, indices, count, [&](uint32_t l, K q) {
            const size_t at = stree_find(sh.pref.data() + sh.start[l], sh.cnt[l], q);
            return at == STREE_ABSENT ? TSEQ_EMPTY : (uint32_t)(sh.start[l] + at);
        });
        const size_t m = p.tcnt[D];                                    // the distinct keys, sorted, and the leaf that stays at each
        std::vector<uint8_t> last(32 * m);
        for (size_t j = 0; j < m; j++) memcpy(&last[32 * j], leaves + 32 * (size_t)p.tlast[p.toff[D] + j], 32);
        double ms = 0;
        if (int r = tseq_run_device(t, t->dev_nodes(), t->empties, p, {}, indices, leaves, paths, roots, &ms)) return r;      // the tree is as it was
        if (int r = stree_set(t, p.tpref.data() + p.toff[D], last.data(), m)) return r;
        t->last_digests += (uint64_t)count * D;
        t->last_ms += ms;
        return DST_OK;
    } catch (const std::bad_alloc&) { return st_fail(t, DST_ERR_HIP, "out of host memory"); }
}

// ---- save, load, audit (tree_blob.h) --------------------------------------------------------------------------------------------------------------
// what the two widths differ in on the way to bytes and back: the blob kind, its length, a prefix as little-endian bytes, a prefix as decimal text
static uint32_t st_blob_kind(const dst_stree*) { return TBLOB_SPARSE; }
static uint32_t st_blob_kind(const dst_wtree*) { return TBLOB_WIDE; }
static void st_put_key(uint8_t* at, uint64_t q) { tblob_put_u64(at, q); }
static void st_put_key(uint8_t* at, u128 q) { tblob_put_u64(at, (uint64_t)q); tblob_put_u64(at + 8, (uint64_t)(q >> 64)); }
static void st_get_key(const uint8_t* at, uint64_t& q) { q = tblob_u64(at); }
static void st_get_key(const uint8_t* at, u128& q) { q = (u128)tblob_u64(at) | ((u128)tblob_u64(at + 8) << 64); }
static std::string st_key_text(u128 q) {
    std::string digits;
    do { digits.insert(digits.begin(), (char)('0' + (int)(q % 10))); q /= 10; } while (q);
    return digits;
}
// the saved tree: the header, the level lengths, the prefixes and the nodes, all in the order of the flat positions (the leaf level first): copies
template <class T>
static int stree_save(const T* t, uint8_t* out, size_t cap, size_t* len) {
    typedef typename T::key K;
    if (int r = st_enter(t)) return r;
    if (!len) return st_fail(t, DST_ERR_ARG, "null pointer");
    const size_t total = t->shape.total(), D = t->depth;
    *len = (size_t)(TBLOB_HEADER + 8 * ((uint64_t)D + 1) + (32 + sizeof(K)) * (uint64_t)total);
    if (!out) return DST_OK;                                                                // size query
    if (cap < *len) return st_fail(t, DST_ERR_ARG, "the buffer is smaller than the saved tree");
    tblob_put_header(out, st_blob_kind(t), t->depth, reinterpret_cast<const uint8_t*>(t->empties + 2 * D), t->shape.cnt[D], total);
    uint8_t* at = out + TBLOB_HEADER;
    for (size_t k = 0; k <= D; k++, at += 8) tblob_put_u64(at, t->shape.cnt[D - k]);
    for (size_t j = 0; j < total; j++, at += sizeof(K)) st_put_key(at, t->shape.pref[j]);
    if (total == 0) return DST_OK;
    if (t->device < 0) { memcpy(at, t->host.data(), 32 * total); return DST_OK; }
    RT_HIP(t->err, hipSetDevice(t->device));
    RT_HIP(t->err, hipMemcpy(at, t->dev_nodes(), 32 * total, hipMemcpyDeviceToHost));
    return DST_OK;
}
// the first stored parent, from the root down and by prefix within a level, that is not the digest of its children (a child that is not stored is
// the E_l of its level): *key = (level << 32) | index within the level, all ones when there is none
template <class T>
static int stree_audit_run(const T* t, uint64_t* key, double* ms) {
    const stree_shape_t<typename T::key>& sh = t->shape;
    const size_t D = t->depth, first = sh.cnt[D], count = sh.total() - first;
    *key = ~(uint64_t)0; *ms = 0;
    if (count == 0) return DST_OK;                                                          // no keys, no parents
    if (t->device < 0) {
        const size_t chunk = 1024;
        std::vector<u128> in(4 * chunk), d(2 * chunk);
        for (size_t l = 0; l < D; l++) {
            const size_t cstart = sh.start[l + 1];
            const u128* e = t->empties + 2 * (l + 1);
            for (size_t i = 0; i < sh.cnt[l]; i += chunk) {
                const size_t m = std::min(chunk, sh.cnt[l] - i);
                for (size_t g = 0; g < m; g++) {
                    size_t left, right;
                    stree_children(sh.pref.data() + cstart, sh.cnt[l + 1], sh.pref[sh.start[l] + i + g], left, right);
                    memcpy(&in[4 * g], left != STREE_ABSENT ? &t->host[2 * (cstart + left)] : e, 32);
                    memcpy(&in[4 * g + 2], right != STREE_ABSENT ? &t->host[2 * (cstart + right)] : e, 32);
                }
                rescue_digest_many_host(in.data(), m, d.data());
                for (size_t g = 0; g < m; g++)
                    if (memcmp(&d[2 * g], &t->host[2 * (sh.start[l] + i + g)], 32) != 0) { *key = ((uint64_t)l << 32) | (uint64_t)(i + g); return DST_OK; }
            }
        }
        return DST_OK;
    }
    if (int r = rtree_stage(t, 8)) return r;
    unsigned long long* d_key = reinterpret_cast<unsigned long long*>(t->stage);
    RT_HIP(t->err, hipMemsetAsync(d_key, 0xFF, 8, t->stream));
    RT_HIP(t->err, hipEventRecord(t->ev[0], t->stream));
    if (k_rescue_stree_audit(t->stream, t->dev_nodes(), t->dev_pref(), t->dev_levels(), t->dev_empties(), t->depth, first, count, d_key))
        return st_fail(t, DST_ERR_HIP, "rescue_stree_audit_kernel: launch failed");
    RT_HIP(t->err, hipEventRecord(t->ev[1], t->stream));
    RT_HIP(t->err, hipMemcpyAsync(key, d_key, 8, hipMemcpyDeviceToHost, t->stream));
    RT_HIP(t->err, hipStreamSynchronize(t->stream));
    return rtree_elapsed(t, ms);
}
// the tree is only read: an error here leaves it usable
template <class T>
static int stree_audit(const T* t, int32_t* bad_level, typename T::key* bad_prefix, double* device_ms) {
    if (int r = st_enter(t)) return r;
    if (!bad_level || !bad_prefix) return st_fail(t, DST_ERR_ARG, "null pointer");
    uint64_t key = 0;
    double ms = 0;
    try {
        if (int r = stree_audit_run(t, &key, &ms)) return r;
    } catch (const std::bad_alloc&) { return st_fail(t, DST_ERR_HIP, "out of host memory"); }
    const bool bad = key != ~(uint64_t)0;
    *bad_level = bad ? (int32_t)(key >> 32) : -1;
    *bad_prefix = bad ? t->shape.pref[t->shape.start[key >> 32] + (size_t)(key & 0xFFFFFFFFu)] : 0;
    if (device_ms) *device_ms = ms;
    return DST_OK;
}
// a tree from its saved form: the E_l come from the empty leaf as in dst_stree_create, nothing else is hashed -- a device tree is one allocation
// and four copies into it, the nodes straight from the blob -- unless the caller asks for the audit
template <class T>
static int stree_load(int device, const uint8_t* blob, size_t len, uint32_t audit, T** out) {
    typedef typename T::key K;
    std::string& g_error = T::global_error();
    if (out) *out = nullptr;
    if (!blob || !out) { g_error = "null pointer"; return DST_ERR_ARG; }
    tblob_view v;
    if (const char* why = tblob_parse(blob, len, st_blob_kind((const T*)nullptr), v)) { g_error = why; return DST_ERR_ARG; }
    std::unique_ptr<T> t(new (std::nothrow) T);
    if (!t) { g_error = "out of host memory"; return DST_ERR_HIP; }
    const size_t D = v.depth, total = (size_t)v.nodes;
    t->device = device < 0 ? -1 : device; t->depth = v.depth;
    memcpy(t->empties + 2 * D, v.empty, 32);
    for (size_t l = D; l-- > 0;) {                                                          // E_l = digest(E_{l+1}, E_{l+1})
        const u128 in[4] = {t->empties[2 * l + 2], t->empties[2 * l + 3], t->empties[2 * l + 2], t->empties[2 * l + 3]};
        rescue_digest_many_host(in, 1, t->empties + 2 * l);
    }
    uint64_t lv[2 * T::L] = {0};
    auto copies = [&]() -> int {                                                            // [nodes][empties][levels][prefixes], as stree_apply_device lays it out:
        uint8_t* d = t->dev;                                                                // the nodes go up straight from the caller's blob, no second host image
        if (total) RT_HIP(t->err, hipMemcpyAsync(d, v.values, 32 * total, hipMemcpyHostToDevice, t->stream));
        RT_HIP(t->err, hipMemcpyAsync(d + 32 * total, t->empties, T::empties_bytes, hipMemcpyHostToDevice, t->stream));
        RT_HIP(t->err, hipMemcpyAsync(d + 32 * total + T::empties_bytes, lv, T::levels_bytes, hipMemcpyHostToDevice, t->stream));
        if (total) RT_HIP(t->err, hipMemcpyAsync(d + 32 * total + T::head_bytes, t->shape.pref.data(), sizeof(K) * total, hipMemcpyHostToDevice, t->stream));
        return DST_OK;
    };
    auto upload = [&]() -> int {
        for (size_t l = 0; l <= D; l++) { lv[2 * l] = t->shape.start[l]; lv[2 * l + 1] = t->shape.cnt[l]; }
        if (int r = rtree_stage(t.get(), 0)) return r;
        RT_HIP(t->err, hipMalloc((void**)&t->dev, T::generation_bytes(total)));
        const int r = copies();
        const hipError_t e = hipStreamSynchronize(t->stream);                               // also after a failed copy: the sources are the caller's and this frame's
        if (r != DST_OK) return r;
        RT_HIP(t->err, e);
        return DST_OK;
    };
    try {
        stree_shape_t<K>& sh = t->shape;
        sh.depth = v.depth;
        sh.pref.resize(total);
        for (size_t j = 0; j < total; j++) st_get_key(v.prefixes + sizeof(K) * j, sh.pref[j]);
        size_t at = 0;
        for (size_t k = 0; k <= D; k++) { sh.start[D - k] = at; sh.cnt[D - k] = (size_t)tblob_u64(v.counts + 8 * k); at += sh.cnt[D - k]; }
        if (device >= 0) { if (int r = upload()) { g_error = t->err; return r; } }
        else { t->host.assign(2 * total, 0); if (total) memcpy(t->host.data(), v.values, 32 * total); }
        if (audit) {
            uint64_t key = 0;
            double ms = 0;
            if (int r = stree_audit_run(t.get(), &key, &ms)) { g_error = t->err; return r; }
            if (key != ~(uint64_t)0) {
                g_error = "audit: the node of level " + std::to_string(key >> 32) + " with prefix " + st_key_text(sh.pref[sh.start[key >> 32] + (size_t)(key & 0xFFFFFFFFu)]) +
                          " is not the digest of its children";
                return DST_ERR_ARG;
            }
        }
    } catch (const std::bad_alloc&) { g_error = "out of host memory"; return DST_ERR_HIP; }
    *out = t.release();
    return DST_OK;
}

// ---- the C-ABI: dst_stree_* over 8-byte keys ------------------------------------------------------------------------------------------------------
int dst_stree_create(int device, uint32_t depth, const uint8_t empty_leaf[32], dst_stree** out) { return stree_create(device, depth, empty_leaf, out); }
void dst_stree_destroy(dst_stree* t) { delete t; }
const char* dst_stree_last_error(const dst_stree* t) { return t ? t->err.c_str() : dst_stree::global_error().c_str(); }
int dst_stree_set(dst_stree* t, const uint64_t* indices, const uint8_t* leaves, size_t count) { return stree_set(t, indices, leaves, count); }
int dst_stree_remove(dst_stree* t, const uint64_t* indices, size_t count, uint64_t* removed) { return stree_remove(t, indices, count, removed); }
int dst_stree_compact(dst_stree* t, uint64_t* removed) { return stree_compact(t, removed); }
int dst_stree_get(const dst_stree* t, const uint64_t* indices, size_t count, uint8_t* leaves, uint8_t* stored) { return stree_get(t, indices, count, leaves, stored); }
int dst_stree_read_level(const dst_stree* t, uint32_t level, uint64_t first, uint64_t count, uint64_t* prefixes, uint8_t* nodes, uint64_t* level_count) {
    return stree_read_level(t, level, first, count, prefixes, nodes, level_count);
}
int dst_stree_root(const dst_stree* t, uint8_t root[32]) { return stree_root(t, root); }
int dst_stree_info(const dst_stree* t, dst_stree_info_t* out) { return stree_info(t, out); }
int dst_stree_paths(const dst_stree* t, const uint64_t* indices, size_t count, uint8_t* paths) { return stree_paths_call(t, indices, count, paths); }
int dst_stree_tapes_many(const dst_stree* t, const uint64_t* indices, size_t count, uint32_t what, uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each) {
    return stree_tapes_many(t, indices, count, what, tape_a, tape_b, cap_elems_each, elems_each);
}
int dst_stree_apply(dst_stree* t, const uint64_t* indices, const uint8_t* leaves, size_t count, uint8_t* paths, uint8_t* roots) { return stree_apply(t, indices, leaves, count, paths, roots); }
int dst_stree_audit(const dst_stree* t, int32_t* bad_level, uint64_t* bad_prefix, double* device_ms) { return stree_audit(t, bad_level, bad_prefix, device_ms); }
int dst_stree_save(const dst_stree* t, uint8_t* out, size_t cap, size_t* len) { return stree_save(t, out, cap, len); }
int dst_stree_load(int device, const uint8_t* blob, size_t len, uint32_t audit, dst_stree** out) { return stree_load(device, blob, len, audit, out); }

// ---- ... and dst_wtree_* over 16-byte keys: little-endian integers at any alignment, copied into u128 before the call of the same name reads them ----
struct wt_keys {
    std::vector<u128> v;
    const u128* p = nullptr;                           // nullptr: no keys were given (the call refuses that where the narrow one does)
    const char* why = nullptr;
    wt_keys(const uint8_t* keys, size_t count) {
        if (!keys || count == 0) return;
        if (count > ((size_t)1 << 40)) { why = "too many keys"; return; }
        try { v.resize(count); memcpy(v.data(), keys, 16 * count); p = v.data(); } catch (const std::bad_alloc&) { why = "out of host memory"; }
    }
};
#define WT_KEYS(k, t, keys, count)                                                                          \
    if (int r_ = st_enter(t)) return r_;                                                                    \
    wt_keys k(keys, count);                                                                                 \
    if (k.why) return st_fail(t, k.why[0] == 't' ? DST_ERR_ARG : DST_ERR_HIP, k.why)
int dst_wtree_create(int device, uint32_t depth, const uint8_t empty_leaf[32], dst_wtree** out) { return stree_create(device, depth, empty_leaf, out); }
void dst_wtree_destroy(dst_wtree* t) { delete t; }
const char* dst_wtree_last_error(const dst_wtree* t) { return t ? t->err.c_str() : dst_wtree::global_error().c_str(); }
int dst_wtree_set(dst_wtree* t, const uint8_t* keys, const uint8_t* leaves, size_t count) { WT_KEYS(k, t, keys, count); return stree_set(t, k.p, leaves, count); }
int dst_wtree_remove(dst_wtree* t, const uint8_t* keys, size_t count, uint64_t* removed) { WT_KEYS(k, t, keys, count); return stree_remove(t, k.p, count, removed); }
int dst_wtree_compact(dst_wtree* t, uint64_t* removed) { return stree_compact(t, removed); }
int dst_wtree_get(const dst_wtree* t, const uint8_t* keys, size_t count, uint8_t* leaves, uint8_t* stored) { WT_KEYS(k, t, keys, count); return stree_get(t, k.p, count, leaves, stored); }
int dst_wtree_read_level(const dst_wtree* t, uint32_t level, uint64_t first, uint64_t count, uint8_t* prefixes, uint8_t* nodes, uint64_t* level_count) {
    return stree_read_level(t, level, first, count, prefixes, nodes, level_count);
}
int dst_wtree_root(const dst_wtree* t, uint8_t root[32]) { return stree_root(t, root); }
int dst_wtree_info(const dst_wtree* t, dst_stree_info_t* out) { return stree_info(t, out); }
int dst_wtree_paths(const dst_wtree* t, const uint8_t* keys, size_t count, uint8_t* paths) { WT_KEYS(k, t, keys, count); return stree_paths_call(t, k.p, count, paths); }
int dst_wtree_tapes_many(const dst_wtree* t, const uint8_t* keys, size_t count, uint32_t what, uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each) {
    WT_KEYS(k, t, keys, count);
    return stree_tapes_many(t, k.p, count, what, tape_a, tape_b, cap_elems_each, elems_each);
}
int dst_wtree_apply(dst_wtree* t, const uint8_t* keys, const uint8_t* leaves, size_t count, uint8_t* paths, uint8_t* roots) { WT_KEYS(k, t, keys, count); return stree_apply(t, k.p, leaves, count, paths, roots); }
int dst_wtree_audit(const dst_wtree* t, int32_t* bad_level, uint8_t bad_prefix[16], double* device_ms) {
    u128 q = 0;
    const int r = stree_audit(t, bad_level, bad_prefix ? &q : nullptr, device_ms);
    if (r == DST_OK) memcpy(bad_prefix, &q, 16);
    return r;
}
int dst_wtree_save(const dst_wtree* t, uint8_t* out, size_t cap, size_t* len) { return stree_save(t, out, cap, len); }
int dst_wtree_load(int device, const uint8_t* blob, size_t len, uint32_t audit, dst_wtree** out) { return stree_load(device, blob, len, audit, out); }
#undef WT_KEYS
// overwrites one stored node where it lives and hashes nothing: how the tests give an audit something to find in a tree that cannot be loaded from
// changed bytes.  Test build only; the product library keeps the entry point and answers DST_ERR_STATE
int dst_wtree_test_set_node(dst_wtree* t, uint32_t level, uint64_t index, const uint8_t node[32]) {
    if (int r = st_enter(t)) return r;
#if DST_TEST_HOOKS
    if (!node || level > t->depth || index >= t->shape.cnt[level]) return st_fail(t, DST_ERR_ARG, "no such stored node");
    const size_t at = t->shape.start[level] + (size_t)index;
    if (t->device < 0) { memcpy(&t->host[2 * at], node, 32); return DST_OK; }
    RT_HIP(t->err, hipSetDevice(t->device));
    RT_HIP(t->err, hipMemcpy(t->dev_nodes() + 2 * at, node, 32, hipMemcpyHostToDevice));
    return DST_OK;
#else
    return st_fail(t, DST_ERR_STATE, "dst_wtree_test_set_node is part of the test build (libdistaff_hip_hooks.so) only");
#endif
}
