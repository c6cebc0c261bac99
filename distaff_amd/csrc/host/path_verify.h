// Checking authentication paths and the witnesses of ordered writes (dst_rescue_path_roots, dst_rescue_verify_paths, dst_rescue_verify_writes): what
// needs neither HIP nor field arithmetic.  The chains themselves -- compute_merkle_root (src/examples/merkle.rs:112-145) of every path -- are hashed
// elsewhere (kernels_hash.hip on a device, host_rescue.h on the host); here are the argument checks before them and the decision after them: given
// the roots the chains resolved to, which path or write is the first that does not hold, and why.  Nodes and roots are 32 opaque bytes here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#define PV_MIN_NODES 2u
#define PV_MAX_NODES 64u
#define PV_WIDE_MAX_NODES 128u                       // the calls with 16-byte indices (dst_rescue_*_w)
// the values of `why` (include/distaff_hip.h: DST_PATH_*)
enum { PV_OK = 0, PV_BAD_LEAF = 1, PV_BAD_ROOT = 2, PV_BAD_NEXT_ROOT = 3 };

// nullptr when `count` paths of n nodes with these indices can be hashed, else what is wrong: 2 <= n <= 64 (128 for the 16-byte indices K of
// the wide calls), count < 2^31, indices[i] < 2^(n-1)
template <class K> inline const char* pv_check_shape_of(uint32_t n, const K* indices, size_t count) {
    if (n < PV_MIN_NODES || n > 8 * sizeof(K)) return sizeof(K) == 8 ? "a path has 2 .. 64 nodes" : "a path has 2 .. 128 nodes";
    if ((uint64_t)count >= ((uint64_t)1 << 31)) return "2^31 paths or more";
    for (size_t i = 0; i < count; i++)
        if (indices[i] >> (n - 1)) return "leaf index past the end";       // n - 1 is below the width of K: the shift is defined
    return nullptr;
}
inline const char* pv_check_shape(uint32_t n, const uint64_t* indices, size_t count) { return pv_check_shape_of<uint64_t>(n, indices, count); }

struct pv_verdict {
    int64_t first_bad = -1;
    uint32_t why = PV_OK;
};
inline bool pv_same(const uint8_t* a, const uint8_t* b) { return memcmp(a, b, 32) == 0; }

// membership / absence: own[i] = what path i resolves to.  Path i holds when (leaves != nullptr) its first node is leaves[i] and own[i] == root; the
// lowest i that does not, and the first thing that fails there (the leaf before the root)
inline pv_verdict pv_decide_paths(const uint8_t* own, const uint8_t* root, const uint8_t* paths, uint32_t n, const uint8_t* leaves, size_t count) {
    pv_verdict v;
    for (size_t i = 0; i < count; i++) {
        uint32_t why = PV_OK;
        if (leaves && !pv_same(paths + 32 * (size_t)n * i, leaves + 32 * i)) why = PV_BAD_LEAF;
        else if (!pv_same(own + 32 * i, root)) why = PV_BAD_ROOT;
        if (why != PV_OK) { v.first_bad = (int64_t)i; v.why = why; break; }
    }
    return v;
}

// ordered writes: own[i] = what path i resolves to with its own first node (the old leaf), next[i] = with the written leaf in its place.  Write i
// holds when own[i] is the root before it -- root_before for i = 0, else next[i - 1], the root after write i - 1 as computed, never as claimed --
// and (roots != nullptr) next[i] == roots[i].  root_after (may be nullptr) = next[count - 1], or root_before when there is no write
inline pv_verdict pv_decide_writes(const uint8_t* own, const uint8_t* next, const uint8_t* root_before, const uint8_t* roots, size_t count, uint8_t* root_after) {
    pv_verdict v;
    for (size_t i = 0; i < count; i++) {
        uint32_t why = PV_OK;
        if (!pv_same(own + 32 * i, i ? next + 32 * (i - 1) : root_before)) why = PV_BAD_ROOT;
        else if (roots && !pv_same(next + 32 * i, roots + 32 * i)) why = PV_BAD_NEXT_ROOT;
        if (why != PV_OK) { v.first_bad = (int64_t)i; v.why = why; break; }
    }
    if (root_after) memcpy(root_after, count ? next + 32 * (count - 1) : root_before, 32);
    return v;
}
