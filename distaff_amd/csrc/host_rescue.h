// utils::hasher::digest (src/utils/hasher.rs:12-40) and the Rescue Merkle trees of the VM's smpath / pmpath on the host: one thread, the
// field and the inverse S-box chain of host_vm.h.  The device < 0 path of dst_rescue_digest_many / dst_rtree_build, i.e. the CPU baseline of
// profiles/rescue_tree.md and what runs where there is no GPU.  Also the layout helpers both paths share (authentication paths, secret tapes).
#pragma once
#include "host_vm.h"

namespace dsth {

struct HasherTables {                                     // rounds 0..9 of HASHER_ARK by half round, HASHER_MDS; converted once
    u128 ark[20][6], mds[36];
    HasherTables() {
        for (int h = 0; h < 20; h++) for (int i = 0; i < 6; i++) ark[h][i] = limbs(HASHER_ARK[(h & 1) * 6 + i][h >> 1]);      // hasher.rs:33,37
        for (int i = 0; i < 36; i++) mds[i] = limbs(HASHER_MDS[i]);
    }
};
inline const HasherTables& hasher_tables() { static const HasherTables t; return t; }

// K digests at once: digest(v[k][0..4]) -> out[k][0..2]; inputs below p.  inv_alpha4 walks the chain on four elements in lock-step, so the 6 K
// state elements go through it in groups of four: with K = 2 that is three full groups per half round, no lane spent on padding.
template <int K>
inline void rescue_digests_host(const u128 (*v)[4], u128 (*out)[2]) {
    const HasherTables& T = hasher_tables();
    u128 s[6 * K + 3] = {0};                              // state k at s[6 k ..): hasher.rs:16-18, state[..4] = values, reversed; 3 elements of padding
    for (int k = 0; k < K; k++) { s[6 * k + 2] = v[k][3]; s[6 * k + 3] = v[k][2]; s[6 * k + 4] = v[k][1]; s[6 * k + 5] = v[k][0]; }
    for (int h = 0; h < 20; h++) {                        // apply_round (hasher.rs:28) in two halves
        for (int k = 0; k < K; k++) for (int i = 0; i < 6; i++) s[6 * k + i] = hf_add(s[6 * k + i], T.ark[h][i]);
        if (h & 1) { for (int g = 0; g < 6 * K; g += 4) inv_alpha4(s + g); }
        else { for (int i = 0; i < 6 * K; i++) s[i] = hf_mul(hf_sqr(s[i]), s[i]); }
        for (int k = 0; k < K; k++) {
            u128 r[6];
            for (int i = 0; i < 6; i++) { u128 acc = 0; for (int j = 0; j < 6; j++) acc = hf_add(acc, hf_mul(T.mds[i * 6 + j], s[6 * k + j])); r[i] = acc; }
            for (int i = 0; i < 6; i++) s[6 * k + i] = r[i];
        }
        for (int i = 6 * K; i < 6 * K + 3; i++) s[i] = 0;
    }
    for (int k = 0; k < K; k++) { out[k][0] = s[6 * k + 5]; out[k][1] = s[6 * k + 4]; }      // hasher.rs:24-25
}
// `count` digests: in = 4 elements each, out = 2 elements each
inline void rescue_digest_many_host(const u128* in, size_t count, u128* out) {
    size_t i = 0;
    for (; i + 2 <= count; i += 2) rescue_digests_host<2>(reinterpret_cast<const u128(*)[4]>(in + 4 * i), reinterpret_cast<u128(*)[2]>(out + 2 * i));
    if (i < count) rescue_digests_host<1>(reinterpret_cast<const u128(*)[4]>(in + 4 * i), reinterpret_cast<u128(*)[2]>(out + 2 * i));
}

// nodes[1 .. leaves) of a node array (2 elements per node, nodes[1] = root) whose leaf level nodes[leaves .. 2 leaves) is in place
inline void rescue_tree_host(u128* nodes, size_t leaves) {
    for (size_t count = leaves >> 1; count >= 1; count >>= 1) rescue_digest_many_host(nodes + 4 * count, count, nodes + 2 * count);      // level by level: parents count .. 2 count
}
// the dirty parents of an update, level by level from the level of leaves / 2 parents (level log_leaves - 1) to the root (level 0): level l has
// cnt[l] of them, their node-array positions at lists[off[l] ..), or no list when the whole level is dirty (cnt[l] == 2^l).  scratch: 6 elements
// per parent of the longest list
inline void rescue_tree_update_host(u128* nodes, uint32_t log_leaves, const uint32_t* lists, const size_t* off, const size_t* cnt, u128* scratch) {
    for (uint32_t l = log_leaves; l-- > 0;) {
        const size_t m = cnt[l];
        if (m == ((size_t)1 << l)) { rescue_digest_many_host(nodes + 4 * m, m, nodes + 2 * m); continue; }
        const uint32_t* list = lists + off[l];
        u128 *in = scratch, *out = scratch + 4 * m;
        for (size_t i = 0; i < m; i++) memcpy(in + 4 * i, nodes + 4 * (size_t)list[i], 64);
        rescue_digest_many_host(in, m, out);
        for (size_t i = 0; i < m; i++) memcpy(nodes + 2 * (size_t)list[i], out + 2 * i, 32);
    }
}

// node-array positions of the authentication path of leaf `index`: [leaf, sibling, uncle, ...], log_leaves + 1 of them (merkle.rs:98-145)
inline void rescue_path_positions(uint32_t log_leaves, uint64_t index, uint64_t* pos) {
    uint64_t p = ((uint64_t)1 << log_leaves) + index;
    pos[0] = p;
    for (uint32_t k = 0; k < log_leaves; k++, p >>= 1) pos[1 + k] = p ^ 1;
}

// the secret tapes of generate_program_inputs (merkle.rs:63-94) from a path of n nodes: what & 1 the leaf and the smpath inputs (2n - 1
// elements per tape), what & 2 the pmpath inputs (n - 1)
inline void rescue_tapes(const u128* path /* 2 per node */, size_t n, u128 index /* below 2^(n-1), n <= 128 */, uint32_t what, std::vector<u128>& a, std::vector<u128>& b) {
    a.clear(); b.clear();
    if (what & 1u) {
        u128 idx = index + ((u128)1 << (n - 1));
        a.push_back(path[0]); b.push_back(path[1]);
        for (size_t i = 1; i < n; i++) {
            a.push_back(0); b.push_back(idx & 1); idx >>= 1;
            a.push_back(path[2 * i]); b.push_back(path[2 * i + 1]);
        }
    }
    if (what & 2u)
        for (size_t i = 1; i < n; i++) { a.push_back(path[2 * i]); b.push_back(path[2 * i + 1]); }
}

}  // namespace dsth
