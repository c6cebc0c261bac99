// Host-side verifier for the proofs this library writes: stark::verify restated in the product's own terms (dst_verify / dst_proof_info of
// include/distaff_hip.h).  No device, no context, no globals; nothing here calls the HIP runtime.
//
// Follows /root/reference/src/stark/verifier.rs (verify :11-75, evaluate_constraints :79-96, compose_registers :98-136,
// compose_constraints :138-162), src/stark/fri/verifier.rs (verify :11-89, verify_remainder :91-124, get_column_values :128),
// src/stark/fri/utils.rs:4-24, src/crypto/merkle.rs:154-264 (verify_batch), src/stark/utils/proof_of_work.rs:34-56,
// src/stark/utils/mod.rs:13-53, src/math/polynom.rs:47-75 (interpolate), src/math/quartic.rs:6-135, and the wire layout of
// src/stark/proof.rs:11-37, fri/mod.rs:18-30, merkle.rs:14-18, options.rs:16-27 under bincode's default encoding (the inverse of the writer
// in host_proof.h).  Rejections carry the reference's strings, in the reference's order of checks.
//
// Two kinds of failure are kept apart.  Bytes that are not a StarkProof this library could have written -- truncated, a length prefix that
// runs past the end, trailing bytes, an options byte outside ProofOptions::new (options.rs:35-46), a hash tag other than 0, a depth outside
// the limits of lib.rs:80-83,138 or the field's 2^40 two-adicity, a field element not below the modulus, a remainder that is not the
// last layer of its own FRI layers (at most 256 values) -- are MALFORMED (parse_proof fails; DST_ERR_ARG).  A proof that parses
// and does not verify is REJECTED with a reason.  Every vector length is capped by the bytes that remain before anything is reserved.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "../host_proof.h"
#include "../host_util.h"
#include "../host_vm.h"
#include "host_air.h"

namespace dsth {
namespace hver {

typedef std::array<uint8_t, 32> digest;
typedef std::array<u128, 4> quad;

struct VBatch { std::vector<digest> values; std::vector<std::vector<digest>> nodes; uint8_t depth = 0; };      // merkle.rs:14
struct VFriLayer { digest root; std::vector<quad> values; std::vector<std::vector<digest>> nodes; uint8_t depth = 0; };   // fri/mod.rs:25
struct VProof {                                                  // proof.rs:11-37
    digest trace_root, constraint_root, rem_root;
    uint8_t domain_depth = 0, ctx_depth = 0, loop_depth = 0, stack_depth = 0;
    uint32_t op_count = 0;
    std::vector<std::vector<digest>> trace_nodes;
    std::vector<std::vector<u128>> trace_evaluations;
    VBatch constraint_proof;
    std::vector<u128> trace_at_z1, trace_at_z2;
    std::vector<VFriLayer> layers;
    std::vector<u128> rem_values;
    uint64_t pow_nonce = 0;
    uint8_t log_blowup = 0, num_queries = 0, grinding = 0;
    uint64_t domain_size() const { return (uint64_t)1 << domain_depth; }
    uint64_t trace_length() const { return domain_size() >> log_blowup; }
};

// ---- bincode reader -----------------------------------------------------------------------------------------------------------------------
struct Reader {
    const uint8_t* p; size_t n, o = 0;
    bool bad = false;
    Reader(const uint8_t* d, size_t len) : p(d), n(len) {}
    size_t left() const { return n - o; }
    bool need(size_t k) { if (bad || k > left()) { bad = true; return false; } return true; }
    uint8_t u8() { if (!need(1)) return 0; return p[o++]; }
    uint32_t u32() { if (!need(4)) return 0; uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[o + i] << (8 * i); o += 4; return v; }
    uint64_t u64() { if (!need(8)) return 0; uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[o + i] << (8 * i); o += 8; return v; }
    bool noncanonical = false;                                   // saw an element >= p: host_vm.h's add / sub are only right below p
    u128 el() { if (!need(16)) return 0; u128 v; memcpy(&v, p + o, 16); o += 16; if (v >= FIELD_P) noncanonical = true; return v; }   // little-endian host (as host_util.h)
    digest h() { digest v; v.fill(0); if (!need(32)) return v; memcpy(v.data(), p + o, 32); o += 32; return v; }
    // a Vec's u64 length prefix, refused unless `item` bytes per element still fit into the input (item = the smallest encoding of one element)
    size_t len(size_t item) { uint64_t k = u64(); if (bad || k > left() / item) { bad = true; return 0; } return (size_t)k; }
    void hv(std::vector<digest>& v) { size_t k = len(32); v.resize(k); for (size_t i = 0; i < k && !bad; i++) v[i] = h(); }
    void hvv(std::vector<std::vector<digest>>& v) { size_t k = len(8); v.resize(k); for (size_t i = 0; i < k && !bad; i++) hv(v[i]); }
    void ev(std::vector<u128>& v) { size_t k = len(16); v.resize(k); for (size_t i = 0; i < k && !bad; i++) v[i] = el(); }
};

// 0, or -1 with the reason in `why`
inline int parse_proof(const uint8_t* data, size_t len, VProof& p, std::string& why) {
    if (!data && len) { why = "proof is NULL"; return -1; }
    Reader r(data, len);
    p.trace_root = r.h();
    p.domain_depth = r.u8(); p.ctx_depth = r.u8(); p.loop_depth = r.u8(); p.stack_depth = r.u8(); p.op_count = r.u32();
    r.hvv(p.trace_nodes);
    size_t k = r.len(8);
    p.trace_evaluations.resize(k);
    for (size_t i = 0; i < k && !r.bad; i++) r.ev(p.trace_evaluations[i]);
    p.constraint_root = r.h();
    r.hv(p.constraint_proof.values); r.hvv(p.constraint_proof.nodes); p.constraint_proof.depth = r.u8();
    r.ev(p.trace_at_z1); r.ev(p.trace_at_z2);
    k = r.len(32 + 8 + 8 + 1);
    p.layers.resize(k);
    for (size_t i = 0; i < k && !r.bad; i++) {
        VFriLayer& l = p.layers[i];
        l.root = r.h();
        size_t m = r.len(64);
        l.values.resize(m);
        for (size_t j = 0; j < m && !r.bad; j++) for (int c = 0; c < 4; c++) l.values[j][c] = r.el();
        r.hvv(l.nodes); l.depth = r.u8();
    }
    p.rem_root = r.h(); r.ev(p.rem_values);
    p.pow_nonce = r.u64();
    p.log_blowup = r.u8(); p.num_queries = r.u8(); p.grinding = r.u8();
    uint8_t hash_tag = r.u8();
    if (r.bad) { why = "proof truncated"; return -1; }
    if (r.o != len) { why = "trailing bytes after proof"; return -1; }
    if (r.noncanonical) { why = "field element not below the modulus"; return -1; }                 // the header's convention: canonical elements only
    if (hash_tag != 0) { why = "unsupported hash function"; return -1; }                             // options.rs:116-119
    if (p.log_blowup < 4 || p.log_blowup > 8) { why = "extension_factor must be a power of 2 between 16 and 256"; return -1; }   // options.rs:35-37
    if (p.num_queries == 0 || p.num_queries > 128) { why = "num_queries must be between 1 and 128"; return -1; }                  // :39-40
    if (p.grinding > 32) { why = "grinding factor cannot be greater than 32"; return -1; }                                      // :42
    if (p.ctx_depth > hair::MAX_CTX || p.loop_depth > hair::MAX_LOOP || p.stack_depth > hair::MAX_STACK) { why = "register depths exceed the limits of the instruction set"; return -1; }
    if (p.domain_depth > 40 || p.domain_depth < p.log_blowup + 4) { why = "domain depth outside [log2(extension_factor) + 4, 40]"; return -1; }   // MIN_TRACE_LENGTH = 16 (lib.rs:82), field.rs:14
    if (p.layers.empty()) { why = "low-degree proof has no layers"; return -1; }
    if (p.layers[0].depth > 38 || 2 * p.layers.size() > (size_t)p.layers[0].depth + 2) { why = "low-degree proof layers do not fit their domain"; return -1; }
    // the remainder is the last committed layer (fri/prover.rs:11-53, MAX_REMAINDER_LENGTH = 256, fri/mod.rs:13): what is left of the first
    // layer's domain after a factor 4 per layer.  Anything else is not a proof the prover writes -- and the remainder check is quadratic in it.
    if (p.rem_values.size() > 256 || p.rem_values.size() != (((size_t)4 << p.layers[0].depth) >> (2 * p.layers.size()))) { why = "remainder length does not match the low-degree proof's layers"; return -1; }
    return 0;
}

// ---- hashes ---------------------------------------------------------------------------------------------------------------------------------
inline digest hash_bytes(const uint8_t* p, size_t len) { digest d; blake3_short(p, len, d.data()); return d; }
inline digest hash_2x1(const digest& a, const digest& b) {
    uint8_t buf[64];
    memcpy(buf, a.data(), 32); memcpy(buf + 32, b.data(), 32);
    return hash_bytes(buf, 64);
}

// merkle.rs:154-264.  Where the reference indexes or unwraps without a check, a missing item is a failed verification.
inline bool verify_batch(const digest& root, const std::vector<uint64_t>& indexes_in, const std::vector<digest>& values,
                         const std::vector<std::vector<digest>>& nodes, uint8_t depth) {
    if (depth > 62) return false;
    std::map<uint64_t, digest> v;
    const uint64_t offset = (uint64_t)1 << depth;
    std::map<uint64_t, size_t> index_map;
    for (size_t i = 0; i < indexes_in.size(); i++) {
        if (indexes_in[i] > offset - 1) return false;
        index_map[indexes_in[i]] = i;
    }
    if (index_map.size() != indexes_in.size()) return false;
    std::set<uint64_t> norm;                                     // normalize_indexes :306
    for (uint64_t i : indexes_in) norm.insert(i - (i & 1));
    std::vector<uint64_t> indexes(norm.begin(), norm.end());
    if (indexes.size() != nodes.size()) return false;
    std::vector<uint64_t> next;
    std::vector<size_t> ptrs;
    for (size_t i = 0; i < indexes.size(); i++) {
        uint64_t index = indexes[i];
        digest a, b;
        auto i1 = index_map.find(index), i2 = index_map.find(index + 1);
        if (i1 != index_map.end()) {
            if (values.size() <= i1->second) return false;
            a = values[i1->second];
            if (i2 != index_map.end()) {
                if (values.size() <= i2->second) return false;
                b = values[i2->second];
                ptrs.push_back(0);
            } else {
                if (nodes[i].size() < 1) return false;
                b = nodes[i][0];
                ptrs.push_back(1);
            }
        } else {
            if (nodes[i].size() < 1 || i2 == index_map.end() || values.size() <= i2->second) return false;
            a = nodes[i][0];
            b = values[i2->second];
            ptrs.push_back(1);
        }
        uint64_t parent = (offset + index) >> 1;
        v[parent] = hash_2x1(a, b);
        next.push_back(parent);
    }
    for (int d = 1; d < depth; d++) {
        std::vector<uint64_t> cur = next;
        next.clear();
        size_t i = 0;
        while (i < cur.size()) {
            uint64_t node_index = cur[i], sib_index = node_index ^ 1;
            digest sib;
            if (i + 1 < cur.size() && cur[i + 1] == sib_index) {
                auto s = v.find(sib_index);
                if (s == v.end()) return false;
                sib = s->second;
                i += 1;
            } else {
                size_t ptr = ptrs[i];
                if (nodes[i].size() <= ptr) return false;
                sib = nodes[i][ptr];
                ptrs[i] += 1;
            }
            auto nd = v.find(node_index);
            if (nd == v.end()) return false;
            digest parent = (node_index & 1) ? hash_2x1(sib, nd->second) : hash_2x1(nd->second, sib);
            v[node_index >> 1] = parent;
            next.push_back(node_index >> 1);
            i += 1;
        }
    }
    auto rt = v.find(1);
    return rt != v.end() && rt->second == root;
}

// ---- small polynomial helpers -------------------------------------------------------------------------------------------------------------
using hair::hf_div;
using hair::hf_inv;
using hair::hf_root_of_unity;
inline u128 hf_neg(u128 a) { return hf_sub(0, a); }
inline void inv_many(const u128* values, u128* result, size_t n) {                                  // field.rs:173 (zeros stay zero)
    u128 last = 1;
    for (size_t i = 0; i < n; i++) { result[i] = last; if (values[i] != 0) last = hf_mul(last, values[i]); }
    last = hf_inv(last);
    for (size_t i = n; i-- > 0;) {
        if (values[i] == 0) result[i] = 0;
        else { result[i] = hf_mul(last, result[i]); last = hf_mul(last, values[i]); }
    }
}
inline u128 quartic_eval(const quad& p, u128 x) {                                                   // quartic.rs:6
    u128 y = hf_add(p[0], hf_mul(p[1], x));
    u128 x2 = hf_mul(x, x);
    y = hf_add(y, hf_mul(p[2], x2));
    return hf_add(y, hf_mul(p[3], hf_mul(x2, x)));
}
inline std::vector<quad> quartic_interpolate_batch(const std::vector<quad>& xs, const std::vector<quad>& ys) {   // quartic.rs:37
    size_t n = xs.size();
    std::vector<quad> equations(n * 4);
    std::vector<u128> inverses(n * 4), invd(n * 4);
    for (size_t i = 0, j = 0; i < n; i++, j += 4) {
        const quad& x = xs[i];
        u128 x01 = hf_mul(x[0], x[1]), x02 = hf_mul(x[0], x[2]), x03 = hf_mul(x[0], x[3]);
        u128 x12 = hf_mul(x[1], x[2]), x13 = hf_mul(x[1], x[3]), x23 = hf_mul(x[2], x[3]);
        equations[j] = {hf_mul(hf_neg(x12), x[3]), hf_add(hf_add(x12, x13), x23), hf_sub(hf_sub(hf_neg(x[1]), x[2]), x[3]), 1};
        equations[j + 1] = {hf_mul(hf_neg(x02), x[3]), hf_add(hf_add(x02, x03), x23), hf_sub(hf_sub(hf_neg(x[0]), x[2]), x[3]), 1};
        equations[j + 2] = {hf_mul(hf_neg(x01), x[3]), hf_add(hf_add(x01, x03), x13), hf_sub(hf_sub(hf_neg(x[0]), x[1]), x[3]), 1};
        equations[j + 3] = {hf_mul(hf_neg(x01), x[2]), hf_add(hf_add(x01, x02), x12), hf_sub(hf_sub(hf_neg(x[0]), x[1]), x[2]), 1};
        for (int k = 0; k < 4; k++) inverses[j + k] = quartic_eval(equations[j + k], x[k]);
    }
    inv_many(inverses.data(), invd.data(), n * 4);
    std::vector<quad> result(n);
    for (size_t i = 0, j = 0; i < n; i++, j += 4) {
        quad r = {0, 0, 0, 0};
        for (int k = 0; k < 4; k++) {
            u128 inv_y = hf_mul(ys[i][k], invd[j + k]);
            for (int c = 0; c < 4; c++) r[c] = hf_add(r[c], hf_mul(inv_y, equations[j + k][c]));
        }
        result[i] = r;
    }
    return result;
}
// the polynomial of degree < m through (xs[i], ys[i]), distinct xs (polynom.rs:47: Lagrange over the master polynomial's quotients)
inline std::vector<u128> interpolate(const std::vector<u128>& xs, const std::vector<u128>& ys) {
    size_t m = xs.size();
    std::vector<u128> roots(m + 1, 0);                           // prod (x - xs[i]), lowest coefficient first
    roots[0] = 1;
    for (size_t i = 0; i < m; i++)
        for (size_t j = i + 1; j-- > 0;) {                       // times (x - xs[i]), in place from the top
            roots[j + 1] = hf_add(roots[j + 1], roots[j]);
            roots[j] = hf_mul(roots[j], hf_neg(xs[i]));
        }
    std::vector<u128> result(m, 0), num(m), den(m), inv_den(m);
    std::vector<std::vector<u128>> numerators(m);
    for (size_t i = 0; i < m; i++) {                             // roots / (x - xs[i]) by synthetic division
        u128 c = 0;
        for (size_t j = m + 1; j-- > 1;) { c = hf_add(roots[j], hf_mul(c, xs[i])); num[j - 1] = c; }
        numerators[i] = num;
        den[i] = hair::poly_eval(num.data(), m, xs[i]);
    }
    inv_many(den.data(), inv_den.data(), m);
    for (size_t i = 0; i < m; i++) {
        u128 y = hf_mul(ys[i], inv_den[i]);
        for (size_t j = 0; j < m; j++) result[j] = hf_add(result[j], hf_mul(numerators[i][j], y));
    }
    return result;
}

struct VerifyResult { bool ok; std::string error; };

// ---- FRI (fri/verifier.rs) ----------------------------------------------------------------------------------------------------------------
inline VerifyResult fri_verify_remainder(const std::vector<u128>& remainder, uint64_t max_degree_plus_1, u128 domain_root, uint64_t blowup) {   // :91
    if (max_degree_plus_1 > remainder.size()) return {false, "remainder degree is greater than number of remainder values"};
    std::vector<size_t> positions;
    for (size_t i = 0; i < remainder.size(); i++) if (i % blowup != 0) positions.push_back(i);
    if (max_degree_plus_1 > positions.size()) return {false, "remainder degree is greater than number of remainder values"};
    std::vector<u128> domain(remainder.size());
    domain[0] = 1;
    for (size_t i = 1; i < domain.size(); i++) domain[i] = hf_mul(domain[i - 1], domain_root);
    std::vector<u128> xs, ys;
    for (size_t i = 0; i < max_degree_plus_1; i++) { xs.push_back(domain[positions[i]]); ys.push_back(remainder[positions[i]]); }
    std::vector<u128> poly = interpolate(xs, ys);
    for (size_t i = max_degree_plus_1; i < positions.size(); i++) {
        size_t p = positions[i];
        if (hair::poly_eval(poly.data(), poly.size(), domain[p]) != remainder[p])
            return {false, "remainder is not a valid degree " + std::to_string(max_degree_plus_1 - 1) + " polynomial"};
    }
    return {true, ""};
}

inline VerifyResult fri_verify(const VProof& proof, const std::vector<u128>& evaluations_in, const std::vector<uint64_t>& positions_in, uint64_t max_degree) {   // :11
    uint64_t domain_size = ((uint64_t)1 << proof.layers[0].depth) * 4;                              // depth <= 38: parse_proof
    uint32_t log_domain = proof.layers[0].depth + 2;
    u128 domain_root = hf_root_of_unity(log_domain);
    u128 quartic_roots[4] = {1, hf_pow(domain_root, domain_size / 4), hf_pow(domain_root, domain_size / 2), hf_pow(domain_root, domain_size / 4 * 3)};
    uint64_t max_degree_plus_1 = max_degree + 1;
    std::vector<uint64_t> positions = positions_in;
    std::vector<u128> evaluations = evaluations_in;
    for (size_t depth = 0; depth < proof.layers.size(); depth++) {
        const VFriLayer& layer = proof.layers[depth];
        std::vector<uint64_t> augmented = augmented_positions(positions, domain_size);            // fri/utils.rs:4
        uint64_t row_length = domain_size / 4;
        const std::string mismatch = "evaluations did not match column value at depth " + std::to_string(depth);
        if (evaluations.size() != positions.size()) return {false, mismatch};
        for (size_t i = 0; i < positions.size(); i++) {                                             // get_column_values :128
            size_t idx = std::find(augmented.begin(), augmented.end(), positions[i] % row_length) - augmented.begin();
            uint64_t col = positions[i] / row_length;
            if (idx >= layer.values.size() || col >= 4 || layer.values[idx][col] != evaluations[i]) return {false, mismatch};
        }
        std::vector<digest> leaves(layer.values.size());                                            // fri/utils.rs:16 hash_values
        for (size_t i = 0; i < leaves.size(); i++) leaves[i] = hash_bytes((const uint8_t*)layer.values[i].data(), 64);
        if (!verify_batch(layer.root, augmented, leaves, layer.nodes, layer.depth))
            return {false, "verification of Merkle proof failed at layer " + std::to_string(depth)};
        if (augmented.size() > layer.values.size()) return {false, mismatch};
        std::vector<quad> xs(augmented.size()), ys(layer.values.begin(), layer.values.begin() + augmented.size());
        for (size_t i = 0; i < augmented.size(); i++) {
            u128 xe = hf_pow(domain_root, augmented[i]);
            xs[i] = {hf_mul(quartic_roots[0], xe), hf_mul(quartic_roots[1], xe), hf_mul(quartic_roots[2], xe), hf_mul(quartic_roots[3], xe)};
        }
        std::vector<quad> row_polys = quartic_interpolate_batch(xs, ys);
        u128 special_x = fe_to_u128(prng(layer.root.data()));
        evaluations.resize(row_polys.size());
        for (size_t i = 0; i < row_polys.size(); i++) evaluations[i] = quartic_eval(row_polys[i], special_x);
        domain_root = hf_pow(domain_root, 4);
        max_degree_plus_1 /= 4;
        domain_size /= 4;
        positions = augmented;
    }
    for (size_t i = 0; i < positions.size() && i < evaluations.size(); i++)
        if (positions[i] >= proof.rem_values.size() || proof.rem_values[positions[i]] != evaluations[i])
            return {false, "remainder values are inconsistent with values of the last column"};
    return fri_verify_remainder(proof.rem_values, max_degree_plus_1, domain_root, (uint64_t)1 << proof.log_blowup);
}

// ---- stark::verify (verifier.rs:11) -------------------------------------------------------------------------------------------------------
inline VerifyResult verify_proof(const uint8_t program_hash[32], const u128* inputs, size_t num_inputs, const u128* outputs, size_t num_outputs, const VProof& proof) {
    // 1 -- proof of work, query positions (:17-32, proof_of_work.rs:34)
    std::vector<uint8_t> fri_roots;
    for (const VFriLayer& l : proof.layers) fri_roots.insert(fri_roots.end(), l.root.begin(), l.root.end());
    fri_roots.insert(fri_roots.end(), proof.rem_root.begin(), proof.rem_root.end());
    digest seed = hash_bytes(fri_roots.data(), fri_roots.size());
    uint8_t buf[64];
    memset(buf, 0, 64);
    memcpy(buf, seed.data(), 32);
    for (int i = 0; i < 8; i++) buf[32 + i] = (uint8_t)(proof.pow_nonce >> (8 * i));
    digest seed1 = hash_bytes(buf, 64);
    uint64_t w = 0;
    for (int i = 7; i >= 0; i--) w = (w << 8) | seed1[i];
    if ((w == 0 ? 64u : (uint32_t)__builtin_ctzll(w)) < proof.grinding) return {false, "seed proof-of-work verification failed"};
    const uint64_t blowup = (uint64_t)1 << proof.log_blowup, trace_length = proof.trace_length();
    std::vector<uint64_t> t_positions;
    if (query_positions(seed1.data(), proof.domain_size(), (uint32_t)blowup, proof.num_queries, t_positions)) return {false, "could not generate enough query positions"};
    std::vector<uint64_t> c_positions = constraint_positions(t_positions);
    // 2 -- minimum operation count (:35)
    if (proof.op_count < 16) return {false, "Verification of minimum operation count failed"};
    // 3 -- openings of the trace tree (leaf = hash of the row, proof.rs:91) and of the constraint tree (leaf = two evaluations)
    std::vector<digest> row_hashes(proof.trace_evaluations.size());
    for (size_t i = 0; i < row_hashes.size(); i++) row_hashes[i] = hash_bytes((const uint8_t*)proof.trace_evaluations[i].data(), proof.trace_evaluations[i].size() * 16);
    if (!verify_batch(proof.trace_root, t_positions, row_hashes, proof.trace_nodes, proof.domain_depth)) return {false, "verification of trace Merkle proof failed"};
    if (!verify_batch(proof.constraint_root, c_positions, proof.constraint_proof.values, proof.constraint_proof.nodes, proof.constraint_proof.depth))
        return {false, "verification of constraint Merkle proof failed"};
    // 4 -- the constraints at the out-of-domain point z (:79-96)
    u128 z = fe_to_u128(prng(proof.constraint_root.data()));
    hair::Shape sh = {proof.ctx_depth, proof.loop_depth, proof.stack_depth, trace_length};
    const size_t width = 15 + sh.ctx_depth + sh.loop_depth + sh.stack_depth;
    if (proof.trace_at_z1.size() != width || proof.trace_at_z2.size() != width) return {false, "invalid deep values"};
    std::vector<fe> draws_fe(hair::NUM_DRAWS);
    prng_vector(proof.trace_root.data(), hair::NUM_DRAWS, draws_fe.data());
    std::vector<u128> draws(hair::NUM_DRAWS);
    for (size_t i = 0; i < hair::NUM_DRAWS; i++) draws[i] = fe_to_u128(draws_fe[i]);
    hair::Public pub;
    memcpy(pub.program_hash, program_hash, 32);                                                     // evaluator.rs:432
    pub.op_count = proof.op_count; pub.inputs = inputs; pub.num_inputs = num_inputs; pub.outputs = outputs; pub.num_outputs = num_outputs;
    hair::Row s1(sh.ctx_depth, sh.loop_depth, sh.stack_depth, proof.trace_at_z1.data()), s2(sh.ctx_depth, sh.loop_depth, sh.stack_depth, proof.trace_at_z2.data());
    u128 i_value, f_value;
    hair::boundaries_at(sh, draws.data(), pub, s1, z, i_value, f_value);
    u128 t_value = hair::transition_at(sh, draws.data(), s1, s2, z);
    const uint32_t log_n = proof.domain_depth - proof.log_blowup;
    const u128 g_n = hf_root_of_unity(log_n);
    u128 c_at_z = hf_div(i_value, hf_sub(z, 1));
    u128 zz = hf_sub(z, hf_pow(g_n, trace_length - 1));
    c_at_z = hf_add(c_at_z, hf_div(f_value, zz));
    zz = hf_div(hf_sub(hf_pow(z, trace_length), 1), zz);
    c_at_z = hf_add(c_at_z, hf_div(t_value, zz));
    // 5 -- DEEP composition at the queried points (:98-163); draws as coefficients.rs:80-104: z | trace1 x256 | trace2 x256 | t1, t2 degree | constraints
    const size_t num_cc = 1 + 4 * 128 + 3;
    std::vector<fe> cc_fe(num_cc);
    prng_vector(proof.constraint_root.data(), num_cc, cc_fe.data());
    std::vector<u128> cc(num_cc);
    for (size_t i = 0; i < num_cc; i++) cc[i] = fe_to_u128(cc_fe[i]);
    const u128 *cc_trace1 = cc.data() + 1, *cc_trace2 = cc.data() + 257, cc_t1 = cc[513], cc_t2 = cc[514], cc_constraints = cc[515];
    const u128 lde_root = hf_root_of_unity(proof.domain_depth), next_z = hf_mul(z, g_n);
    const u128 incremental_degree = (u128)((hair::MAX_CONSTRAINT_DEGREE - 1) * trace_length - 1 - (trace_length - 2));   // utils/mod.rs:13,20
    if (proof.trace_evaluations.size() != t_positions.size()) return {false, "invalid number of trace evaluations"};
    std::vector<u128> evaluations;
    for (size_t q = 0; q < t_positions.size(); q++) {
        const std::vector<u128>& regs = proof.trace_evaluations[q];
        const uint64_t position = t_positions[q];
        u128 x = hf_pow(lde_root, position);
        u128 inv1 = hf_inv(hf_sub(x, z)), inv2 = hf_inv(hf_sub(x, next_z));                         // one inversion per point, not per register
        u128 comp = 0;
        for (size_t i = 0; i < regs.size() && i < width; i++) {
            comp = hf_add(comp, hf_mul(hf_mul(hf_sub(regs[i], proof.trace_at_z1[i]), inv1), cc_trace1[i]));
            comp = hf_add(comp, hf_mul(hf_mul(hf_sub(regs[i], proof.trace_at_z2[i]), inv2), cc_trace2[i]));
        }
        u128 adj = hf_mul(hf_mul(comp, hf_pow(x, incremental_degree)), cc_t2);
        comp = hf_add(hf_mul(comp, cc_t1), adj);
        size_t leaf = std::find(c_positions.begin(), c_positions.end(), position / 2) - c_positions.begin();
        if (leaf >= proof.constraint_proof.values.size()) return {false, "invalid constraint proof"};
        u128 c_eval;
        memcpy(&c_eval, proof.constraint_proof.values[leaf].data() + (position % 2) * 16, 16);
        evaluations.push_back(hf_add(comp, hf_mul(hf_mul(hf_sub(c_eval, c_at_z), inv1), cc_constraints)));
    }
    // 6 -- low-degree proof
    VerifyResult r = fri_verify(proof, evaluations, t_positions, (hair::MAX_CONSTRAINT_DEGREE - 1) * trace_length - 1);
    if (!r.ok) return {false, "verification of low-degree proof failed: " + r.error};
    return {true, ""};
}

// options.rs:68-79
inline uint32_t security_level(const VProof& p, bool optimistic) {
    uint32_t one_over_rho = ((uint32_t)1 << p.log_blowup) / (uint32_t)hair::MAX_CONSTRAINT_DEGREE;
    uint32_t security_factor = 31 - (uint32_t)__builtin_clz(one_over_rho);
    uint32_t result = security_factor * (optimistic ? p.num_queries : p.num_queries / 2);
    if (result >= 80) result += p.grinding;
    return result;
}

}  // namespace hver
}  // namespace dsth
