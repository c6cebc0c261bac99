// Stand-alone check of the parser of saved trees, distaff_amd/csrc/host/tree_blob.h, meant to be built with -fsanitize=address,undefined and run
// as a program (tests/test_rescue_tree_restore_host.py).  The parser takes untrusted bytes, so every blob here lives in a heap buffer of exactly
// its length: a read past the end is a sanitizer report.  Sparse blobs are made from random key sets by a std::set model (level l = the distinct
// key >> (depth - l)) and must parse to exactly those levels; each malformed variant of them must be refused with the text of its own check;
// and blobs with random damage -- bytes changed, cut short, grown -- must be refused or accepted without a report, an accepted one having
// levels that the model's rule confirms.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>
#include "host/tree_blob.h"

typedef std::vector<std::vector<uint64_t>> levels_t;                 // the leaf level first

static std::vector<uint8_t> make_sparse(uint32_t depth, const levels_t& lv, std::mt19937_64& rng, int64_t keys = -1, int64_t nodes = -1) {
    size_t total = 0;
    for (auto& l : lv) total += l.size();
    std::vector<uint8_t> b(TBLOB_HEADER + 8 * lv.size() + 40 * total);
    uint8_t empty[32] = {7};
    tblob_put_header(b.data(), TBLOB_SPARSE, depth, empty, keys < 0 ? lv[0].size() : (uint64_t)keys, nodes < 0 ? total : (uint64_t)nodes);
    uint8_t* at = b.data() + TBLOB_HEADER;
    for (auto& l : lv) { tblob_put_u64(at, l.size()); at += 8; }
    for (auto& l : lv) for (uint64_t q : l) { tblob_put_u64(at, q); at += 8; }
    for (size_t j = 0; j < total; j++, at += 32) { tblob_put_u64(at, rng()); tblob_put_u64(at + 8, rng() >> 1); tblob_put_u64(at + 16, rng()); tblob_put_u64(at + 24, rng() >> 1); }
    return b;
}
static levels_t model_levels(uint32_t depth, const std::set<uint64_t>& keys) {
    levels_t lv;
    std::set<uint64_t> cur = keys;
    for (uint32_t l = depth;; l--) {
        lv.emplace_back(cur.begin(), cur.end());
        if (l == 0) break;
        std::set<uint64_t> up;
        for (uint64_t q : cur) up.insert(q >> 1);
        cur.swap(up);
    }
    return lv;
}
// the parser's verdict on bytes held in a heap block of exactly their length
static const char* parse(const std::vector<uint8_t>& b, uint32_t kind, tblob_view& v, std::unique_ptr<uint8_t[]>& hold) {
    hold.reset(new uint8_t[b.size() ? b.size() : 1]);
    if (!b.empty()) memcpy(hold.get(), b.data(), b.size());
    return tblob_parse(hold.get(), b.size(), kind, v);
}
static bool is_model(const tblob_view& v) {                           // an accepted sparse blob has the levels of its own leaf level
    std::set<uint64_t> keys;
    const uint64_t n = tblob_u64(v.counts);
    for (uint64_t i = 0; i < n; i++) keys.insert(tblob_u64(v.prefixes + 8 * i));
    if (keys.size() != n || n != v.keys) return false;
    const levels_t lv = model_levels(v.depth, keys);
    const uint8_t* at = v.prefixes;
    uint64_t total = 0;
    for (uint32_t k = 0; k <= v.depth; k++) {
        if (tblob_u64(v.counts + 8 * k) != lv[k].size()) return false;
        for (uint64_t q : lv[k]) { if (tblob_u64(at) != q || (v.depth - k < 64 && (q >> (v.depth - k)))) return false; at += 8; }
        total += lv[k].size();
    }
    return total == v.nodes;
}
#define CHECK(c) do { if (!(c)) { printf("FAILED %s line %d (blob %d)\n", #c, __LINE__, blobs); return 1; } } while (0)
#define REFUSED(bytes, kind, word) do { const char* why_ = parse(bytes, kind, v, hold); if (!why_ || !strstr(why_, word)) { printf("FAILED line %d (blob %d): wanted '%s', got '%s'\n", __LINE__, blobs, word, why_ ? why_ : "accepted"); return 1; } } while (0)

int main() {
    std::mt19937_64 rng(20240);
    int blobs = 0, damaged = 0, accepted_damaged = 0;
    tblob_view v;
    std::unique_ptr<uint8_t[]> hold;
    for (int tree_no = 0; tree_no < 300; tree_no++, blobs++) {
        const uint32_t depth = tree_no < 8 ? 1 + tree_no : tree_no % 5 == 0 ? 63 : 1 + (uint32_t)(rng() % 63);
        const uint64_t mask = ((uint64_t)1 << depth) - 1;
        std::set<uint64_t> keys;
        const size_t want = tree_no % 7 == 0 ? 0 : 1 + rng() % 30;
        const uint64_t cluster = rng() & mask;
        for (size_t i = 0; i < want; i++) keys.insert(rng() % 3 ? rng() & mask : (cluster ^ (rng() & 7)) & mask);
        const levels_t lv = model_levels(depth, keys);
        const std::vector<uint8_t> good = make_sparse(depth, lv, rng);
        CHECK(parse(good, TBLOB_SPARSE, v, hold) == nullptr);
        CHECK(v.depth == depth && v.keys == keys.size() && is_model(v) && v.values + 32 * v.nodes == hold.get() + good.size());
        REFUSED(good, TBLOB_DENSE, "not a dense one");
        // the header and the length
        std::vector<uint8_t> b = good;
        b.pop_back(); REFUSED(b, TBLOB_SPARSE, "truncated");
        b = good; b.push_back(0); REFUSED(b, TBLOB_SPARSE, "after the end");
        b.assign(good.begin(), good.begin() + 63); REFUSED(b, TBLOB_SPARSE, "header");
        b.clear(); REFUSED(b, TBLOB_SPARSE, "header");
        b = good; b[3] ^= 0x20; REFUSED(b, TBLOB_SPARSE, "magic");
        b = good; b[7] = '0'; REFUSED(b, TBLOB_SPARSE, "version");
        b = good; tblob_put_u32(b.data() + 8, 7); REFUSED(b, TBLOB_SPARSE, "unknown kind");
        b = good; tblob_put_u32(b.data() + 12, 0); REFUSED(b, TBLOB_SPARSE, "1 .. 63");
        b = good; tblob_put_u32(b.data() + 12, 64 + (uint32_t)(rng() % 1000)); REFUSED(b, TBLOB_SPARSE, "1 .. 63");
        b = good; memset(b.data() + 32, 0xFF, 16); REFUSED(b, TBLOB_SPARSE, "empty leaf");
        b = good; tblob_put_u64(b.data() + 56, 0xFFFFFFFFull + rng() % 3); REFUSED(b, TBLOB_SPARSE, "2^32 - 2");
        b = good; tblob_put_u64(b.data() + 56, ~(uint64_t)0 / 40 + 1); REFUSED(b, TBLOB_SPARSE, "2^32 - 2");       // 40 * nodes would wrap
        if (keys.empty()) {
            REFUSED(make_sparse(depth, lv, rng, 1), TBLOB_SPARSE, "key count");
            continue;
        }
        b = good; memset(b.data() + b.size() - 16, 0xFF, 16); REFUSED(b, TBLOB_SPARSE, "node element");
        b = good; tblob_put_u64(b.data() + b.size() - 32, 0xFFFFD30000000001ull); tblob_put_u64(b.data() + b.size() - 24, ~(uint64_t)0); REFUSED(b, TBLOB_SPARSE, "node element");
        b = good; tblob_put_u64(b.data() + b.size() - 32, 0xFFFFD30000000000ull); tblob_put_u64(b.data() + b.size() - 24, ~(uint64_t)0); CHECK(parse(b, TBLOB_SPARSE, v, hold) == nullptr);      // p - 1
        REFUSED(make_sparse(depth, lv, rng, (int64_t)keys.size() + 1), TBLOB_SPARSE, "key count");
        // the shape: one level damaged at a time
        const size_t k = rng() % (depth + 1);                                // run k is level depth - k
        levels_t bad = lv;
        bad[k].push_back(bad[k].back()); REFUSED(make_sparse(depth, bad, rng), TBLOB_SPARSE, k == depth ? "more than one root" : "stored twice");
        if (lv[k].size() > 1) { bad = lv; std::swap(bad[k][0], bad[k][1]); REFUSED(make_sparse(depth, bad, rng), TBLOB_SPARSE, "do not ascend"); }
        bad = lv; bad[k].back() |= (uint64_t)1 << (depth - k); REFUSED(make_sparse(depth, bad, rng), TBLOB_SPARSE, "not below 2^level");
        if (k > 0) {
            bad = lv; bad[k].pop_back(); REFUSED(make_sparse(depth, bad, rng), TBLOB_SPARSE, "lacks the parent");
            const uint64_t top = ((uint64_t)1 << (depth - k)) - 1;            // a prefix nobody is below: one past the last, when the level has room
            if (lv[k].back() < top) { bad = lv; bad[k].push_back(lv[k].back() + 1); REFUSED(make_sparse(depth, bad, rng), TBLOB_SPARSE, k == depth ? "more than one root" : "nothing below it"); }
            if (lv[k].front() > 0) { bad = lv; bad[k].insert(bad[k].begin(), lv[k].front() - 1); REFUSED(make_sparse(depth, bad, rng), TBLOB_SPARSE, "nothing below it"); }
        }
        const uint64_t total = (good.size() - TBLOB_HEADER - 8 * (depth + 1)) / 40;      // the header's node count lies, the length agrees with the lie
        REFUSED(make_sparse(depth, lv, rng, -1, (int64_t)total + 1), TBLOB_SPARSE, "truncated");
        { std::vector<uint8_t> c = make_sparse(depth, lv, rng, -1, (int64_t)total - 1); c.resize(tblob_sparse_bytes(depth, total - 1)); REFUSED(c, TBLOB_SPARSE, "level counts"); }
        { std::vector<uint8_t> c = make_sparse(depth, lv, rng, -1, (int64_t)total + 1); c.resize(tblob_sparse_bytes(depth, total + 1)); REFUSED(c, TBLOB_SPARSE, "level counts"); }
        // random damage: never a report; what is accepted is a tree
        for (int d = 0; d < 40; d++, damaged++) {
            b = good;
            const unsigned what = rng() % 4;
            if (what == 0) b.resize(rng() % (b.size() + 1));
            else if (what == 1) b.resize(b.size() + 1 + rng() % 64, (uint8_t)rng());
            else for (unsigned n = 1 + rng() % 3; n--;) b[rng() % (what == 2 ? b.size() : TBLOB_HEADER + 8 * (depth + 1))] ^= (uint8_t)(1u << (rng() % 8));
            if (parse(b, TBLOB_SPARSE, v, hold) == nullptr) { accepted_damaged++; CHECK(is_model(v) && tblob_below_p(v.values, 2 * v.nodes) && v.values + 32 * v.nodes == hold.get() + b.size()); }
        }
    }
    // dense blobs
    for (uint32_t log_leaves = 1; log_leaves <= 10; log_leaves++, blobs++) {
        std::vector<uint8_t> good(tblob_dense_bytes(log_leaves));
        const uint64_t nodes = ((uint64_t)2 << log_leaves) - 1;
        tblob_put_header(good.data(), TBLOB_DENSE, log_leaves, nullptr, (uint64_t)1 << log_leaves, nodes);
        for (uint64_t j = 0; j < 2 * nodes; j++) { tblob_put_u64(good.data() + TBLOB_HEADER + 16 * j, rng()); tblob_put_u64(good.data() + TBLOB_HEADER + 16 * j + 8, rng() >> 1); }
        CHECK(parse(good, TBLOB_DENSE, v, hold) == nullptr && v.depth == log_leaves && v.nodes == nodes && v.values == hold.get() + TBLOB_HEADER);
        REFUSED(good, TBLOB_SPARSE, "not a sparse one");
        std::vector<uint8_t> b = good;
        b.pop_back(); REFUSED(b, TBLOB_DENSE, "truncated");
        b = good; b.push_back(1); REFUSED(b, TBLOB_DENSE, "after the end");
        b = good; tblob_put_u32(b.data() + 12, 0); REFUSED(b, TBLOB_DENSE, "1 .. 26");
        b = good; tblob_put_u32(b.data() + 12, 27); REFUSED(b, TBLOB_DENSE, "1 .. 26");
        b = good; tblob_put_u32(b.data() + 12, log_leaves + 1); REFUSED(b, TBLOB_DENSE, "counts disagree");
        b = good; tblob_put_u64(b.data() + 48, 3); REFUSED(b, TBLOB_DENSE, "counts disagree");
        b = good; b[47] = 1; REFUSED(b, TBLOB_DENSE, "no empty leaf");
        b = good; memset(b.data() + TBLOB_HEADER + 16 * (rng() % (2 * nodes)), 0xFF, 16); REFUSED(b, TBLOB_DENSE, "node element");
        for (int d = 0; d < 40; d++, damaged++) {
            b = good;
            if (rng() % 2) b.resize(rng() % (b.size() + 8)); else b[rng() % TBLOB_HEADER] ^= (uint8_t)(1u << (rng() % 8));
            if (parse(b, TBLOB_DENSE, v, hold) == nullptr) { accepted_damaged++; CHECK(b.size() == tblob_dense_bytes(v.depth)); }
        }
    }
    printf("%d blobs ok (%d damaged variants, %d of them still trees)\n", blobs, damaged, accepted_damaged);
    return 0;
}
