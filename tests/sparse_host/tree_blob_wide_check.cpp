// The kind-3 parser of host/tree_blob.h (16-byte prefixes, depth <= 127) alone, against a model: the levels of random key sets are std::set of
// (level, prefix) with prefix = key >> (depth - level) over unsigned __int128; their blobs must parse with the pointers where the layout puts them;
// variants that are wrong in one place -- also in the high half of a prefix only -- must be refused with their own text; and random damage must
// never read out of bounds (the sanitizers watch).  Built with sanitizers by tests/test_wide_tree_restore_host.py.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>
#include "host/tree_blob.h"

typedef unsigned __int128 u128;
static void put_u128(uint8_t* p, u128 v) { tblob_put_u64(p, (uint64_t)v); tblob_put_u64(p + 8, (uint64_t)(v >> 64)); }

static std::vector<uint8_t> make_blob(uint32_t depth, const std::set<u128>& keys, std::vector<std::vector<u128>>* out_levels = nullptr) {
    std::vector<std::vector<u128>> levels;               // the leaf level first
    std::set<u128> cur = keys;
    for (uint32_t l = depth;; l--) {
        levels.emplace_back(cur.begin(), cur.end());
        if (l == 0) break;
        std::set<u128> up;
        for (u128 q : cur) up.insert(q >> 1);
        cur.swap(up);
    }
    size_t total = 0;
    for (auto& lv : levels) total += lv.size();
    std::vector<uint8_t> b((size_t)tblob_wide_bytes(depth, total), 0);
    uint8_t empty[32] = {7};
    tblob_put_header(b.data(), TBLOB_WIDE, depth, empty, keys.size(), total);
    uint8_t* at = b.data() + TBLOB_HEADER;
    for (auto& lv : levels) { tblob_put_u64(at, lv.size()); at += 8; }
    for (auto& lv : levels) for (u128 q : lv) { put_u128(at, q); at += 16; }
    for (size_t j = 0; j < total; j++, at += 32) at[0] = (uint8_t)j;
    if (out_levels) *out_levels = levels;
    return b;
}
#define REFUSED(b, text) do { tblob_view v_; const char* why_ = tblob_parse((b).data(), (b).size(), TBLOB_WIDE, v_); \
    if (!why_ || std::string(why_).find(text) == std::string::npos) { printf("line %d: expected \"%s\", got \"%s\"\n", __LINE__, text, why_ ? why_ : "(accepted)"); return 1; } } while (0)

int main() {
    std::mt19937_64 rng(3);
    size_t ok = 0;
    for (int round = 0; round < 300; round++) {
        const uint32_t depths[] = {1, 2, 7, 63, 64, 65, 100, 127};
        const uint32_t depth = depths[round % 8];
        const u128 mask = (((u128)1 << (depth - 1)) << 1) - 1;
        std::set<u128> keys;
        const size_t count = depth < 7 ? rng() % 3 : rng() % 30;
        for (size_t i = 0; i < count; i++) {
            const u128 k = (((u128)rng() << 64) | rng()) & mask;
            keys.insert(k);
            if (depth > 64 && rng() % 2) keys.insert(k ^ ((u128)1 << 64));       // equal low halves
            if (rng() % 2) keys.insert(k ^ 1);
        }
        std::vector<std::vector<u128>> levels;
        std::vector<uint8_t> good = make_blob(depth, keys, &levels);
        tblob_view v;
        const char* why = tblob_parse(good.data(), good.size(), TBLOB_WIDE, v);
        if (why) { printf("round %d: a good blob was refused: %s\n", round, why); return 1; }
        size_t total = 0;
        for (auto& lv : levels) total += lv.size();
        if (v.depth != depth || v.keys != keys.size() || v.nodes != total || v.counts != good.data() + 64 || v.prefixes != v.counts + 8 * (depth + 1) || v.values != v.prefixes + 16 * total) {
            printf("round %d: the view is not the layout\n", round); return 1;
        }
        {                                                // the narrow loader does not know the kind; the wide one refuses the other kinds
            tblob_view w;
            const char* r = tblob_parse(good.data(), good.size(), TBLOB_SPARSE, w);
            if (!r || std::string(r).find("unknown kind") == std::string::npos) { printf("kind 3 was not refused by the narrow parser\n"); return 1; }
            std::vector<uint8_t> b = good;
            tblob_put_u32(b.data() + 8, TBLOB_SPARSE); REFUSED(b, "8-byte keys");
            tblob_put_u32(b.data() + 8, TBLOB_DENSE); REFUSED(b, "dense tree");
            tblob_put_u32(b.data() + 8, 4); REFUSED(b, "unknown kind");
        }
        std::vector<uint8_t> b = good;
        b.pop_back(); REFUSED(b, "truncated");
        b = good; b.push_back(0); REFUSED(b, "after the end");
        b = good; tblob_put_u32(b.data() + 12, 128); REFUSED(b, "1 .. 127");
        if (keys.size() >= 2 && depth > 64) {
            uint8_t* leaf = b.data() + 64 + 8 * (depth + 1);
            b = good; leaf = b.data() + 64 + 8 * (depth + 1);
            put_u128(leaf + 16 * (keys.size() - 1), levels[0].back() | ((u128)1 << depth)); REFUSED(b, "below 2^level");      // wrong in the high half only
            b = good; leaf = b.data() + 64 + 8 * (depth + 1);
            put_u128(leaf, levels[0][1]); REFUSED(b, "stored twice");
            b = good; leaf = b.data() + 64 + 8 * (depth + 1);
            put_u128(leaf, levels[0][1]); put_u128(leaf + 16, levels[0][0]); REFUSED(b, "do not ascend");
            uint8_t* parents = leaf + 16 * keys.size();
            b = good; parents = b.data() + 64 + 8 * (depth + 1) + 16 * keys.size();
            put_u128(parents, levels[1][0] ^ ((u128)1 << 64));                    // a parent wrong in the high half only
            { tblob_view v_; if (!tblob_parse(b.data(), b.size(), TBLOB_WIDE, v_)) { printf("round %d: a parent wrong in its high half was accepted\n", round); return 1; } }
        }
        for (int hit = 0; hit < 20; hit++) {             // random damage: any verdict, no fault
            b = good;
            for (int k = 0; k < 1 + hit % 3; k++) b[rng() % b.size()] ^= (uint8_t)(1u << (rng() % 8));
            if (hit % 5 == 0) b.resize(rng() % (b.size() + 1));
            tblob_view v_;
            (void)tblob_parse(b.data(), b.size(), TBLOB_WIDE, v_);
        }
        ok++;
    }
    printf("%zu blobs ok\n", ok);
    return 0;
}
