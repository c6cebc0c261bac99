// Stand-alone check of distaff_amd/csrc/host/stree_levels.h (the bookkeeping of the sparse Rescue trees) against a brute-force std::map model,
// meant to be built with -fsanitize=address,undefined and run as a program (tests/test_sparse_rescue_tree_host.py).  Node values are 64-bit
// stand-ins: a leaf is its tag, a parent is mix(left, right) with the level's "empty" constant for a missing side -- the structure of the real
// tree without the field.  Every round applies a random set through the plan (carry-over, new leaves, dirty parents bottom-up with
// stree_children) and compares every level, and random openings, with the model rebuilt from scratch.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include "host/stree_levels.h"

static uint64_t mix(uint64_t a, uint64_t b) { return (a * 0x9E3779B97F4A7C15ull) ^ (b + 0xC2B2AE3D27D4EB4Full + (a << 7) + (b >> 3)); }
#define CHECK(c) do { if (!(c)) { printf("FAILED %s line %d (round %d depth %u)\n", #c, __LINE__, round_no, depth); return 1; } } while (0)

int main() {
    std::mt19937_64 rng(12345);
    int rounds = 0;
    for (int tree_no = 0; tree_no < 160; tree_no++) {
        const uint32_t depth = tree_no < 8 ? 1 + tree_no : tree_no % 5 == 0 ? 63 : 1 + (uint32_t)(rng() % 63);
        const uint64_t mask = depth == 63 ? ((uint64_t)1 << 63) - 1 : ((uint64_t)1 << depth) - 1;
        uint64_t empty[64];
        empty[depth] = rng();
        for (uint32_t l = depth; l-- > 0;) empty[l] = mix(empty[l + 1], empty[l + 1]);
        stree_shape shape;
        shape.depth = depth;
        std::vector<uint64_t> val;                                   // node values at the shape's flat positions
        std::map<uint64_t, uint64_t> model;
        const uint64_t cluster = rng() & mask;
        for (int round_no = 0; round_no < 25; round_no++, rounds++) {
            // a set: random keys, keys near a cluster (shared prefixes), keys stored already; distinct by construction of the map
            std::map<uint64_t, uint64_t> add;
            const size_t want = rng() % 40;
            for (size_t i = 0; i < want; i++) {
                uint64_t k = rng() & mask;
                const unsigned kind = rng() % 4;
                if (kind == 1) k = (cluster ^ (rng() & 15)) & mask;
                if (kind == 2 && !model.empty()) { auto it = model.lower_bound(k); k = it == model.end() ? model.begin()->first : it->first; }
                if (kind == 3) k = (rng() % 3 == 0) ? 0 : (rng() % 2 ? mask : (k & ~(mask >> 1)));
                add[k] = rng();
            }
            std::vector<uint64_t> keys;
            for (auto& kv : add) keys.push_back(kv.first);
            uint64_t expect_digests = 0;
            for (uint32_t l = 0; l < depth; l++) {
                std::vector<uint64_t> q;
                for (uint64_t k : keys) q.push_back(k >> (depth - l));
                q.erase(std::unique(q.begin(), q.end()), q.end());
                expect_digests += q.size();
            }
            const stree_plan p = stree_plan_set(shape, keys);
            CHECK(p.digests == expect_digests);
            CHECK(p.src.size() == p.next.total() && p.dcnt[depth] == keys.size());
            std::vector<uint64_t> nv(p.next.total(), 0xDEADDEADDEADDEADull);
            for (size_t j = 0; j < nv.size(); j++) if (p.src[j] != STREE_NEW) { CHECK(p.src[j] < val.size()); nv[j] = val[p.src[j]]; }
            for (size_t i = 0; i < keys.size(); i++) {
                const uint32_t at = p.dirty[p.doff[depth] + i];
                CHECK(at >= p.next.start[depth] && at < p.next.start[depth] + p.next.cnt[depth] && p.next.pref[at] == keys[i] && p.src[at] == STREE_NEW);
                nv[at] = add[keys[i]];
            }
            for (uint32_t l = depth; l-- > 0;) {
                const size_t cstart = p.next.start[l + 1];
                for (size_t g = 0; g < p.dcnt[l]; g++) {
                    const uint32_t at = p.dirty[p.doff[l] + g];
                    CHECK(at >= p.next.start[l] && at < p.next.start[l] + p.next.cnt[l] && p.src[at] == STREE_NEW);
                    size_t left, right;
                    stree_children(p.next.pref.data() + cstart, p.next.cnt[l + 1], p.next.pref[at], left, right);
                    CHECK(left != STREE_ABSENT || right != STREE_ABSENT);
                    nv[at] = mix(left != STREE_ABSENT ? nv[cstart + left] : empty[l + 1], right != STREE_ABSENT ? nv[cstart + right] : empty[l + 1]);
                }
            }
            shape = p.next; val = nv;
            for (auto& kv : add) model[kv.first] = kv.second;
            // the model from scratch, level by level
            std::map<uint64_t, uint64_t> level = model;
            for (uint32_t l = depth;; l--) {
                CHECK(shape.cnt[l] == level.size());
                size_t j = shape.start[l];
                for (auto& kv : level) { CHECK(shape.pref[j] == kv.first && val[j] == kv.second); j++; }
                // lookups: every stored prefix is found where it is, neighbours that are not stored are absent
                for (auto& kv : level) {
                    CHECK(stree_find(shape.pref.data() + shape.start[l], shape.cnt[l], kv.first) != STREE_ABSENT);
                    if (!level.count(kv.first ^ 1)) CHECK(stree_find(shape.pref.data() + shape.start[l], shape.cnt[l], kv.first ^ 1) == STREE_ABSENT);
                }
                if (l == 0) break;
                std::map<uint64_t, uint64_t> up;
                for (auto& kv : level) {
                    const uint64_t q = kv.first >> 1;
                    if (up.count(q)) continue;
                    auto a = level.find(2 * q), b = level.find(2 * q + 1);
                    up[q] = mix(a != level.end() ? a->second : empty[l], b != level.end() ? b->second : empty[l]);
                }
                level.swap(up);
            }
            // openings of present and absent keys: the slots' levels and prefixes walk up the tree, and fold to the root
            for (int o = 0; o < 6; o++) {
                uint64_t index = rng() & mask;
                if (o < 3 && !model.empty()) { auto it = model.lower_bound(index); if (it != model.end()) index = it->first; }
                uint64_t v = 0, idx = index;
                for (uint32_t k = 0; k <= depth; k++) {
                    uint32_t l; uint64_t prefix;
                    stree_path_slot(depth, index, k, l, prefix);
                    CHECK(l <= depth && (k == 0 ? l == depth && prefix == index : l == depth - (k - 1) && prefix == (idx ^ 1)));
                    const size_t pos = stree_find(shape.pref.data() + shape.start[l], shape.cnt[l], prefix);
                    const uint64_t node = pos != STREE_ABSENT ? val[shape.start[l] + pos] : empty[l];
                    if (k == 0) { v = node; CHECK(node == (model.count(index) ? model[index] : empty[depth])); continue; }
                    v = (idx & 1) ? mix(node, v) : mix(v, node);
                    idx >>= 1;
                }
                CHECK(v == (shape.cnt[0] ? val[shape.start[0]] : empty[0]));
            }
        }
    }
    printf("%d rounds ok\n", rounds);
    return 0;
}
