// Stand-alone check of the removal plan of distaff_amd/csrc/host/stree_levels.h (stree_plan_remove, beside stree_plan_set) against a brute-force
// std::map model, meant to be built with -fsanitize=address,undefined and run as a program (tests/test_sparse_rescue_tree_remove_host.py).  Node
// values are 64-bit stand-ins as in stree_levels_check.cpp: a leaf is its tag, a parent is mix(left, right) with the level's "empty" constant
// for a missing side.  Every round is a random set, a random removal of stored keys, or the removal without rehashing of the keys that hold the
// empty leaf (what dst_stree_compact does); the plan is applied (carry-over, new leaves, dirty parents bottom-up) and the shape, the carry
// sources, the dirty lists and every node value are compared with the model rebuilt from scratch.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include "host/stree_levels.h"

static uint64_t mix(uint64_t a, uint64_t b) { return (a * 0x9E3779B97F4A7C15ull) ^ (b + 0xC2B2AE3D27D4EB4Full + (a << 7) + (b >> 3)); }
#define CHECK(c) do { if (!(c)) { printf("FAILED %s line %d (round %d depth %u)\n", #c, __LINE__, round_no, depth); return 1; } } while (0)

int main() {
    std::mt19937_64 rng(54321);
    int rounds = 0, removals = 0, compactions = 0, emptied = 0;
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
        for (int round_no = 0; round_no < 30; round_no++, rounds++) {
            const unsigned what = round_no == 0 ? 0 : (unsigned)(rng() % 5);          // 0, 1: set; 2, 3: remove; 4: compact
            stree_plan p;
            std::map<uint64_t, uint64_t> add;
            std::vector<uint64_t> gone;
            if (what < 2) {
                const size_t want = rng() % 40;
                for (size_t i = 0; i < want; i++) {
                    uint64_t k = rng() & mask;
                    const unsigned kind = rng() % 4;
                    if (kind == 1) k = (cluster ^ (rng() & 15)) & mask;
                    if (kind == 2 && !model.empty()) { auto it = model.lower_bound(k); k = it == model.end() ? model.begin()->first : it->first; }
                    if (kind == 3) k = (rng() % 3 == 0) ? 0 : (rng() % 2 ? mask : (k & ~(mask >> 1)));
                    add[k] = rng() % 4 == 0 ? empty[depth] : rng();                   // a key written with the empty value stays stored
                }
                std::vector<uint64_t> keys;
                for (auto& kv : add) keys.push_back(kv.first);
                p = stree_plan_set(shape, keys);
                CHECK(p.dcnt[depth] == keys.size());
            } else {
                if (what == 4) { for (auto& kv : model) if (kv.second == empty[depth]) gone.push_back(kv.first); compactions++; }
                else {
                    const unsigned mode = rng() % 8;                                   // 0: every key; 1: one key; else a random share
                    const uint64_t share = 1 + rng() % 4, one = model.empty() ? 0 : rng() % model.size();
                    uint64_t at = 0;
                    for (auto& kv : model) { if (mode == 0 || (mode == 1 ? at == one : rng() % 5 < share)) gone.push_back(kv.first); at++; }
                    removals++;
                }
                p = stree_plan_remove(shape, gone, what != 4);
                CHECK(p.dcnt[depth] == 0);
                for (uint64_t k : gone) model.erase(k);
                if (model.empty() && !gone.empty()) emptied++;
            }
            CHECK(p.next.depth == depth && p.src.size() == p.next.total() && p.next.pref.size() == p.next.total());
            // the touched prefixes per level: the ancestors of the written / removed keys
            std::vector<std::set<uint64_t>> touched(depth + 1);
            for (uint32_t l = 0; l <= depth; l++) {
                for (auto& kv : add) touched[l].insert(kv.first >> (depth - l));
                for (uint64_t k : gone) touched[l].insert(k >> (depth - l));
            }
            // carry sources: a node that is not written comes from the same prefix of the same level; an untouched node is never written
            uint64_t digests = 0;
            for (uint32_t l = 0; l <= depth; l++) {
                std::vector<uint32_t> want_dirty;
                for (size_t j = p.next.start[l]; j < p.next.start[l] + p.next.cnt[l]; j++) {
                    const uint64_t q = p.next.pref[j];
                    if (j > p.next.start[l]) CHECK(p.next.pref[j - 1] < q);
                    const bool hit = touched[l].count(q) != 0;
                    if (what == 4) CHECK(p.src[j] != STREE_NEW);
                    else CHECK((p.src[j] == STREE_NEW) == hit);
                    if (p.src[j] != STREE_NEW) CHECK(p.src[j] >= shape.start[l] && p.src[j] < shape.start[l] + shape.cnt[l] && shape.pref[p.src[j]] == q);
                    if (hit && what != 4) want_dirty.push_back((uint32_t)j);
                }
                CHECK(p.dcnt[l] == want_dirty.size());
                for (size_t g = 0; g < want_dirty.size(); g++) CHECK(p.dirty[p.doff[l] + g] == want_dirty[g]);
                if (l < depth) digests += want_dirty.size();
            }
            CHECK(p.digests == digests && (what != 4 || p.dirty.empty()));
            // apply: carry over, write the new leaves, hash the dirty parents bottom-up
            std::vector<uint64_t> nv(p.next.total(), 0xDEADDEADDEADDEADull);
            for (size_t j = 0; j < nv.size(); j++) if (p.src[j] != STREE_NEW) nv[j] = val[p.src[j]];
            {
                size_t i = 0;
                for (auto& kv : add) { const uint32_t at = p.dirty[p.doff[depth] + i++]; CHECK(p.next.pref[at] == kv.first); nv[at] = kv.second; }
            }
            for (uint32_t l = depth; l-- > 0;) {
                const size_t cstart = p.next.start[l + 1];
                for (size_t g = 0; g < p.dcnt[l]; g++) {
                    const uint32_t at = p.dirty[p.doff[l] + g];
                    size_t left, right;
                    stree_children(p.next.pref.data() + cstart, p.next.cnt[l + 1], p.next.pref[at], left, right);
                    CHECK(left != STREE_ABSENT || right != STREE_ABSENT);
                    nv[at] = mix(left != STREE_ABSENT ? nv[cstart + left] : empty[l + 1], right != STREE_ABSENT ? nv[cstart + right] : empty[l + 1]);
                }
            }
            shape = p.next; val = nv;
            for (auto& kv : add) model[kv.first] = kv.second;
            // the model from scratch, level by level: the pruned shape and every value
            std::map<uint64_t, uint64_t> level = model;
            for (uint32_t l = depth;; l--) {
                CHECK(shape.cnt[l] == level.size());
                size_t j = shape.start[l];
                for (auto& kv : level) { CHECK(shape.pref[j] == kv.first && val[j] == kv.second); j++; }
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
            if (model.empty()) CHECK(shape.total() == 0);
        }
    }
    if (removals < 500 || compactions < 300 || emptied < 50) { printf("FAILED coverage: %d removals, %d compactions, %d emptied\n", removals, compactions, emptied); return 1; }
    printf("%d rounds ok (%d removals, %d compactions, %d trees emptied)\n", rounds, removals, compactions, emptied);
    return 0;
}
