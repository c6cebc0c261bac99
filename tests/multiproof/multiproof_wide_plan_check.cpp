// host/multiproof_plan.h alone over stree_wide positions, against a model over std::set / std::map of (level, 128-bit position).  Plain form: the
// checks of multiproof_plan_check.cpp at depths where a position crosses the two halves.  With known-empty flags -- random bits for the supplied
// nodes, random flags for the leaves, and the extremes all / none -- the model states the rule (a parent is known-empty exactly when both
// children are) and the plan must make exactly one job for every member of every K_l that is not, read E-table entries exactly where a child is
// known-empty, name the table in `where` for such path nodes, count the shipped nodes, and end in the root (E_0's entry when there is no job).
// mp_count's histogram is exercised to 128 bit lengths.  Built with sanitizers by tests/test_wide_multiproof_host.py.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <utility>
#include "host/multiproof_plan.h"

typedef unsigned __int128 u128;
typedef std::pair<uint32_t, u128> node_id;
static size_t checked = 0;
#define REQUIRE(c) do { if (!(c)) { printf("line %d: %s (depth %u, %zu indices, mode %d)\n", __LINE__, #c, depth, idx.size(), mode); exit(1); } } while (0)

static stree_wide wide(u128 v) { return stree_wide{(uint64_t)v, (uint64_t)(v >> 64)}; }
static u128 narrow(const stree_wide& w) { return ((u128)w.hi << 64) | w.lo; }

// mode 0: plain (no bits); 1: random flags; 2: everything known-empty; 3: bits given, none set
static void check(uint32_t depth, const std::vector<u128>& idx, int mode, std::mt19937_64& rng) {
    const size_t count = idx.size(), n = depth + 1;
    std::vector<stree_wide> in(count);
    for (size_t i = 0; i < count; i++) in[i] = wide(idx[i]);
    // the definition: the supplied positions, and who is known-empty
    std::vector<node_id> want;
    std::vector<std::map<u128, bool>> ke(depth + 1);
    std::vector<uint8_t> leaf_empty(count, 0);
    for (size_t i = 0; i < count; i++) { leaf_empty[i] = mode == 2 || (mode == 1 && rng() % 2); ke[depth][idx[i]] = mode != 0 && leaf_empty[i]; }
    std::vector<uint8_t> flag;                            // per supplied node: absent
    for (uint32_t l = depth; l >= 1; l--) {
        for (auto& kv : ke[l]) {
            const u128 p = kv.first;
            bool other;
            if (ke[l].count(p ^ 1)) { if (p & 1) continue; other = ke[l][p ^ 1]; }
            else { want.push_back({l, p ^ 1}); flag.push_back(mode == 2 || (mode == 1 && rng() % 3 != 0)); other = mode != 0 && flag.back(); }
            ke[l - 1][p >> 1] = kv.second && other;
        }
    }
    const size_t M = want.size();
    std::vector<uint8_t> bits((M + 7) / 8 + 1, 0);
    size_t shipped = 0;
    for (size_t m = 0; m < M; m++) { if (mode != 0 && flag[m]) bits[m >> 3] |= (uint8_t)(1u << (m & 7)); else shipped++; }
    uint64_t digests = 0;
    for (uint32_t l = 0; l < depth; l++) for (auto& kv : ke[l]) digests += kv.second ? 0 : 1;
    {                                                    // the sizes alone: the histogram over up to 128 bit lengths
        mp_plan_t<stree_wide> p;
        REQUIRE(mp_plan_make(depth, in.data(), count, MP_SUPPLIED, p) == nullptr);
        uint64_t all = 0;
        for (uint32_t l = 0; l < depth; l++) all += ke[l].size();
        REQUIRE(p.sizes.nodes == M && p.sizes.digests == all && p.spos.size() == M);
        for (size_t m = 0; m < M; m++) REQUIRE(node_id(p.slevel[m], narrow(p.spos[m])) == want[m]);
    }
    mp_plan_t<stree_wide> p;
    REQUIRE(mp_plan_make(depth, in.data(), count, MP_SUPPLIED | MP_JOBS | MP_WHERE, p, mode ? bits.data() : nullptr, mode ? leaf_empty.data() : nullptr) == nullptr);
    REQUIRE(p.sizes.nodes == M && p.shipped == shipped && p.sizes.digests == digests && p.table == (mode ? n : 0));
    REQUIRE(p.inputs() == count + shipped + p.table && p.pool() == p.inputs() + digests && p.jobs.size() == 3 * digests);
    std::map<uint32_t, node_id> id;                      // pool index -> what it holds; table entries apart
    for (size_t i = 0; i < count; i++) id[(uint32_t)i] = {depth, idx[i]};
    for (size_t m = 0, s = 0; m < M; m++) if (!(mode != 0 && flag[m])) id[(uint32_t)(count + s++)] = want[m];
    auto table_level = [&](uint32_t ref, uint32_t& l) { if (!p.table || ref < count + shipped || ref >= p.inputs()) return false; l = ref - (uint32_t)(count + shipped); return true; };
    size_t next = 0;
    uint32_t levels = 0;
    for (uint32_t l = depth; l-- > 0;) {
        size_t expect = 0;
        for (auto& kv : ke[l]) expect += kv.second ? 0 : 1;
        REQUIRE(p.joff[l] == next && p.jcnt[l] == expect);
        levels += expect ? 1 : 0;
        std::map<uint32_t, node_id> made;
        for (size_t g = 0; g < p.jcnt[l]; g++) {
            const uint32_t* j = p.jobs.data() + 3 * (next + g);
            REQUIRE(j[2] == p.inputs() + next + g && !id.count(j[2]));
            uint32_t tl = 0;
            bool have = false;
            u128 parent = 0;
            for (int side = 0; side < 2; side++) {
                if (table_level(j[side], tl)) continue;
                REQUIRE(id.count(j[side]));
                const node_id c = id[j[side]];
                REQUIRE(c.first == l + 1 && (c.second & 1) == (u128)side);
                REQUIRE(!have || parent == c.second >> 1);
                parent = c.second >> 1; have = true;
            }
            REQUIRE(have);                               // a job of two table entries would be a parent of two empty subtrees
            REQUIRE(ke[l].count(parent) && !ke[l][parent]);
            for (int side = 0; side < 2; side++) {       // a side reads the table exactly where the model knows the child to be empty
                const u128 c = 2 * parent + side;
                const bool member = ke[l + 1].count(c) != 0;
                bool empty = false;
                if (member) empty = ke[l + 1][c];
                else { for (size_t m = 0; m < M; m++) if (want[m] == node_id(l + 1, c)) empty = mode != 0 && flag[m]; }
                if (table_level(j[side], tl)) REQUIRE(tl == l + 1 && empty);
                else REQUIRE(!empty || (member && l + 1 == depth));      // a leaf that is known-empty by value may stand for itself
            }
            REQUIRE(!made.count(j[2]));
            made[j[2]] = {l, parent};
        }
        std::set<node_id> distinct;
        for (auto& kv : made) distinct.insert(kv.second);
        REQUIRE(distinct.size() == expect);
        id.insert(made.begin(), made.end());
        next += p.jcnt[l];
    }
    REQUIRE(p.levels == levels);
    if (digests) REQUIRE(p.root == p.pool() - 1 && id[p.root] == node_id(0, 0));
    else REQUIRE(mode != 0 && p.root == p.empty_at(0));
    REQUIRE(p.where.size() == count * n);
    for (size_t i = 0; i < count; i++) {
        uint32_t tl = 0;
        if (table_level(p.where[i * n], tl)) REQUIRE(tl == depth && leaf_empty[i]); else REQUIRE(p.where[i * n] == i);
        for (size_t k = 1; k < n; k++) {
            const uint32_t l = (uint32_t)(depth - k + 1);
            const u128 c = (idx[i] >> (k - 1)) ^ 1;
            const uint32_t ref = p.where[i * n + k];
            if (table_level(ref, tl)) {
                REQUIRE(tl == l);
                bool empty = false;
                if (ke[l].count(c)) empty = ke[l][c];
                else { for (size_t m = 0; m < M; m++) if (want[m] == node_id(l, c)) empty = flag[m]; }
                REQUIRE(empty);
            } else REQUIRE(id.count(ref) && id[ref] == node_id(l, c));
        }
    }
    checked++;
}

int main() {
    std::mt19937_64 rng(11);
    auto random_key = [&](uint32_t depth) { u128 v = ((u128)rng() << 64) | rng(); return depth == 128 ? v : v & (((u128)1 << depth) - 1); };
    for (uint32_t depth = 1; depth <= 3; depth++)        // every subset of the small depths, every mode
        for (uint32_t mask = 1; mask < (1u << (1u << depth)); mask++) {
            std::vector<u128> idx;
            for (uint32_t i = 0; i < (1u << depth); i++) if (mask >> i & 1) idx.push_back(i);
            for (int mode = 0; mode < 4; mode++) check(depth, idx, mode, rng);
            std::shuffle(idx.begin(), idx.end(), rng);
            for (int mode = 0; mode < 4; mode++) check(depth, idx, mode, rng);
        }
    for (int round = 0; round < 200; round++) {
        const uint32_t depths[] = {5, 12, 63, 64, 65, 66, 100, 126, 127};
        const uint32_t depth = depths[round % 9];
        std::set<u128> s;
        const size_t count = 1 + rng() % (depth == 5 ? 12 : 40);      // well below the 32 keys of depth 5
        while (s.size() < count) {
            const u128 k = random_key(depth);
            s.insert(k);
            if (rng() % 2) s.insert(k ^ ((u128)1 << (rng() % depth)));      // a relative that differs in one bit: shared ancestors at every height
            if (depth > 64 && rng() % 4 == 0) s.insert(k ^ ((u128)1 << 64)); // equal low halves
        }
        if (round % 7 == 0) { s.insert(0); s.insert((((u128)1 << (depth - 1)) << 1) - 1); }
        std::vector<u128> idx(s.begin(), s.end());
        std::shuffle(idx.begin(), idx.end(), rng);
        for (int mode = 0; mode < 4; mode++) check(depth, idx, mode, rng);
    }
    {                                                    // what is refused
        const uint32_t depth = 127; const int mode = 0;
        std::vector<u128> idx = {5, ((u128)1 << 64) | 5, 5};
        mp_plan_t<stree_wide> p;
        const stree_wide twice[3] = {wide(idx[0]), wide(idx[1]), wide(idx[2])};
        REQUIRE(mp_plan_make(127, twice, 3, MP_JOBS, p) != nullptr);
        REQUIRE(mp_plan_make(127, twice, 2, MP_JOBS, p) == nullptr);     // equal low halves are two keys
        const size_t M = (size_t)p.sizes.nodes;
        REQUIRE(M == 190);                               // two supplied nodes on each of the 64 levels below the fork, one on each of the 62 above
        std::vector<uint8_t> padded((M + 7) / 8, 0);
        padded.back() = 0x80;                            // bit 191: padding
        const char* why = mp_plan_make(127, twice, 2, MP_JOBS, p, padded.data(), nullptr);
        REQUIRE(why != nullptr && std::string(why).find("padding") != std::string::npos);
    }
    printf("%zu sets ok\n", checked);
    return 0;
}
