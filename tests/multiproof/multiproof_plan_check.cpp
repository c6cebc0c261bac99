// host/multiproof_plan.h alone against a model over std::set: every pool node is given its identity (level, position); the supplied positions
// must be the definition's, in its order; running the job lists level by level must give every member of every K_l exactly once, from its two
// children in left / right order, and end in (0, 0) at the last pool node; the path node indices must name the leaf and the siblings of each
// index.  Every subset of depth 1 .. 3 and a sample of depth 4 in two orders, random sets up to depth 12, and depth 63.  Built with sanitizers by
// tests/test_rescue_multiproof_host.py.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <utility>
#include "host/multiproof_plan.h"

typedef std::pair<uint32_t, uint64_t> node_id;
static size_t checked = 0;
#define REQUIRE(c) do { if (!(c)) { printf("line %d: %s (depth %u, %zu indices)\n", __LINE__, #c, depth, idx.size()); exit(1); } } while (0)

static void check(uint32_t depth, const std::vector<uint64_t>& idx) {
    const size_t count = idx.size(), n = depth + 1;
    std::vector<node_id> want;                           // the definition
    uint64_t digests = 0;
    std::vector<size_t> width(depth + 1);
    std::set<uint64_t> level(idx.begin(), idx.end());
    for (uint32_t l = depth; l >= 1; l--) {
        std::set<uint64_t> up;
        for (uint64_t p : level) { if (!level.count(p ^ 1)) want.push_back({l, p ^ 1}); up.insert(p >> 1); }      // p ascends, one member per pair: so does p ^ 1
        level.swap(up);
        width[l - 1] = level.size();
        digests += level.size();
    }
    for (uint32_t what : {0u, (uint32_t)MP_SUPPLIED, (uint32_t)(MP_SUPPLIED | MP_JOBS), (uint32_t)(MP_JOBS | MP_WHERE), (uint32_t)(MP_SUPPLIED | MP_JOBS | MP_WHERE)}) {
        mp_plan p;
        REQUIRE(mp_plan_make(depth, idx.data(), count, what, p) == nullptr);
        REQUIRE(p.sizes.nodes == want.size() && p.sizes.digests == digests && p.pool() == count + want.size() + digests);
        if (what & MP_SUPPLIED) {
            REQUIRE(p.slevel.size() == want.size() && p.spos.size() == want.size());
            for (size_t m = 0; m < want.size(); m++) REQUIRE(node_id(p.slevel[m], p.spos[m]) == want[m]);
        }
        std::map<uint32_t, node_id> id;
        for (size_t i = 0; i < count; i++) id[(uint32_t)i] = {depth, idx[i]};
        for (size_t m = 0; m < want.size(); m++) id[(uint32_t)(count + m)] = want[m];
        if (what & MP_JOBS) {
            REQUIRE(p.jobs.size() == 3 * digests);
            size_t next = 0;
            for (uint32_t l = depth; l-- > 0;) {
                REQUIRE(p.joff[l] == next && p.jcnt[l] == width[l]);
                std::map<uint32_t, node_id> made;            // a level's jobs read nothing the level writes
                for (size_t g = 0; g < p.jcnt[l]; g++) {
                    const uint32_t *j = p.jobs.data() + 3 * (next + g);
                    REQUIRE(id.count(j[0]) && id.count(j[1]) && !id.count(j[2]) && !made.count(j[2]));
                    const node_id a = id[j[0]], b = id[j[1]];
                    REQUIRE(a.first == l + 1 && b.first == l + 1 && !(a.second & 1) && b.second == a.second + 1);
                    REQUIRE(j[2] == count + want.size() + next + g);
                    made[j[2]] = {l, a.second >> 1};
                }
                id.insert(made.begin(), made.end());
                next += p.jcnt[l];
            }
            REQUIRE(id.size() == p.pool() && id[(uint32_t)(p.pool() - 1)] == node_id(0, 0));
            std::set<node_id> distinct;
            for (auto& kv : id) distinct.insert(kv.second);
            REQUIRE(distinct.size() == id.size());           // every node once
        }
        if ((what & MP_WHERE) && (what & MP_JOBS)) {
            REQUIRE(p.where.size() == count * n);
            for (size_t i = 0; i < count; i++) {
                REQUIRE(p.where[i * n] == i);
                for (size_t k = 1; k < n; k++) REQUIRE(id.count(p.where[i * n + k]) && id[p.where[i * n + k]] == node_id((uint32_t)(depth - k + 1), (idx[i] >> (k - 1)) ^ 1));
            }
        }
    }
    checked++;
}

int main() {
    std::mt19937_64 rng(7);
    for (uint32_t depth = 1; depth <= 4; depth++)
        for (uint32_t mask = 1; mask < (1u << (1u << depth)); mask += depth < 4 ? 1 : 29) {      // depth 4: every 29th of the 65 535 subsets
            std::vector<uint64_t> idx;
            for (uint64_t i = 0; i < (1u << depth); i++) if (mask >> i & 1) idx.push_back(i);
            check(depth, idx);
            std::shuffle(idx.begin(), idx.end(), rng);
            check(depth, idx);
        }
    for (int round = 0; round < 300; round++) {
        const uint32_t depth = 1 + (uint32_t)(rng() % 12);
        std::set<uint64_t> s;
        const size_t count = 1 + rng() % std::min<size_t>((size_t)1 << depth, 200);
        while (s.size() < count) s.insert(rng() & (((uint64_t)1 << depth) - 1));
        std::vector<uint64_t> idx(s.begin(), s.end());
        std::shuffle(idx.begin(), idx.end(), rng);
        check(depth, idx);
    }
    for (int round = 0; round < 20; round++) {
        std::set<uint64_t> s = {0, 1, (uint64_t)1 << 62, ((uint64_t)1 << 63) - 1};
        while (s.size() < 4 + (size_t)round) { const uint64_t k = rng() >> 1; s.insert(k); s.insert(k ^ (rng() % 5)); }
        std::vector<uint64_t> idx(s.begin(), s.end());
        std::shuffle(idx.begin(), idx.end(), rng);
        check(63, idx);
    }
    {                                                    // what is refused
        mp_plan p;
        const uint64_t twice[3] = {5, 2, 5};
        if (mp_plan_make(3, twice, 3, MP_JOBS, p) == nullptr) { printf("a repeated index was accepted\n"); return 1; }
    }
    printf("%zu sets ok\n", checked);
    return 0;
}
