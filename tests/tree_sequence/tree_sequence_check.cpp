// TEST INFRASTRUCTURE: drives host/tree_sequence.h alone (the plan of an ordered batch of leaf writes) against a model that restates the
// definition with two nested loops: the sibling of operation i on level l is read from the last earlier operation whose ancestor on that level
// is the sibling node, else from the tree.  Built with -fsanitize=address,undefined by tests/test_rescue_tree_sequence_host.py and run as a
// program: exit status 0 and "rounds ok" on stdout, nothing on stderr.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include "host/tree_sequence.h"

static int fail(const char* what, unsigned depth, size_t i, unsigned l) {
    printf("FAILED: %s (depth %u, operation %zu, level %u)\n", what, depth, i, l);
    return 1;
}

static int round_of(std::mt19937_64& rng, uint32_t depth, size_t count, unsigned spread_bits) {
    const uint64_t mask = ((uint64_t)1 << depth) - 1;
    std::vector<uint64_t> idx(count);
    const uint64_t base = rng() & mask;
    for (auto& v : idx) {                                              // clustered: the low spread_bits vary, now and then the top bit too
        v = (base ^ (rng() & (((uint64_t)1 << spread_bits) - 1))) & mask;
        if (rng() % 5 == 0) v ^= (uint64_t)1 << (depth - 1);
        if (rng() % 7 == 0 && &v != &idx[0]) v = idx[rng() % (size_t)(&v - &idx[0])];
    }
    // the tree before the call: a pseudo-random third of the nodes "stored" at a position derived from (level, prefix), the rest empty
    auto original = [&](uint32_t l, uint64_t q) -> uint32_t {
        const uint64_t h = (q * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)l << 56) ^ base;
        return h % 3 == 0 ? TSEQ_EMPTY : (uint32_t)((h >> 8) % 0x7FFFFFFEu);
    };
    const tseq_plan p = tseq_plan_make(depth, idx.data(), count, original);
    if (p.src.size() != (size_t)(depth + 1) * count) return fail("size of src", depth, 0, 0);
    for (size_t i = 0; i < count; i++) {
        uint32_t want = original(depth, idx[i]);                       // the leaf's own old value
        for (size_t j = 0; j < i; j++) if (idx[j] == idx[i]) want = TSEQ_VERSION | (uint32_t)j;
        if (p.src[i] != want) return fail("own source", depth, i, depth);
        for (uint32_t l = depth; l >= 1; l--) {
            const uint64_t sib = (idx[i] >> (depth - l)) ^ 1;
            want = original(l, sib);
            for (size_t j = 0; j < i; j++) if ((idx[j] >> (depth - l)) == sib) want = TSEQ_VERSION | (uint32_t)j;
            if (p.src[(size_t)(depth - l + 1) * count + i] != want) return fail("sibling source", depth, i, l);
        }
    }
    for (uint32_t l = 0; l <= depth; l++) {                            // the touched nodes: every distinct prefix once, sorted, with its last operation
        std::map<uint64_t, uint32_t> last;
        for (size_t i = 0; i < count; i++) last[l == 0 ? 0 : idx[i] >> (depth - l)] = (uint32_t)i;
        if (p.tcnt[l] != last.size() || p.toff[l] + p.tcnt[l] > p.touched() || p.tlast.size() != p.touched()) return fail("touched count", depth, 0, l);
        size_t at = p.toff[l];
        for (const auto& kv : last) {
            if (p.tpref[at] != kv.first || p.tlast[at] != kv.second) return fail("touched node", depth, at, l);
            at++;
        }
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(20260101);
    int rounds = 0;
    for (uint32_t depth : {1u, 2u, 3u, 5u, 10u, 26u, 62u, 63u})
        for (size_t count : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)8, (size_t)33, (size_t)200})
            for (unsigned spread : {0u, 1u, 3u, 8u}) {
                if (round_of(rng, depth, count, spread < depth ? spread : depth)) return 1;
                rounds++;
            }
    printf("%d rounds ok\n", rounds);
    return 0;
}
