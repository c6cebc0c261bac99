// TEST INFRASTRUCTURE: drives host/path_verify.h alone (the argument checks and the first_bad / why decision of dst_rescue_verify_paths and
// dst_rescue_verify_writes over arrays of computed roots) against a model in two loops: the first marks, for EVERY path or write, each property
// that fails there; the second takes the lowest marked position and the first property in the order leaf, root, next root.  Built with
// -fsanitize=address,undefined by tests/test_rescue_path_verify_host.py and run as a program: exit status 0 and "rounds ok" on stdout, nothing on
// stderr.  Every array is allocated at its exact size, so a read past an end is reported.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "host/path_verify.h"

static int fail(const char* what, size_t count, long long got, unsigned why) {
    printf("FAILED: %s (count %zu, first_bad %lld, why %u)\n", what, count, got, why);
    return 1;
}
// node `v` of a pool of few values: equal nodes are frequent, and two different nodes differ in one byte only, the last
static void put(uint8_t* at, unsigned v) { for (int b = 0; b < 32; b++) at[b] = (uint8_t)(0xA0 + b); at[31] = (uint8_t)v; }

static int shape_checks() {
    for (uint32_t n = 0; n <= 70; n++) {
        const bool ok = pv_check_shape(n, nullptr, 0) == nullptr;
        if (ok != (n >= 2 && n <= 64)) return fail("the range of n", 0, n, 0);
    }
    for (uint32_t n = 2; n <= 64; n++) {
        const uint64_t top = n == 64 ? ~(uint64_t)0 >> 1 : ((uint64_t)1 << (n - 1)) - 1;        // the largest index of a path of n nodes
        std::vector<uint64_t> idx = {0, top, top >> 1, 1 & top};
        if (pv_check_shape(n, idx.data(), idx.size())) return fail("valid indices refused", idx.size(), n, 0);
        for (size_t at = 0; at < idx.size(); at++) {
            std::vector<uint64_t> bad = idx;
            bad[at] = top + 1;
            if (!pv_check_shape(n, bad.data(), bad.size())) return fail("index 2^(n-1) accepted", at, n, 0);
            bad[at] = ~(uint64_t)0;
            if (!pv_check_shape(n, bad.data(), bad.size())) return fail("index 2^64 - 1 accepted", at, n, 0);
        }
    }
    if (!pv_check_shape(2, nullptr, (size_t)1 << 31) || !pv_check_shape(2, nullptr, ((size_t)1 << 31) + 5)) return fail("2^31 paths accepted", 0, 0, 0);      // refused before any index is read
    return 0;
}

static int paths_round(std::mt19937_64& rng, size_t count, uint32_t n, bool with_leaves, unsigned pool) {
    std::vector<uint8_t> own(32 * count), paths(32 * (size_t)n * count), leaves(with_leaves ? 32 * count : 0), root(32);
    put(root.data(), 0);
    for (size_t i = 0; i < count; i++) {
        put(own.data() + 32 * i, rng() % pool);
        for (uint32_t k = 0; k < n; k++) put(paths.data() + 32 * ((size_t)n * i + k), 100 + rng() % pool);
        if (with_leaves) put(leaves.data() + 32 * i, 100 + rng() % pool);
    }
    std::vector<int> leaf_fails(count, 0), root_fails(count, 0);                                  // loop 1: every property of every path
    for (size_t i = 0; i < count; i++) {
        leaf_fails[i] = with_leaves && paths[32 * (size_t)n * i + 31] != leaves[32 * i + 31];
        root_fails[i] = own[32 * i + 31] != root[31];
    }
    long long want = -1; unsigned want_why = PV_OK;                                               // loop 2: the lowest position, the first property
    for (size_t i = count; i-- > 0;) if (leaf_fails[i] || root_fails[i]) { want = (long long)i; want_why = leaf_fails[i] ? PV_BAD_LEAF : PV_BAD_ROOT; }
    const pv_verdict v = pv_decide_paths(own.data(), root.data(), paths.data(), n, with_leaves ? leaves.data() : nullptr, count);
    if (v.first_bad != want || v.why != want_why) return fail("pv_decide_paths", count, v.first_bad, v.why);
    return 0;
}

static int writes_round(std::mt19937_64& rng, size_t count, bool with_roots, bool with_after, unsigned pool) {
    std::vector<uint8_t> own(32 * count), next(32 * count), roots(with_roots ? 32 * count : 0), before(32), after(32, 0xEE);
    // mostly a consistent history (own[i] = the root before write i, roots[i] = next[i]) with a few breaks, so that late positions are reached
    put(before.data(), 0);
    unsigned cur = 0;
    for (size_t i = 0; i < count; i++) {
        put(own.data() + 32 * i, rng() % 6 == 0 ? rng() % pool : cur);
        cur = 1 + rng() % (pool - 1);
        put(next.data() + 32 * i, cur);
        if (with_roots) put(roots.data() + 32 * i, rng() % 6 == 0 ? rng() % pool : cur);
    }
    std::vector<int> root_fails(count, 0), next_fails(count, 0);
    for (size_t i = 0; i < count; i++) {
        root_fails[i] = own[32 * i + 31] != (i ? next[32 * (i - 1) + 31] : before[31]);
        next_fails[i] = with_roots && next[32 * i + 31] != roots[32 * i + 31];
    }
    long long want = -1; unsigned want_why = PV_OK;
    for (size_t i = count; i-- > 0;) if (root_fails[i] || next_fails[i]) { want = (long long)i; want_why = root_fails[i] ? PV_BAD_ROOT : PV_BAD_NEXT_ROOT; }
    const pv_verdict v = pv_decide_writes(own.data(), next.data(), before.data(), with_roots ? roots.data() : nullptr, count, with_after ? after.data() : nullptr);
    if (v.first_bad != want || v.why != want_why) return fail("pv_decide_writes", count, v.first_bad, v.why);
    if (with_after && memcmp(after.data(), count ? next.data() + 32 * (count - 1) : before.data(), 32)) return fail("root_after", count, v.first_bad, v.why);
    return 0;
}

int main() {
    if (shape_checks()) return 1;
    std::mt19937_64 rng(20240611);
    // directed: nothing to check; one path or write that holds, one that fails each way; the failure in the last position only
    for (size_t count : {(size_t)0, (size_t)1, (size_t)2, (size_t)9})
        for (unsigned pool : {1u, 2u})
            for (int flags = 0; flags < 4; flags++) {
                if (paths_round(rng, count, 2 + (uint32_t)(rng() % 63), flags & 1, pool)) return 1;
                if (writes_round(rng, count, flags & 1, flags & 2, pool + 1)) return 1;
            }
    unsigned rounds = 0;
    for (; rounds < 4000; rounds++) {
        const size_t count = rng() % 40;
        const unsigned pool = 1 + rng() % 3;
        if (paths_round(rng, count, 2 + (uint32_t)(rng() % 63), rng() & 1, pool)) return 1;
        if (writes_round(rng, count, rng() & 1, rng() & 1, pool + 1)) return 1;
    }
    printf("%u rounds ok\n", rounds);
    return 0;
}
