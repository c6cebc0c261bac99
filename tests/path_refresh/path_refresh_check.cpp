// TEST INFRASTRUCTURE: drives host/path_refresh.h alone (pr_plan: which write supplies which node of which held path) against a model in two loops
// -- for every held path and every position, ALL writes in order, the last one that matches kept -- for both key widths, on random and directed
// inputs.  Built with -fsanitize=address,undefined by tests/test_rescue_path_refresh_host.py and run as a program: exit status 0 and "rounds ok" on
// stdout, nothing on stderr.  Every array is allocated at its exact size, so a read past an end is reported.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "host/path_refresh.h"

typedef unsigned __int128 u128;

template <class K> static std::vector<int32_t> model(uint32_t n, const std::vector<K>& keys, const std::vector<K>& held) {
    std::vector<int32_t> sel((size_t)n * held.size(), -1);
    for (size_t j = 0; j < held.size(); j++)
        for (size_t i = 0; i < keys.size(); i++) {
            if (keys[i] == held[j]) sel[(size_t)n * j] = (int32_t)i;
            for (uint32_t k = 1; k < n; k++)
                if ((K)(keys[i] >> (k - 1)) == (K)((K)(held[j] >> (k - 1)) ^ (K)1)) sel[(size_t)n * j + k] = (int32_t)i;
        }
    return sel;
}

template <class K> static int compare(const char* what, uint32_t n, const std::vector<K>& keys, const std::vector<K>& held) {
    const std::vector<int32_t> want = model(n, keys, held);
    std::vector<int32_t> got((size_t)n * held.size(), 12345);
    pr_plan<K>(n, keys.empty() ? nullptr : keys.data(), keys.size(), held.empty() ? nullptr : held.data(), held.size(), got.data());
    for (size_t at = 0; at < got.size(); at++)
        if (got[at] != want[at]) {
            printf("FAILED: %s (%zu-byte keys, n %u, %zu writes, %zu held): path %zu position %zu is write %d, the model says %d\n", what, sizeof(K), n, keys.size(), held.size(),
                   at / n, at % n, got[at], want[at]);
            return 1;
        }
    // every write with a key other than h competes for exactly one position of h's path; a write to h for position 0 alone
    for (size_t j = 0; j < held.size(); j++)
        for (size_t i = 0; i < keys.size(); i++) {
            unsigned positions = keys[i] == held[j];
            for (uint32_t k = 1; k < n; k++) positions += (K)(keys[i] >> (k - 1)) == (K)((K)(held[j] >> (k - 1)) ^ (K)1);
            if (positions != 1) { printf("FAILED: %s: write %zu competes for %u positions of path %zu\n", what, i, positions, j); return 1; }
        }
    return 0;
}

template <class K> static K random_key(std::mt19937_64& rng, uint32_t n) {
    K v = (K)rng();
    if (sizeof(K) > 8) v = (K)(v << 32 << 32) | (K)rng();
    const uint32_t bits = n - 1;                                                                     // keys lie below 2^(n-1)
    return bits >= 8 * sizeof(K) ? v : (K)(v & (K)(((K)1 << bits) - 1));
}

template <class K> static int directed() {
    const uint32_t widest = (uint32_t)(8 * sizeof(K));
    for (uint32_t n : {2u, 3u, 4u, 33u, 34u, 64u, widest}) {
        const uint32_t depth = n - 1;
        const K top = (K)(((K)1 << (depth - 1)) << 1) - 1;                                           // 2^depth - 1 without shifting by the width
        const K h = (K)(top / 3);                                                                    // 0101...
        std::vector<K> keys, held = {h, 0, top, h};
        if (compare<K>("nothing written", n, keys, held)) return 1;
        for (uint32_t b = 0; b < depth; b++) keys.push_back((K)(h ^ ((K)1 << b)));                 // one write under every sibling subtree of h
        if (compare<K>("one write per sibling subtree", n, keys, held)) return 1;
        keys.push_back(h); keys.push_back((K)(h ^ 1)); keys.push_back(h); keys.push_back(0); keys.push_back(top); keys.push_back((K)(h ^ 1));
        if (compare<K>("repeats and writes to the held key", n, keys, held)) return 1;
        if (compare<K>("nothing held", n, keys, std::vector<K>())) return 1;
        std::vector<K> same(17, (K)(h ^ ((K)1 << (depth - 1))));                                    // one key 17 times: the last write wins everywhere
        if (compare<K>("one key many times", n, same, held)) return 1;
    }
    return 0;
}

template <class K> static int random_rounds(std::mt19937_64& rng, unsigned rounds) {
    for (unsigned r = 0; r < rounds; r++) {
        const uint32_t n = r % 3 == 0 ? 2 + (uint32_t)(rng() % 4) : 2 + (uint32_t)(rng() % (8 * sizeof(K) - 1));
        const size_t count = rng() % 40, held_n = rng() % 12;
        std::vector<K> keys(count), held(held_n);
        for (auto& k : keys) k = random_key<K>(rng, n);
        for (auto& k : held) k = random_key<K>(rng, n);
        // near keys: a held key with one bit flipped, a repeat of an earlier write, a held key itself
        for (size_t i = 0; i < count && held_n; i++) {
            const unsigned what = (unsigned)(rng() % 6);
            const K h = held[rng() % held_n];
            if (what == 0) keys[i] = (K)(h ^ ((K)1 << (rng() % (n - 1))));
            else if (what == 1) keys[i] = h;
            else if (what == 2 && i) keys[i] = keys[rng() % i];
        }
        if (compare<K>("random", n, keys, held)) return 1;
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(20240712);
    if (directed<uint64_t>() || directed<u128>()) return 1;
    const unsigned rounds = 1500;
    if (random_rounds<uint64_t>(rng, rounds) || random_rounds<u128>(rng, rounds)) return 1;
    int32_t none = 777;                                                                              // no write, nothing held: nothing is read or written
    pr_plan<uint64_t>(2, nullptr, 0, nullptr, 0, &none);
    if (none != 777) return 1;
    printf("%u rounds ok\n", 2 * rounds);
    return 0;
}
