// TEST INFRASTRUCTURE (host build against the stand-in HIP header of this directory): the flat statement of the low-degree stack
// operations (air_stack_nested.h: st_basis_table / st_class_sums / st_output_basis -- the basis terms of an output merged across ALL selected
// groups, every coefficient an add / subtract of class sums formed once per point) against st_output, the nested statement it replaces
// inside the kernels and which air_merge_test.cpp pins against the per-operation sum.  Equality is exact: both sides are canonical field
// elements.
//
// Coverage: every output (slots 0..7, ST_AUX0, ST_AUX1); every GROUPS value of the launch lists of the three product sets, and
// AG_LOW0 | AG_LOW1; SDK in {0, 4}; DEEP in {false, true} with slices of 8, 9 and 12 items; and two selections of the outputs that take
// the flat form: the one the kernels use (st_flat_default) and ALL outputs, so that the computed terms (kind 5), the shared values
// (j >= 100) and the auxiliary constraints go through the flat tables too.
//
// Inputs.  (a) 20 000 rows of uniform field elements; lo2[4], lo0h, mid[4] and top[2] are drawn independently of each other -- the
// statement may assume no relation between table entries (sum lo2 = 1 is false in the kernel: lo2[2] carries the reference's quirk).
// The all-outputs selection sees the first 2 000 of them.  (b) EDGE = {0, 1, 2, p - 1, p - 2, 2^64, 2^127}: a class sum pairs one entry
// of lo2 (or lo0h), one of mid and one of top; for every (x, y, z) in 7^3, lo2[a] = EDGE[x + a], lo0h = EDGE[x + 4], mid[b] = EDGE[y + b],
// top[c] = EDGE[z + c] (indices mod 7), so every triple (a, b, c) meets every combination, with the stack rows cycling through EDGE.
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <thread>
#include <vector>
#include "../../distaff_amd/csrc/air_stack_nested.h"

static const int NE = 7;
static fe EDGE[NE];

struct Row { StackRows s; fe lo2[4], lo0h, mid[4], top[2]; StackHigh h; };

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
static fe uniform() {
    for (;;) {
        const fe x = fe_make((uint32_t)rnd(), (uint32_t)rnd(), (uint32_t)rnd(), (uint32_t)rnd());
        if (x.v[3] != FE_P3 || x.v[2] != FE_P2 || x.v[1] < FE_P1) return x;                    // below the modulus
    }
}

static std::vector<Row> uniform_rows, edge_rows;

static void make_rows() {
    EDGE[0] = fe_zero(); EDGE[1] = fe_one(); EDGE[2] = fe_make(2, 0, 0, 0);
    EDGE[3] = fe_make(FE_P0 - 1, FE_P1, FE_P2, FE_P3); EDGE[4] = fe_sub(EDGE[3], fe_one());
    EDGE[5] = fe_make(0, 0, 1, 0); EDGE[6] = fe_make(0, 0, 0, 0x80000000u);
    uniform_rows.resize(20000);
    for (Row& r : uniform_rows) {
        for (fe& v : r.s.o) v = uniform();
        for (fe& v : r.s.nw) v = uniform();
        for (fe& v : r.lo2) v = uniform();
        r.lo0h = uniform();
        for (fe& v : r.mid) v = uniform();
        for (fe& v : r.top) v = uniform();
        r.h.push = uniform(); r.h.cmp = uniform(); r.h.rescr = uniform(); r.h.keep = uniform();
        for (fe& v : r.h.resc) v = uniform();
    }
    edge_rows.resize(NE * NE * NE);
    for (int t = 0; t < NE * NE * NE; t++) {
        Row& r = edge_rows[t];
        const int x = t % NE, y = (t / NE) % NE, z = t / (NE * NE);
        for (int j = 0; j < 12; j++) r.s.o[j] = EDGE[(t + j) % NE];
        for (int j = 0; j < 8; j++) r.s.nw[j] = EDGE[(3 * t + j + 1) % NE];
        for (int a = 0; a < 4; a++) r.lo2[a] = EDGE[(x + a) % NE];
        r.lo0h = EDGE[(x + 4) % NE];
        for (int b = 0; b < 4; b++) r.mid[b] = EDGE[(y + b) % NE];
        for (int c = 0; c < 2; c++) r.top[c] = EDGE[(z + c) % NE];
        r.h.push = EDGE[(t + 1) % NE]; r.h.cmp = EDGE[(t + 2) % NE]; r.h.rescr = EDGE[(t + 3) % NE]; r.h.keep = EDGE[(t + 5) % NE];
        for (int i = 0; i < 6; i++) r.h.resc[i] = EDGE[(2 * t + i) % NE];
    }
}

static std::atomic<long> all_bad{0}, all_checked{0}, printed{0};

// the rows as an instance with these template arguments sees them: items at and above a compile-time depth are zeros, and so are
// the items past the end of the slice
template <int SDK, bool DEEP>
static StackRows shaped(const StackRows& in, int sl) {
    StackRows s = in;
    s.sl = sl;
    if (SDK != 0) for (int j = SDK; j < 12; j++) s.o[j] = fe_zero();
    for (int j = (DEEP ? sl : 8); j < 12; j++) s.o[j] = fe_zero();
    return s;
}

template <uint32_t GROUPS, int SDK, bool DEEP, uint32_t FLAT>
static void check_rows(const std::vector<Row>& rows, size_t count, int sl, const char* input) {
    long bad = 0, checked = 0;
    for (size_t it = 0; it < count && it < rows.size(); it++) {
        const Row& r = rows[it];
        const StackRows s = shaped<SDK, DEEP>(r.s, sl);
        StClassSums<st_class_count<GROUPS, SDK, DEEP, FLAT>()> cs;
        st_class_sums<GROUPS, SDK, DEEP, FLAT>(cs, r.lo2, r.lo0h, r.mid, r.top);
        static_for_air<0, 10>([&](auto i_) {
            constexpr int I = decltype(i_)::value;                  // slots 0..7, ST_AUX0 = 8, ST_AUX1 = 9
            if constexpr (st_touches<I, GROUPS>()) {
                const fe got = st_output_basis<I, GROUPS, SDK, DEEP, FLAT>(s, cs, r.lo2, r.lo0h, r.mid, r.top, r.h);
                const fe want = st_output<I, GROUPS, SDK, DEEP>(s, r.lo2, r.lo0h, r.mid, r.top, r.h);
                checked++;
                if (!fe_eq(got, want)) {
                    if (printed++ < 20) printf("MISMATCH output %d, groups 0x%X, SDK %d, %s slice of %d, flat 0x%X, %s row %zu\n", I, (unsigned)GROUPS, SDK, DEEP ? "deep" : "plain", sl, (unsigned)FLAT, input, it);
                    bad++;
                }
            }
        });
    }
    all_bad += bad; all_checked += checked;
}

template <uint32_t GROUPS, int SDK, bool DEEP>
static void run_shape(int sl) {
    constexpr uint32_t DEF = st_flat_default<GROUPS, SDK, DEEP>();
    check_rows<GROUPS, SDK, DEEP, DEF>(uniform_rows, 20000, sl, "uniform");
    check_rows<GROUPS, SDK, DEEP, DEF>(edge_rows, edge_rows.size(), sl, "edge");
    check_rows<GROUPS, SDK, DEEP, 0x3FFu>(uniform_rows, 2000, sl, "uniform");
    check_rows<GROUPS, SDK, DEEP, 0x3FFu>(edge_rows, edge_rows.size(), sl, "edge");
}

template <uint32_t GROUPS>
static void run_groups(std::vector<std::thread>& pool) {
    pool.emplace_back([] { run_shape<GROUPS, 0, false>(8); });
    pool.emplace_back([] { run_shape<GROUPS, 4, false>(8); });
    pool.emplace_back([] { run_shape<GROUPS, 0, true>(8); run_shape<GROUPS, 4, true>(8); });
    pool.emplace_back([] { run_shape<GROUPS, 0, true>(9); run_shape<GROUPS, 4, true>(9); });
    pool.emplace_back([] { run_shape<GROUPS, 0, true>(12); run_shape<GROUPS, 4, true>(12); });
}

int main() {
    make_rows();
    std::vector<std::thread> pool;
    // depth-4 set
    run_groups<AG_HIGH>(pool); run_groups<AG_LOW0>(pool); run_groups<AG_LOW1>(pool);
    // small and deep sets
    run_groups<AG_RESCR>(pool); run_groups<(AG_PUSH | AG_CMP | AG_KEEP)>(pool);
    run_groups<(AG_LOW(0, 0) | AG_LOW(0, 2))>(pool); run_groups<(AG_LOW(0, 1) | AG_LOW(0, 3))>(pool);
    run_groups<(AG_LOW(1, 2) | AG_LOW(1, 3))>(pool); run_groups<(AG_LOW(1, 0) | AG_LOW(1, 1))>(pool);
    // every low-degree operation in one statement
    run_groups<(AG_LOW0 | AG_LOW1)>(pool);
    for (auto& t : pool) t.join();
    printf("%ld comparisons, %ld mismatches\n", all_checked.load(), all_bad.load());
    return all_bad.load() ? 1 : 0;
}
