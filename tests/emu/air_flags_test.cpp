// TEST INFRASTRUCTURE (host build against the stand-in HIP header of this directory): the op flags and the op-bit constraints of the
// constraint kernel (air_kernel.h: air_op_flags, air_op_bits) against the products written out factor by factor, as trace_state.rs:281-350
// and decoder/op_bits.rs:10-79 state them.  The kernel forms most entries of its flag tables by subtraction from one product per table
// (x * (1 - b) = x - x * b) and constraints 10 - 12 without the multiplications of their stated forms; the algebra holds for every field
// element, so what can go wrong is a carry or borrow path of the limb arithmetic.  The expected values therefore use none of it: additions
// and subtractions are plain 128-bit integer arithmetic modulo p, products the portable host multiplication (fe_mul_portable, which
// tests/hostfield pins against the oracle).
//
// Operands.  EDGE = {0, 1, 2, p - 1, p - 2, 2^64, 2^127}.  A product pairs registers of one of two sets: the five ld bits with the two hd
// bits (lo2, mid, top, hdf, the low-degree flags, BEGIN / NOOP / PUSH / ASSERT, the products of constraints 11 and 12), and the three cf
// bits with ld[0], ld[1] (the eight cf flags; lo2[2] = (1 - ld[0]) * cf[1], the reference's quirk).  Sweep A runs every combination of
// EDGE in the seven registers of the first set (7^7 rows), sweep B every combination in the five of the second (7^5 rows); the registers
// a sweep does not enumerate, the op counters and the next row's cf bits are drawn per row, half of them from EDGE and half uniform.
// Then 20 000 rows with every register uniform below p.
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <thread>
#include <vector>
#include "../../distaff_amd/csrc/air_kernel.h"

typedef unsigned __int128 u128;
static const u128 P = (u128)0 - ((u128)45 << 40) + 1;               // 2^128 - 45 * 2^40 + 1

static u128 to_u(const fe& a) { return ((u128)a.v[3] << 96) | ((u128)a.v[2] << 64) | ((u128)a.v[1] << 32) | a.v[0]; }
static fe to_fe(u128 x) { return fe_make((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)(x >> 64), (uint32_t)(x >> 96)); }
// the expected side: integers below p
static u128 radd(u128 a, u128 b) { u128 s = a + b; return (s < a || s >= P) ? s - P : s; }
static u128 rsub(u128 a, u128 b) { return a >= b ? a - b : a + (P - b); }
static u128 rmul(u128 a, u128 b) { return to_u(fe_mul_portable(to_fe(a), to_fe(b))); }
static u128 rnot(u128 a) { return rsub(1, a); }
static u128 rbin(u128 a) { return rsub(rmul(a, a), a); }

static thread_local uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
static u128 uniform() { for (;;) { u128 x = ((u128)rnd() << 64) | rnd(); if (x < P) return x; } }
static const int NE = 7;
static u128 EDGE[NE];
static u128 drawn() { return (rnd() & 1) ? EDGE[rnd() % NE] : uniform(); }

// the values of the op-bit section in emission order
struct Recorder {
    fe d[15]; unsigned seen = 0;
    void emit(uint32_t cidx, int, const fe& v) { if (cidx < 15) { d[cidx] = v; seen |= 1u << cidx; } }
};

static thread_local long bad = 0, checked = 0;                      // per thread; for_rows adds them up
static std::atomic<long> all_bad{0}, all_checked{0};
static void expect(const fe& got, u128 want, const char* what, int idx, long row) {
    checked++;
    if (to_u(got) != want) { if (bad < 20) printf("MISMATCH %s[%d], row %ld\n", what, idx, row); bad++; }
}

struct Bits { u128 opc, n_opc, cf[3], n_cf[3], ld[5], hd[2], per[AIR_PERIODIC_STRIDE]; };

static void check_row(const Bits& b, long row) {
    AirRows<2, 1> r{};
    r.c_opc = to_fe(b.opc); r.n_opc = to_fe(b.n_opc);
    for (int i = 0; i < 3; i++) { r.cf[i] = to_fe(b.cf[i]); r.n_cf[i] = to_fe(b.n_cf[i]); }
    for (int i = 0; i < 5; i++) r.ld[i] = to_fe(b.ld[i]);
    for (int i = 0; i < 2; i++) r.hd[i] = to_fe(b.hd[i]);
    fe per[AIR_PERIODIC_STRIDE];
    for (int i = 0; i < AIR_PERIODIC_STRIDE; i++) per[i] = to_fe(b.per[i]);

    AirFlags f;
    air_op_flags(f, r);
    Recorder rec;
    air_op_bits(rec, r, f, per);

    // ---- the flags, factor by factor (trace_state.rs:281-350) ----
    u128 cff[8];
    for (int i = 0; i < 8; i++) {
        const u128 x0 = (i & 1) ? b.cf[0] : rnot(b.cf[0]), x1 = (i & 2) ? b.cf[1] : rnot(b.cf[1]), x2 = (i & 4) ? b.cf[2] : rnot(b.cf[2]);
        cff[i] = rmul(rmul(x0, x1), x2);
        expect(f.cff[i], cff[i], "cf flag", i, row);
    }
    u128 ldf[32];
    ldf[0] = rmul(rnot(b.ld[0]), rnot(b.ld[1])); ldf[1] = rmul(b.ld[0], rnot(b.ld[1]));
    ldf[2] = rmul(rnot(b.ld[0]), b.cf[1]);                                  // sic: cf_op_bits[1] (trace_state.rs:301)
    ldf[3] = rmul(b.ld[0], b.ld[1]);
    for (int k = 2, len = 4; k < 5; k++, len *= 2)                          // every further bit doubles the table (trace_state.rs:303-317)
        for (int i = 0; i < len; i++) { ldf[len + i] = rmul(ldf[i], b.ld[k]); ldf[i] = rmul(ldf[i], rnot(b.ld[k])); }
    for (int i = 0; i < 32; i++) expect(f.ldf(i), ldf[i], "low-degree flag", i, row);      // without the ASSERT adjustment: assert_flag carries it
    for (int i = 0; i < 4; i++) {
        const u128 x0 = (i & 1) ? b.ld[0] : rnot(b.ld[0]);
        const u128 x1 = i == 2 ? b.cf[1] : ((i & 2) ? b.ld[1] : rnot(b.ld[1]));
        expect(f.lo2[i], rmul(x0, x1), "lo2", i, row);
        expect(f.mid[i], rmul((i & 1) ? b.ld[2] : rnot(b.ld[2]), (i & 2) ? b.ld[3] : rnot(b.ld[3])), "mid", i, row);
    }
    expect(f.top[0], rnot(b.ld[4]), "top", 0, row);
    expect(f.top[1], b.ld[4], "top", 1, row);
    u128 hdf[4];
    for (int i = 0; i < 4; i++) hdf[i] = rmul((i & 1) ? b.hd[0] : rnot(b.hd[0]), (i & 2) ? b.hd[1] : rnot(b.hd[1]));
    expect(f.begin_flag, rmul(ldf[0], hdf[0]), "begin", 0, row);
    expect(f.noop_flag, rmul(ldf[31], hdf[3]), "noop", 0, row);
    expect(f.ld_all, ldf[31], "ld_all", 0, row);
    const u128 push = rmul(hdf[0], b.ld[0]);                                // PUSH (trace_state.rs:343)
    expect(f.hdf[0], push, "hd flag", 0, row);
    for (int i = 1; i < 4; i++) expect(f.hdf[i], hdf[i], "hd flag", i, row);
    expect(f.assert_flag, rmul(ldf[0], b.hd[0]), "assert", 0, row);         // ASSERT (trace_state.rs:346)
    expect(f.n_void, rmul(rmul(b.n_cf[0], b.n_cf[1]), b.n_cf[2]), "next void", 0, row);

    // ---- the op-bit constraints, multiplied out (decoder/op_bits.rs:10-79) ----
    if (rec.seen != 0x7FFFu) { if (bad < 20) printf("MISMATCH: constraints emitted %x, row %ld\n", rec.seen, row); bad++; }
    for (int i = 0; i < 3; i++) expect(rec.d[i], rbin(b.cf[i]), "constraint", i, row);
    for (int i = 0; i < 5; i++) expect(rec.d[3 + i], rbin(b.ld[i]), "constraint", 3 + i, row);
    for (int i = 0; i < 2; i++) expect(rec.d[8 + i], rbin(b.hd[i]), "constraint", 8 + i, row);
    u128 ld_prod = 1, hd_prod = 1;
    for (int i = 0; i < 5; i++) ld_prod = rmul(ld_prod, b.ld[i]);
    for (int i = 0; i < 2; i++) hd_prod = rmul(hd_prod, b.hd[i]);
    const u128 cf_sum = radd(radd(b.cf[0], b.cf[1]), b.cf[2]);
    const u128 hacc = cff[0];
    expect(rec.d[10], rsub(radd(rmul(radd(b.opc, 1), hacc), rmul(b.opc, rnot(hacc))), b.n_opc), "constraint", 10, row);
    expect(rec.d[11], rmul(b.opc, rmul(rnot(ld_prod), rnot(hd_prod))), "constraint", 11, row);
    expect(rec.d[12], rmul(cf_sum, rnot(rmul(ld_prod, hd_prod))), "constraint", 12, row);
    const u128 n_void = rmul(rmul(b.n_cf[0], b.n_cf[1]), b.n_cf[2]);
    expect(rec.d[13], rmul(cff[7], rnot(n_void)), "constraint", 13, row);
    u128 v = 0;
    for (int i : {1, 4, 5, 6}) v = radd(v, rmul(cff[i], b.per[21]));        // BEGIN, LOOP, WRAP, BREAK: prefix mask
    for (int i : {2, 3}) v = radd(v, rmul(cff[i], b.per[20]));              // TEND, FEND: cycle mask
    v = radd(v, rmul(push, b.per[22]));                                     // PUSH: its mask
    expect(rec.d[14], v, "constraint", 14, row);
}

static void draw_rest(Bits& b) {
    b.opc = drawn(); b.n_opc = drawn();
    for (int i = 0; i < 3; i++) b.n_cf[i] = drawn();
    for (int i = 0; i < AIR_PERIODIC_STRIDE; i++) b.per[i] = uniform();
}

// rows [first, first + total) on four threads, row first + c from make(c); every thread draws from its own generator
template <class MAKE>
static void for_rows(long first, long total, MAKE make) {
    const int T = 4;
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++) pool.emplace_back([=]() {
        rs = 0x9E3779B97F4A7C15ull * (uint64_t)(2 * (first + t) + 1);
        bad = checked = 0;
        for (long c = t; c < total; c += T) { Bits b; make(c, b); check_row(b, first + c); }
        all_bad += bad; all_checked += checked;
    });
    for (auto& th : pool) th.join();
}

int main() {
    EDGE[0] = 0; EDGE[1] = 1; EDGE[2] = 2; EDGE[3] = P - 1; EDGE[4] = P - 2; EDGE[5] = (u128)1 << 64; EDGE[6] = (u128)1 << 127;
    long rows = 0, total = 1;
    // sweep A: ld[0..4], hd[0..1]
    for (int i = 0; i < 7; i++) total *= NE;
    for_rows(rows, total, [](long c, Bits& b) {
        for (int i = 0; i < 5; i++) { b.ld[i] = EDGE[c % NE]; c /= NE; }
        for (int i = 0; i < 2; i++) { b.hd[i] = EDGE[c % NE]; c /= NE; }
        for (int i = 0; i < 3; i++) b.cf[i] = drawn();
        draw_rest(b);
    });
    rows += total;
    // sweep B: cf[0..2], ld[0..1]
    total = 1;
    for (int i = 0; i < 5; i++) total *= NE;
    for_rows(rows, total, [](long c, Bits& b) {
        for (int i = 0; i < 3; i++) { b.cf[i] = EDGE[c % NE]; c /= NE; }
        for (int i = 0; i < 2; i++) { b.ld[i] = EDGE[c % NE]; c /= NE; }
        for (int i = 2; i < 5; i++) b.ld[i] = drawn();
        for (int i = 0; i < 2; i++) b.hd[i] = drawn();
        draw_rest(b);
    });
    rows += total;
    // uniform rows
    total = 20000;
    for_rows(rows, total, [](long, Bits& b) {
        for (int i = 0; i < 3; i++) b.cf[i] = uniform();
        for (int i = 0; i < 5; i++) b.ld[i] = uniform();
        for (int i = 0; i < 2; i++) b.hd[i] = uniform();
        b.opc = uniform(); b.n_opc = uniform();
        for (int i = 0; i < 3; i++) b.n_cf[i] = uniform();
        for (int i = 0; i < AIR_PERIODIC_STRIDE; i++) b.per[i] = uniform();
    });
    rows += total;
    const long bad_rows = all_bad, comparisons = all_checked;
    printf("%ld rows, %ld comparisons, %ld mismatches\n", rows, comparisons, bad_rows);
    return bad_rows ? 1 : 0;
}
