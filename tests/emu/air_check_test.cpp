// TEST INFRASTRUCTURE (host build against the stand-in HIP header of this directory, linked with emu_runtime.cpp): the verdict of the
// check of the trace rows (air_kernel.h: air_check_kernel) against "some constraint of the per-constraint evaluation is non-zero".
//
// The check side: air_check_kernel itself, called for one row at a time through the launch lists of the three product instance sets as
// their units state them (air_chain_sd4 / _small / _deep, included below), with the partial stack values handed on through AirArgs::ev
// exactly as on the device; the failing-step word is fresh for every row, so the row's own verdict is read, not a minimum.
// The per-constraint side: a recorder that SUMS what is emitted per constraint index -- the decoder sections (air_op_bits, air_sponge,
// air_flow) and, for the user stack, the per-operation statement with all of its sections in one call (air_stack_perop.h), which is the
// formulation the product chains do not use -- and then asks whether any of the sums is non-zero.
//
// Rows (argv[1]: the periodic table and the valid traces, written by tests/test_air_trace_check_host.py from the oracle):
//   valid     every step of the valid traces: no constraint may be non-zero on either side
//   one cell  a valid trace with ONE register of one row replaced by a uniform or an EDGE value: the steps before and at that row
//   bits      op bits 0 / 1 at random, everything else uniform: the op-bit constraints vanish, the other sections decide
//   edge      every register from EDGE = {0, 1, 2, p - 1, p - 2, 2^64, 2^127} (air_flags_test.cpp's set)
//   uniform   every register uniform below p
// at the shapes of the valid traces, (2, 1, 8) and the widest (16, 8, 32); every instance set that takes the shape is asked.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../distaff_amd/csrc/kernels_air_sd4.hip"
#include "../../distaff_amd/csrc/kernels_air_small.hip"
#include "../../distaff_amd/csrc/kernels_air_deep.hip"
#include "../../distaff_amd/csrc/rescue_constants.h"

typedef unsigned __int128 u128;
static const u128 P = (u128)0 - ((u128)45 << 40) + 1;               // 2^128 - 45 * 2^40 + 1
static fe to_fe(u128 x) { return fe_make((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)(x >> 64), (uint32_t)(x >> 96)); }

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
static u128 uniform() { for (;;) { u128 x = ((u128)rnd() << 64) | rnd(); if (x < P) return x; } }
static const int NE = 7;
static u128 EDGE[NE];

// the per-constraint evaluation: sums per constraint index
struct Recorder {
    fe d[128]; bool seen[128];
    Recorder() { for (int i = 0; i < 128; i++) { d[i] = fe_zero(); seen[i] = false; } }
    void emit(uint32_t cidx, int, const fe& v) { d[cidx] = fe_add(d[cidx], v); seen[cidx] = true; }
    bool any_nonzero() const { for (int i = 0; i < 128; i++) if (seen[i] && !fe_is_zero(d[i])) return true; return false; }
};

struct Table {
    size_t W, n; uint32_t cd, ld, sd;
    std::vector<fe> cols;                                            // [W][n]
};

static fe g_periodic[128 * AIR_PERIODIC_STRIDE];
static AirConsts g_consts;

static AirArgs args_of(const Table& t, fe* ev, unsigned long long* word) {
    AirArgs a{};
    a.lde = t.cols.data(); a.periodic = g_periodic; a.consts = &g_consts;
    for (int i = 0; i < 10; i++) a.ev[i] = ev + (size_t)i * t.n;
    a.bad_step = word;
    a.n = t.n; a.col_stride = t.n; a.W = (uint32_t)t.W;
    a.ctx_depth = t.cd; a.loop_depth = t.ld; a.stack_depth = t.sd;
    a.cl = t.cd > 1 ? t.cd : 1; a.ll = t.ld > 1 ? t.ld : 1; a.sl = t.sd > 8 ? t.sd : 8;
    return a;
}

static bool reference_verdict(const Table& t, const AirArgs& a, size_t k) {
    const AirColumns cols{a.lde + k, a.lde + k + 1, a.col_stride};
    AirRows<16, 8> rows;
    fe o[32], nw[32];
    air_load_rows<32>(rows, o, nw, a, cols, (int)t.sd);
    AirFlags f;
    air_op_flags(f, rows);
    const fe* per = a.periodic + (size_t)(((uint32_t)k << 3) & 127u) * AIR_PERIODIC_STRIDE;
    Recorder rec;
    air_op_bits(rec, rows, f, per);
    air_sponge<true>(rec, a, cols, rows, nw, f, per);
    air_flow<16, 8>(rec, a, cols, rows, f, (int)a.cl, (int)a.ll);
    air_stack_per_operation<32, AS_STACK_ANY>(rec, o, nw, (int)(t.sd > 8 ? t.sd : 8), (int)t.sd, 20 + a.cl + a.ll, f, per, a.consts);
    return rec.any_nonzero();
}

// one row through a set's launch list: the walk the units hand to air_chain_*
struct RowChain {
    const AirArgs& a; size_t k;
    template <int CL, int LL, int SD, int SLCAP, int SECT, uint32_t GROUPS, int FLAGS> void run() const {
        blockIdx.x = (unsigned)(k / AIR_THREADS); blockIdx.y = 0; threadIdx.x = (unsigned)(k % AIR_THREADS);
        gridDim = dim3((unsigned)((a.n + AIR_THREADS - 1) / AIR_THREADS), 1); blockDim = dim3(AIR_THREADS);
        air_check_kernel<CL, LL, SD, SLCAP, SECT, GROUPS, FLAGS>(a);
    }
    template <int CL, int LL, int SD, int SLCAP> void boundary() const {}
};

static long g_rows = 0, g_verdicts = 0, g_bad = 0, g_true = 0;

// every step of the table (or the steps [from, to)) on both sides
static void compare(const Table& t, const char* what, size_t from = 0, size_t to = (size_t)-1) {
    std::vector<fe> ev(10 * t.n);
    unsigned long long word;
    AirArgs a = args_of(t, ev.data(), &word);
    const bool small_shape = t.cd <= 2 && t.ld <= 1 && t.sd <= 8;
    if (to > t.n - 1) to = t.n - 1;
    for (size_t k = from; k < to; k++) {
        const bool want = reference_verdict(t, a, k);
        g_rows++; g_true += want;
        for (int set = 0; set < 3; set++) {
            if ((set == 0 && !(small_shape && t.sd == 4)) || (set == 1 && !small_shape)) continue;
            for (int i = 0; i < 10; i++) ev[(size_t)i * t.n + k] = to_fe(uniform());      // a chain defines every partial value it reads
            word = ~0ull;
            const RowChain ch{a, k};
            if (set == 0) air_chain_sd4(ch); else if (set == 1) air_chain_small(ch); else air_chain_deep(ch);
            const bool got = word != ~0ull;
            g_verdicts++;
            if (got != want || (got && word != k)) {
                if (g_bad < 20) printf("MISMATCH %s: shape (%u, %u, %u) step %zu set %d: check says %d (word %llu), the constraints say %d\n", what, t.cd, t.ld, t.sd, k, set, (int)got, word, (int)want);
                g_bad++;
            }
        }
    }
}

static Table drawn_table(uint32_t cd, uint32_t ld, uint32_t sd, size_t n, int kind) {      // kind 0 uniform, 1 edge, 2 bits
    Table t; t.cd = cd; t.ld = ld; t.sd = sd; t.W = 15 + cd + ld + sd; t.n = n; t.cols.resize(t.W * n);
    for (size_t c = 0; c < t.W; c++)
        for (size_t k = 0; k < n; k++) {
            u128 v = kind == 1 ? EDGE[rnd() % NE] : uniform();
            if (kind == 2 && c >= 5 && c < 15) v = rnd() & 1;
            t.cols[c * n + k] = to_fe(v);
        }
    return t;
}

int main(int argc, char** argv) {
    EDGE[0] = 0; EDGE[1] = 1; EDGE[2] = 2; EDGE[3] = P - 1; EDGE[4] = P - 2; EDGE[5] = (u128)1 << 64; EDGE[6] = (u128)1 << 127;
    if (argc < 2) { printf("usage: air_check_test DATA\n"); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { printf("cannot open %s\n", argv[1]); return 2; }
    auto rd = [&](void* p, size_t bytes) { if (fread(p, 1, bytes, fh) != bytes) { printf("short read\n"); exit(2); } };
    // periodic table: [128][23] elements; columns 23..28 are the cubes of columns 8..13 (api.hip build_periodic_table)
    for (int s = 0; s < 128; s++) {
        fe* row = g_periodic + (size_t)s * AIR_PERIODIC_STRIDE;
        rd(row, 23 * sizeof(fe));
        for (int i = 0; i < 6; i++) row[23 + i] = fe_cube(row[8 + i]);
    }
    memcpy(g_consts.sponge_mds, SPONGE_MDS, sizeof(g_consts.sponge_mds)); memcpy(g_consts.sponge_inv_mds, SPONGE_INV_MDS, sizeof(g_consts.sponge_inv_mds));
    memcpy(g_consts.hasher_mds, HASHER_MDS, sizeof(g_consts.hasher_mds)); memcpy(g_consts.hasher_inv_mds, HASHER_INV_MDS, sizeof(g_consts.hasher_inv_mds));
    uint64_t count; rd(&count, 8);
    std::vector<Table> valid(count);
    for (Table& t : valid) {
        uint64_t h[5]; rd(h, sizeof(h));
        t.W = h[0]; t.n = h[1]; t.cd = (uint32_t)h[2]; t.ld = (uint32_t)h[3]; t.sd = (uint32_t)h[4];
        t.cols.resize(t.W * t.n); rd(t.cols.data(), t.cols.size() * sizeof(fe));
    }
    fclose(fh);

    // valid rows: nothing may be non-zero
    for (const Table& t : valid) {
        const long before = g_true;
        compare(t, "valid");
        if (g_true != before) { printf("MISMATCH: %ld steps of a valid trace (%u, %u, %u) have a non-zero constraint: the fixture is wrong\n", g_true - before, t.cd, t.ld, t.sd); g_bad++; }
    }
    // one cell of a valid trace replaced: the step that has the row as its next row and the step that has it as its current row
    long failing_cells = 0;
    for (const Table& t : valid)
        for (int rep = 0; rep < 600; rep++) {
            Table m = t;
            const size_t c = rep < (int)t.W * 4 ? (size_t)rep % t.W : rnd() % t.W, k = 1 + rnd() % (t.n - 2);
            fe v; do { v = to_fe((rep & 1) ? EDGE[rnd() % NE] : uniform()); } while (memcmp(&m.cols[c * m.n + k], &v, sizeof(fe)) == 0);
            m.cols[c * m.n + k] = v;
            const long before = g_true;
            compare(m, "one cell", k - 1, k + 1);
            failing_cells += g_true != before;
        }
    // drawn rows
    const uint32_t shapes[][3] = {{1, 0, 4}, {1, 0, 8}, {3, 0, 25}, {2, 1, 8}, {0, 0, 4}, {16, 8, 32}};
    for (const auto& s : shapes)
        for (int kind = 0; kind < 3; kind++) compare(drawn_table(s[0], s[1], s[2], 97, kind), kind == 0 ? "uniform" : kind == 1 ? "edge" : "bits");
    printf("%ld steps, %ld verdicts, %ld steps with a non-zero constraint, %ld replaced cells that fail, %ld mismatches\n", g_rows, g_verdicts, g_true, failing_cells, g_bad);
    if (failing_cells < 1500) { printf("too few of the replaced cells fail: the sweep does not test what it says\n"); return 1; }
    return g_bad ? 1 : 0;
}
