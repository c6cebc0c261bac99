// ORACLE (test infrastructure, NOT product code) -- whole-array checkers of prover intermediates.
//
// The step-by-step oracle (prover.hpp) recomputes every intermediate, which at the benchmarked sizes (2^20 .. 2^24 steps) takes
// hours on one core.  The checkers below instead VERIFY an array the device produced, at every element, in O(size) work spread
// over host threads (at most 16; OMP_NUM_THREADS when set):
//   * evaluations against coefficients: sum_pos r^pos v[pos] == (r^N - 1) * sum_j a_j / (r g^j - 1) for a random r (an error
//     escapes with probability <= N / p), with a bisection over blocks that names the first disagreeing evaluation;
//   * Merkle trees: every node against the hash of its two children (the device's own children, so one wrong node is named);
//   * leaves: BLAKE3 of every trace row / FRI row;
//   * constraint evaluation, DEEP composition and FRI folding: every element recomputed from its inputs (prover.rs, fri/prover.rs).
// Every checker also rejects a stored value >= p: a sum mod p would not notice a non-canonical p + k where k belongs.
// A checker returns -1 when the array is right, otherwise the first failing index, and describes the failure in `msg`.
#pragma once
#include "prover.hpp"
#include <cstdlib>
#include <string>
#include <thread>

namespace orc {

static inline unsigned chk_threads() {
    const char* e = getenv("OMP_NUM_THREADS");
    long t = e ? atol(e) : 0;
    if (t <= 0) t = (long)std::thread::hardware_concurrency();
    return (unsigned)std::max(1L, std::min(16L, t));
}

// f(thread, begin, end) on contiguous chunks of [0, n), in order; returns the number of chunks used
template <class F> static unsigned chk_parallel(size_t n, F f) {
    unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(chk_threads(), (n + 4095) / 4096));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; t++) {
        size_t b = n * t / T, e = n * (t + 1) / T;
        if (T == 1) f(0u, b, e); else th.emplace_back([=, &f]() { f(t, b, e); });
    }
    for (auto& x : th) x.join();
    return T;
}

static const long CHK_PASS = -1;

static inline std::string chk_hex(u128 v) { char b[40]; snprintf(b, sizeof b, "0x%016llx%016llx", (unsigned long long)(v >> 64), (unsigned long long)v); return b; }

// first index i with v[i] >= p, or -1
static inline long chk_first_noncanonical(const u128* v, size_t n) {
    std::vector<long> first(16, CHK_PASS);
    chk_parallel(n, [&](unsigned t, size_t b, size_t e) { for (size_t i = b; i < e; i++) if (v[i] >= P) { first[t] = (long)i; return; } });
    for (long f : first) if (f != CHK_PASS) return f;
    return CHK_PASS;
}

// sum_{j < m} c[j] y^j, Horner per thread chunk
static inline u128 chk_poly_eval(const u128* c, size_t m, u128 y) {
    std::vector<u128> part(16, 0);
    std::vector<size_t> begin(16, 0);
    unsigned T = chk_parallel(m, [&](unsigned t, size_t b, size_t e) {
        u128 acc = 0;
        for (size_t j = e; j-- > b;) acc = add(mul(acc, y), c[j]);
        part[t] = acc; begin[t] = b;
    });
    u128 r = 0;
    for (unsigned t = 0; t < T; t++) r = add(r, mul(part[t], exp(y, (u128)begin[t])));
    return r;
}

// ---- evaluations against coefficients ------------------------------------------------------------------------------------
// v[pos] = sum_j a[j] g^(j pos) on the N-point domain of g = root of unity of order N.  With q_j = a_j / (r g^j - 1) and
// Q(y) = sum_j q_j y^j:  sum_{pos in [s, s+len)} r^pos v[pos] = r^s (r^len Q(g^(s+len)) - Q(g^s)).
struct EvalIdentity {
    const u128* a; size_t m; const u128* v; size_t N; u128 r, g;
    vec q;
    bool init(std::string& msg) {
        vec den(m), inv_den(m);
        u128 gj = 1;
        for (size_t j = 0; j < m; j++) { den[j] = sub(mul(r, gj), 1); gj = mul(gj, g); if (den[j] == 0) { msg = "unlucky random point r"; return false; } }
        inv_many_fill(den.data(), inv_den.data(), m);
        q.resize(m);
        chk_parallel(m, [&](unsigned, size_t b, size_t e) { for (size_t j = b; j < e; j++) q[j] = mul(a[j], inv_den[j]); });
        return true;
    }
    u128 expected(size_t s, size_t len) const {
        u128 gs = exp(g, (u128)s), ge = exp(g, (u128)((s + len) % N));
        return mul(exp(r, (u128)s), sub(mul(exp(r, (u128)len), chk_poly_eval(q.data(), m, ge)), chk_poly_eval(q.data(), m, gs)));
    }
    u128 actual(size_t s, size_t len) const {
        std::vector<u128> part(16, 0);
        unsigned T = chk_parallel(len, [&](unsigned t, size_t b, size_t e) {
            u128 rp = exp(r, (u128)(s + b)), acc = 0;
            for (size_t i = s + b; i < s + e; i++) { acc = add(acc, mul(rp, v[i])); rp = mul(rp, r); }
            part[t] = acc;
        });
        u128 acc = 0;
        for (unsigned t = 0; t < T; t++) acc = add(acc, part[t]);
        return acc;
    }
};

static inline long chk_evals_vs_coeffs(const u128* a, size_t m, const u128* v, size_t N, u128 r, std::string& msg) {
    long bad = chk_first_noncanonical(a, m);
    if (bad != CHK_PASS) { msg = "coefficient " + std::to_string(bad) + " is not below p: " + chk_hex(a[bad]); return bad; }
    bad = chk_first_noncanonical(v, N);
    if (bad != CHK_PASS) { msg = "evaluation " + std::to_string(bad) + " is not below p: " + chk_hex(v[bad]); return bad; }
    EvalIdentity id{a, m, v, N, r, get_root_of_unity(N), {}};
    if (!id.init(msg)) return 0;
    if (id.actual(0, N) == id.expected(0, N)) return CHK_PASS;
    size_t s = 0, len = N;                                       // bisection: the leftmost block whose sum disagrees
    while (len > 1) {
        size_t half = len / 2;
        if (id.actual(s, half) != id.expected(s, half)) len = half;
        else { s += half; len -= half; }
    }
    msg = "evaluation " + std::to_string(s) + " disagrees with the coefficients: " + chk_hex(v[s]);
    return (long)s;
}

// ---- Merkle trees (merkle.rs:269 build_merkle_nodes) ---------------------------------------------------------------------
// nodes[1 .. L) of a tree over L leaves (nodes[0] unused); returns the DEEPEST node that is not the hash of its two children
static inline long chk_merkle_nodes(const uint8_t* leaves, size_t L, const uint8_t* nodes, std::string& msg) {
    std::vector<long> last(16, CHK_PASS);
    chk_parallel(L > 1 ? L - 1 : 0, [&](unsigned t, size_t b, size_t e) {
        for (size_t k = b + 1; k < e + 1; k++) {
            const uint8_t* ch = k >= L / 2 ? leaves + 64 * (k - L / 2) : nodes + 64 * k;
            uint8_t h[32];
            blake3(ch, 64, h);
            if (memcmp(h, nodes + 32 * k, 32)) last[t] = (long)k;
        }
    });
    for (size_t t = 16; t-- > 0;) if (last[t] != CHK_PASS) { msg = "tree node " + std::to_string(last[t]) + " is not the hash of its children"; return last[t]; }
    return CHK_PASS;
}

// ---- leaves ---------------------------------------------------------------------------------------------------------------
// trace leaves (prover.rs:35, trace_table.rs:174): leaf i = BLAKE3 of row i, W elements of 16 little-endian bytes
static inline long chk_row_leaves(const u128* rows, size_t count, size_t W, const uint8_t* leaves, std::string& msg) {
    long bad = chk_first_noncanonical(rows, count * W);
    if (bad != CHK_PASS) { msg = "row " + std::to_string(bad / W) + " holds a value not below p in register " + std::to_string(bad % W); return bad / (long)W; }
    std::vector<long> first(16, CHK_PASS);
    chk_parallel(count, [&](unsigned t, size_t b, size_t e) {
        uint8_t h[32];
        for (size_t i = b; i < e; i++) {
            blake3((const uint8_t*)(rows + i * W), W * 16, h);
            if (memcmp(h, leaves + 32 * i, 32)) { first[t] = (long)i; return; }
        }
    });
    for (long f : first) if (f != CHK_PASS) { msg = "leaf " + std::to_string(f) + " is not the hash of its row"; return f; }
    return CHK_PASS;
}

// FRI leaves (fri/utils.rs:16): row r of a layer of M = 4R evaluations is (e[r], e[r+R], e[r+2R], e[r+3R])
static inline long chk_fri_leaves(const u128* e, size_t M, const uint8_t* leaves, std::string& msg) {
    long bad = chk_first_noncanonical(e, M);
    if (bad != CHK_PASS) { msg = "evaluation " + std::to_string(bad) + " is not below p"; return bad; }
    const size_t R = M / 4;
    std::vector<long> first(16, CHK_PASS);
    chk_parallel(R, [&](unsigned t, size_t b, size_t en) {
        uint8_t buf[64], h[32];
        for (size_t r = b; r < en; r++) {
            for (int k = 0; k < 4; k++) to_bytes(e[r + k * R], buf + 16 * k);
            blake3(buf, 64, h);
            if (memcmp(h, leaves + 32 * r, 32)) { first[t] = (long)r; return; }
        }
    });
    for (long f : first) if (f != CHK_PASS) { msg = "FRI leaf " + std::to_string(f) + " is not the hash of its row"; return f; }
    return CHK_PASS;
}

// ---- FRI fold (fri/prover.rs:25-49) ---------------------------------------------------------------------------------------
// Row r sits at x_r * (1, w, w^2, w^3), x_r = g^r, w = g^R (g of order M).  The quartic through it, written in t = X / x_r, has the
// coefficients d_k = (1/4) sum_q v_q w^(-qk) (a 4-point inverse DFT), so its value at alpha is sum_k d_k (alpha / x_r)^k: no
// inversion per row, x_r^-1 is a running power of g^-1.  Same values as quartic_interpolate_batch + quartic_evaluate_batch.
static inline void fri_fold_rows(const u128* e, size_t M, u128 alpha, size_t b, size_t en, u128* out) {
    const size_t R = M / 4;
    const u128 g = get_root_of_unity(M), ginv = inv(g), w = exp(g, (u128)R), inv4 = inv(4);
    u128 xinv = exp(ginv, (u128)b);
    for (size_t r = b; r < en; r++) {
        u128 s0 = add(e[r], e[r + 2 * R]), s1 = sub(e[r], e[r + 2 * R]);
        u128 t0 = add(e[r + R], e[r + 3 * R]), wt1 = mul(w, sub(e[r + R], e[r + 3 * R]));
        u128 d0 = add(s0, t0), d2 = sub(s0, t0), d1 = sub(s1, wt1), d3 = add(s1, wt1);
        u128 y = mul(alpha, xinv);
        out[r - b] = mul(inv4, add(mul(add(mul(add(mul(d3, y), d2), y), d1), y), d0));
        xinv = mul(xinv, ginv);
    }
}

static inline long chk_fri_fold(const u128* e, size_t M, u128 alpha, const u128* next, std::string& msg) {
    long bad = chk_first_noncanonical(e, M);
    if (bad != CHK_PASS) { msg = "evaluation " + std::to_string(bad) + " of the layer is not below p"; return bad; }
    bad = chk_first_noncanonical(next, M / 4);
    if (bad != CHK_PASS) { msg = "folded entry " + std::to_string(bad) + " is not below p"; return bad; }
    std::vector<long> first(16, CHK_PASS);
    chk_parallel(M / 4, [&](unsigned t, size_t b, size_t en) {
        vec f(4096);
        for (size_t c = b; c < en; c += 4096) {
            size_t ce = std::min(en, c + 4096);
            fri_fold_rows(e, M, alpha, c, ce, f.data());
            for (size_t r = c; r < ce; r++) if (f[r - c] != next[r]) { first[t] = (long)r; return; }
        }
    });
    for (long f : first) if (f != CHK_PASS) { msg = "folded entry " + std::to_string(f) + " is wrong: " + chk_hex(next[f]); return f; }
    return CHK_PASS;
}

// ---- DEEP composition (prover.rs:94-101, trace_table.rs:206-261, constraint_poly.rs:39) -------------------------------------
// comp(x) = t1(x) (k1 + k2 x^inc) + k3 (c(x) - c(z)) / (x - z),  t1(x) = sum_c d1_c (T_c(x) - T_c(z)) / (x - z) + sum_c d2_c (T_c(x) - T_c(z g)) / (x - z g)
// at the positions [start, start + count) of the N-point domain; rows / cevals / comp hold those positions only.
static inline long chk_composition(const u128* rows, size_t count, size_t start, size_t W, const u128* cevals, const u128* comp,
                                   size_t n, size_t N, const u128* draws, const u128* z1, const u128* z2, u128 c_z, std::string& msg) {
    long bad = chk_first_noncanonical(comp, count);
    if (bad != CHK_PASS) { msg = "composition value at " + std::to_string(start + bad) + " is not below p"; return bad; }
    bad = chk_first_noncanonical(cevals, count);
    if (bad != CHK_PASS) { msg = "constraint value at " + std::to_string(start + bad) + " is not below p"; return bad; }
    bad = chk_first_noncanonical(rows, count * W);
    if (bad != CHK_PASS) { msg = "row " + std::to_string(start + bad / W) + " holds a value not below p"; return bad / (long)W; }
    const u128 z = draws[0], zg = mul(z, get_root_of_unity(n)), k1 = draws[513], k2 = draws[514], k3 = draws[515];
    const u128 gN = get_root_of_unity(N), g_inc = exp(gN, (u128)get_incremental_trace_degree(n));
    u128 A0 = 0, B0 = 0;
    for (size_t c = 0; c < W; c++) { A0 = add(A0, mul(draws[1 + c], z1[c])); B0 = add(B0, mul(draws[257 + c], z2[c])); }
    std::vector<long> first(16, CHK_PASS);
    chk_parallel(count, [&](unsigned t, size_t b, size_t en) {
        const size_t K = 2048;
        vec den(2 * K), invd(2 * K), num_z(K), num_zg(K);
        u128 x = exp(gN, (u128)(start + b)), xi = exp(g_inc, (u128)(start + b));
        for (size_t c0 = b; c0 < en; c0 += K) {
            size_t ce = std::min(en, c0 + K);
            for (size_t i = c0; i < ce; i++) {
                const u128* row = rows + i * W;
                u128 a = 0, bb = 0;
                for (size_t c = 0; c < W; c++) { a = add(a, mul(draws[1 + c], row[c])); bb = add(bb, mul(draws[257 + c], row[c])); }
                u128 kx = add(k1, mul(k2, xi));
                num_z[i - c0] = add(mul(sub(a, A0), kx), mul(k3, sub(cevals[i], c_z)));
                num_zg[i - c0] = mul(sub(bb, B0), kx);
                den[2 * (i - c0)] = sub(x, z); den[2 * (i - c0) + 1] = sub(x, zg);
                x = mul(x, gN); xi = mul(xi, g_inc);
            }
            inv_many_fill(den.data(), invd.data(), 2 * (ce - c0));
            for (size_t i = c0; i < ce; i++) {
                u128 want = add(mul(num_z[i - c0], invd[2 * (i - c0)]), mul(num_zg[i - c0], invd[2 * (i - c0) + 1]));
                if (want != comp[i]) { first[t] = (long)i; return; }
            }
        }
    });
    for (long f : first) if (f != CHK_PASS) { msg = "composition value at " + std::to_string(start + f) + " is wrong: " + chk_hex(comp[f]); return f; }
    return CHK_PASS;
}

// ---- constraint evaluation (prover.rs:43-64, constraint_table.rs:45-88) --------------------------------------------------------
// For every listed step s of the 8n-point domain (x = g_8n^s; cur / nxt = LDE rows at s B/8 and s B/8 + B): the reference evaluator's
// transition combination == tvals[i] (and every transition constraint vanishes on trace steps), and off the trace domain
// c(x) = bi / (x - 1) + bf / (x - x_last) + t (x - x_last) / (x^n - 1) == cvals[i], the constraint LDE at natural position s B/8.
static inline long chk_constraints(const Evaluator& proto, size_t n, size_t ctx, size_t lp, size_t st, const uint64_t* steps, size_t count,
                                   const u128* cur, const u128* nxt, const u128* tvals, const u128* cvals, std::string& msg) {
    long bad = chk_first_noncanonical(tvals, count);
    if (bad != CHK_PASS) { msg = "transition value at step " + std::to_string(steps[bad]) + " is not below p"; return bad; }
    bad = chk_first_noncanonical(cvals, count);
    if (bad != CHK_PASS) { msg = "constraint value at step " + std::to_string(steps[bad]) + " is not below p"; return bad; }
    const size_t W = 15 + ctx + lp + st;
    const u128 g8n = get_root_of_unity(8 * n), x_last = exp(get_root_of_unity(n), (u128)(n - 1)), g8 = get_root_of_unity(8);
    std::vector<long> first(16, CHK_PASS);
    std::vector<std::string> why(16);
    chk_parallel(count, [&](unsigned t, size_t b, size_t en) {
        Evaluator ev = proto;
        TraceState c(ctx, lp, st), nx(ctx, lp, st);
        const size_t K = 1024;
        vec den(3 * K), invd(3 * K), tv(K), bi(K), bf(K), xs(K);
        u128 x = 0;
        for (size_t c0 = b; c0 < en; c0 += K) {
            size_t ce = std::min(en, c0 + K);
            for (size_t i = c0; i < ce; i++) {
                const uint64_t s = steps[i];
                x = (i > b && s == steps[i - 1] + 1) ? mul(x, g8n) : exp(g8n, (u128)s);
                c.load_row([&](size_t j) { return cur[i * W + j]; });
                nx.load_row([&](size_t j) { return nxt[i * W + j]; });
                bool ok = true;
                size_t k = i - c0;
                tv[k] = ev.evaluate_transition(c, nx, x, s, &ok);
                ev.evaluate_boundaries(c, x, bi[k], bf[k]);
                xs[k] = x;
                if (!ok || tv[k] != tvals[i]) {
                    first[t] = (long)i;
                    why[t] = ok ? "transition combination at step " + std::to_string(s) + " is wrong: " + chk_hex(tvals[i])
                                : "a transition constraint does not vanish at trace step " + std::to_string(s);
                    return;
                }
                bool trace_step = s % 8 == 0;
                den[3 * k] = trace_step ? 1 : sub(x, 1);
                den[3 * k + 1] = trace_step ? 1 : sub(x, x_last);
                den[3 * k + 2] = trace_step ? 1 : sub(exp(g8, (u128)(s % 8)), 1);       // x^n = g_8^s
            }
            inv_many_fill(den.data(), invd.data(), 3 * (ce - c0));
            for (size_t i = c0; i < ce; i++) {
                size_t k = i - c0;
                if (steps[i] % 8 == 0) continue;                                          // the divisors vanish on the trace domain
                u128 cx = add(add(mul(bi[k], invd[3 * k]), mul(bf[k], invd[3 * k + 1])), mul(mul(tv[k], sub(xs[k], x_last)), invd[3 * k + 2]));
                if (cx != cvals[i]) { first[t] = (long)i; why[t] = "constraint value at step " + std::to_string(steps[i]) + " is wrong: " + chk_hex(cvals[i]); return; }
            }
        }
    });
    for (size_t t = 0; t < 16; t++) if (first[t] != CHK_PASS) { msg = why[t]; return first[t]; }
    return CHK_PASS;
}

}  // namespace orc
