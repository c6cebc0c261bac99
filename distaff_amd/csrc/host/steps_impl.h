// The prover steps shared by all drivers (host/steps.h declares them): the implementation, included by api.hip alone.  Host code: every function here only enqueues on
// c->stream, except where its comment says that it waits.
#pragma once
#include "steps.h"
#include "../host_util.h"
#include "../host_vm.h"

// ---- steps 3-5 ------------------------------------------------------------------------------------------------------------------
// constraint degrees in constraint-index order (decoder/mod.rs:31-47, stack/mod.rs:40-41) and the coefficient each
// constraint receives when they are visited in degree-group order (evaluator.rs:335-358,385-406; coefficients.rs:140-185)
static void transition_coefficients(const dst_ctx* c, const fe* draws344, std::vector<fe>& tc) {
    const size_t cl = c->prm.ctx_depth > 1 ? c->prm.ctx_depth : 1, ll = c->prm.loop_depth > 1 ? c->prm.loop_depth : 1;
    const size_t sl = c->stack_depth > 8 ? c->stack_depth : 8;
    std::vector<int> deg = {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 8, 8, 6, 4, 6, 7, 6, 6, 4};
    deg.resize(20 + cl + ll, 4);
    deg.resize(20 + cl + ll + 2 + c->stack_depth, 7);
    // compacted coefficient list (build_transition_coefficients)
    const fe* t = draws344 + 188;
    std::vector<fe> cc;
    auto take = [&](size_t from, size_t cnt) { for (size_t i = 0; i < cnt; i++) cc.push_back(t[from + i]); };
    take(0, 40); take(40, 2 * cl); take(72, 2 * ll); take(88, 4); take(92, 2 * sl);
    const size_t nc = deg.size();
    tc.assign(2 * nc, fe_zero());
    size_t i = 0;
    for (int d = 0; d <= 8; d++)
        for (size_t k = 0; k < nc; k++)
            if (deg[k] == d) { tc[k] = cc[2 * i]; tc[nc + k] = cc[2 * i + 1]; i++; }
}

int step::eval_constraints(dst_ctx* c, const dst_public* pub, const uint8_t* coeffs, int64_t* bad_step, bool defer_check, bool check_here) {
    c->pub = *pub;
    c->air_draws.resize(344);
    memcpy(c->air_draws.data(), coeffs, 344 * sizeof(fe));
    c->ceval_inverted = false;                                   // the evaluation writes plain evaluations
    std::vector<fe> tc;
    transition_coefficients(c, c->air_draws.data(), tc);
    // the 344 constraint coefficients and the compacted transition coefficients -> device, queued from the page-locked staging area (`tc`
    // goes out of scope while the copies may still be pending: the evaluation's verdict is not waited for)
    if (tc.size() > ScratchTail::MAX_TC) { c->err = "too many transition coefficients for the staging area"; return DST_ERR_ARG; }
    const ScratchTail tail(c);
    fe* h = reinterpret_cast<fe*>(c->h_stage + HS_DRAWS);
    memcpy(h, c->air_draws.data(), 344 * sizeof(fe));
    memcpy(h + 344, tc.data(), tc.size() * sizeof(fe));
    HIP_TRY(c, hipMemcpyAsync(tail.coef(), h, 344 * sizeof(fe), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(tail.tc(), h + 344, tc.size() * sizeof(fe), hipMemcpyHostToDevice, c->stream));
    const int r = k_eval_constraints(c, tail.coef(), tail.tc(), bad_step, defer_check, check_here);      // prover.rs:53-64
    if (r == DST_ERR_AIR) c->err = "transition constraints were not satisfied";
    return r;
}

// The two boundary combinations (evaluator.rs:181-326) in COEFFICIENT form.  With v_k(x) = T_k(x) - const_k for the constrained
// registers k, the reference evaluates I(x) = sum_k v_k(x) * (cc_k + cc'_k * x^p), p = 6n + 2, on the 8n-point domain and interpolates
// it again (constraint_table.rs:54-62).  I has degree < 7n + 2 < 8n, so the interpolant is I itself, and its coefficients are two
// linear combinations of the trace polynomials: A = sum_k cc_k v_k at [0, n) and A' = sum_k cc'_k v_k at [p, p + n).  Nothing is
// evaluated and nothing is interpolated: ip / fp (8n coefficients each, before the divisions) are written directly.
// DISTAFF_BOUNDARY=eval keeps the evaluate-and-interpolate route (the tests compare its evaluation vectors with the oracle's).
int step::boundary_polys(dst_ctx* c, const fe* draws344, fe* ip, fe* fp, fe* o0, fe* o1, fe* o2, fe* o3) {
    const size_t n = c->n, D = 8 * n, W = c->W, p = 6 * n + 2;
    const uint32_t ctx_depth = c->prm.ctx_depth, loop_depth = c->prm.loop_depth;
    const size_t sd = c->stack_depth;
    const size_t cl = ctx_depth > 1 ? ctx_depth : 1, ll = loop_depth > 1 ? loop_depth : 1;
    // host: weights per trace register (plain, degree-adjusted) and the constant terms, for the first-step and last-step combinations
    std::vector<u128> w(4 * W, 0);                       // [pass][adj][register]
    u128 g[4] = {0, 0, 0, 0};                            // [pass][adj]
    const u128 one = 1;
    for (int pass = 0; pass < 2; pass++) {
        const fe* cc = draws344 + pass * 94;
        auto term = [&](int col, u128 constant, size_t idx) {       // value = T_col(x) - constant (col < 0: no register, value = -constant)
            for (int adj = 0; adj < 2; adj++) {
                const u128 k = fe_to_u128(cc[idx + adj]);
                if (col >= 0) w[(pass * 2 + adj) * W + col] = hf_add(w[(pass * 2 + adj) * W + col], k);
                if (constant != 0) g[pass * 2 + adj] = hf_add(g[pass * 2 + adj], hf_mul(k, constant));
            }
        };
        term(0, pass ? fe_to_u128(c->op_counter) : 0, 0);
        if (pass == 0) { for (int i = 0; i < 4; i++) term(1 + i, 0, 2 + 2 * i); }
        else { for (int i = 0; i < 2; i++) term(1 + i, fe_to_u128(c->program_hash[i]), 2 + 2 * i); }
        for (int i = 0; i < 3; i++) term(5 + i, pass ? one : 0, 10 + 2 * i);
        for (int i = 0; i < 5; i++) term(8 + i, pass ? one : 0, 16 + 2 * i);
        for (int i = 0; i < 2; i++) term(13 + i, pass ? one : 0, 26 + 2 * i);
        for (size_t i = 0; i < cl; i++) if (i < ctx_depth) term(15 + (int)i, 0, 30 + 2 * i);
        for (size_t i = 0; i < ll; i++) if (i < loop_depth) term(15 + (int)ctx_depth + (int)i, 0, 62 + 2 * i);
        const uint32_t nio = pass ? c->pub.num_outputs : c->pub.num_inputs;
        for (uint32_t i = 0; i < nio && i < 8; i++) {
            u128 v; memcpy(&v, pass ? c->pub.outputs[i] : c->pub.inputs[i], 16);
            term(i < sd ? 15 + (int)ctx_depth + (int)loop_depth + (int)i : -1, v, 78 + 2 * i);
        }
    }
    std::vector<fe> up(4 * W + 4);
    for (size_t i = 0; i < 4 * W; i++) up[i] = fe_from_u128(w[i]);
    for (int i = 0; i < 4; i++) up[4 * W + i] = fe_from_u128(g[i]);
    fe* d_w = (fe*)c->d_stage;                           // staging area is free until the openings
    // through the page-locked staging area: the copy is queued and the host moves on
    fe* h_w = reinterpret_cast<fe*>(c->h_stage + HS_WEIGHTS);
    memcpy(h_w, up.data(), up.size() * sizeof(fe));
    HIP_TRY(c, hipMemcpyAsync(d_w, h_w, up.size() * sizeof(fe), hipMemcpyHostToDevice, c->stream));
    fe* outs[4] = {o0, o1, o2, o3};                       // [pass][adj]
    if (ip) {                                            // the 8n-coefficient polynomials themselves (DISTAFF_COMBINE=steps)
        HIP_TRY(c, hipMemsetAsync(ip, 0, D * sizeof(fe), c->stream));
        HIP_TRY(c, hipMemsetAsync(fp, 0, D * sizeof(fe), c->stream));
        outs[0] = ip; outs[1] = ip + p; outs[2] = fp; outs[3] = fp + p;
    }
    k_lincomb4(c, c->polys, W, n, d_w, outs[0], outs[1], outs[2], outs[3]);
    for (int q = 0; q < 4; q++) k_sub_at0(c, outs[q], d_w + 4 * W + q);
    return DST_OK;
}

// What the fused combination (k_combine_fused) reads of the two boundary constraints: I = A + x^p A', F = C + x^p C' (see
// step::boundary_polys), p = 6n + 2, each of A, A', C, C' a linear combination of the trace polynomials with n coefficients.  Written
// behind a leading zero and divided in place -- A, A' by (x - 1), C, C' by (x - x_last) -- so that q4[k][0] is the sum / the value at
// x_last and q4[k][1 + i] the quotient coefficient i.  Four divisions over n + 1 coefficients instead of two over 8n.
int step::boundary_quotients(dst_ctx* c, const fe* draws344, fe* q4, size_t stride) {
    const size_t n = c->n;
    HIP_TRY(c, hipMemsetAsync(q4, 0, 4 * stride * sizeof(fe), c->stream));
    // ip = q4[0] (A at offset 0) ... boundary_polys writes A, A', C, C' at (ip, ip + p, fp, fp + p): hand it views whose
    // "+ p" lands on the next array
    int r = boundary_polys(c, draws344, nullptr, nullptr, q4 + 1, q4 + stride + 1, q4 + 2 * stride + 1, q4 + 3 * stride + 1);
    if (r) return r;
    fe* arrays[4] = {q4, q4 + stride, q4 + 2 * stride, q4 + 3 * stride};
    const fe divisors[4] = {fe_one(), fe_one(), c->x_last, c->x_last};
    k_syn_div_batch(c, arrays, divisors, 4, n + 1);            // one set of launches for the four
    return DST_OK;
}

int step::combine(dst_ctx* c, int parts) {
    const size_t n = c->n, D = 8 * n;
    fe* ip = c->cwork; fe* fp = c->cwork + D; fe* tp = c->cwork + 2 * D; fe* work = c->cwork + 3 * D;
    const bool steps = dst_internal_combine_by_steps(c);         // the reference's sequence of whole-array steps (tests), else the fused pass
    fe* q4 = c->cwork; const size_t qs = n + 16;                 // fused: boundary quotients (4 x (n + 1) coefficients)
    const fe* draws = c->air_draws.data();
    if (parts & 1) {
        if (!steps) { if (int rb = boundary_quotients(c, draws, q4, qs)) return rb; }
        else {
            if (dst_internal_boundary_by_evaluation(c)) {
                k_intt8_cosets(c, c->ceval, ip, work);
                k_intt8_cosets(c, c->ceval + D, fp, work);
            } else if (int rb = boundary_polys(c, draws, ip, fp)) return rb;
            k_syn_div(c, ip, D, fe_one());
            k_syn_div(c, fp, D, c->x_last);
        }
    }
    if (parts & 2) {
        const bool inverted = c->ceval_inverted;                // per coset, by its owner (dst_prove_sharded), or not (every other driver)
        c->ceval_inverted = false;
        if (!steps) {
            // the eight inverse coset transforms, then ONE pass: 8-point step across cosets, division of the transition part, sum
            const fe* inv = c->ceval + 2 * D;
            if (!inverted) { k_intt_cosets_local(c, c->ceval + 2 * D, work, 8); inv = work; }
            k_combine_fused(c, inv, q4, qs, c->cpoly);
        } else {
            if (inverted) k_cross8(c, c->ceval + 2 * D, tp);
            else k_intt8_cosets(c, c->ceval + 2 * D, tp, work);
            k_syn_div_expanded(c, tp, c->cpoly, D, n, c->x_last);
            k_add(c, c->cpoly, ip, D);
            k_add(c, c->cpoly, fp, D);
        }
    }
    return DST_OK;
}

// ---- step 7 ---------------------------------------------------------------------------------------------------------------------
void step::fri_file_root(dst_ctx* c, int d, const uint8_t root[32]) {
    if (c->fri_roots.size() <= (size_t)d) c->fri_roots.resize(d + 1);
    c->fri_roots[d].assign(root, root + 32);
}

int step::fri_commit_natural(dst_ctx* c, int d0) {
    const int L = c->num_fri_layers;
    digest* d_roots = reinterpret_cast<digest*>(c->d_fri_chain);
    fe* d_alpha = reinterpret_cast<fe*>(c->d_fri_chain + DST_MAX_FRI_LAYERS * 32);
    uint8_t* h_roots = c->h_stage + HS_FRI_ROOTS;                      // page-locked: queued, picked up after the wait below
    int d = d0;
    for (; d < L && !fri_tail_starts_at(c, d); d++) {
        const size_t R = c->fri_size[d] / 4;
        const bool coset_major = d == 0 && !c->sharded_layout;        // the composition as the single-GPU phases leave it
        const fe* e = fri_layer_natural(c, d);
        if (coset_major) k_fri_leaves_layer0(c); else k_fri_leaves_at(c, e, c->fri_leaves[d], R);
        k_merkle(c, c->fri_leaves[d], c->fri_nodes[d], R, 0);
        k_fri_draw(c, d, d_alpha + d, d_roots + d);
        if (d + 1 == L) continue;
        if (coset_major) k_fri_fold_dev(c, 0, d_alpha); else k_fri_fold_at(c, e, c->fri_e[d + 1], R, d, fe_zero(), d_alpha + d);
    }
    if (d > d0) HIP_TRY(c, hipMemcpyAsync(h_roots, d_roots + d0, (size_t)(d - d0) * 32, hipMemcpyDeviceToHost, c->stream));
    if (d < L) {
        // the small layers in one launch: their evaluations are in fri_e[d ..] in natural order
        uint8_t tail_roots[DST_MAX_FRI_LAYERS * 32];
        if (int rt = k_fri_tail(c, d, tail_roots)) return rt;          // waits for the stream
        for (int i = d; i < L; i++) fri_file_root(c, i, tail_roots + 32 * (i - d));
    } else {
        CTX_SYNC(c, "the gathered FRI layer");
        HIP_TRY(c, hipGetLastError());
    }
    for (int i = d0; i < d; i++) fri_file_root(c, i, h_roots + 32 * (i - d0));
    c->fri_committed = L; c->fri_folded = L - 1;
    return DST_OK;
}

void step::fri_shard_layer(dst_ctx* c, int d) {
    const size_t nd = fri_nd(c, d), nb = nd / 4;
    k_fri_leaves_cm(c, c->fri_e[d], c->fri_leaves[d], nd);
    k_merkle(c, c->fri_leaves[d], c->fri_nodes[d], nb * c->Bc, nb);
    c->fri_committed = d + 1;
}
void step::fri_shard_fold(dst_ctx* c, int d, fe x, const fe* alpha_dev) {
    k_fri_fold_cm(c, c->fri_e[d], c->fri_e[d + 1], fri_nd(c, d), d, x, alpha_dev);
    c->fri_folded = d + 1;
}

// ---- step 8 ---------------------------------------------------------------------------------------------------------------------
int step::query_seed(dst_ctx* c, uint64_t* nonce, std::vector<uint64_t>& positions) {
    std::vector<uint8_t> roots;
    for (int d = 0; d < c->num_fri_layers; d++) roots.insert(roots.end(), c->fri_roots[d].begin(), c->fri_roots[d].end());
    uint8_t seed0[32], seed1[32];
    if (!blake3_short(roots.data(), roots.size(), seed0)) { c->err = "too many FRI roots"; return DST_ERR_ARG; }   // prover.rs:120-127
    if (int r = dst_pow_grind(c, seed0, c->prm.grinding_factor, seed1, nonce)) return r;
    if (query_positions(seed1, c->N, (uint32_t)c->B, c->prm.num_queries, positions)) { c->err = "could not generate enough query positions"; return DST_ERR_ARG; }
    return DST_OK;
}
