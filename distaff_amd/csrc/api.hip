// C-ABI of libdistaff_hip.so (include/distaff_hip.h): context, tables, the prover phases and proof assembly.  The verifier (verify/), the
// shared prover steps (host/steps_impl.h) and the Rescue trees (host/rtree_impl.h, host/stree_impl.h) are host code compiled with this unit.
// The phase order and every Fiat-Shamir dependency follow stark::prove (/root/reference/src/stark/prover.rs:17-168).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "ctx.h"
#include "host/ctx_tables.h"     // root powers, shared with k_ntt_init (kernels_ntt.hip)
#include "host/steps.h"
#include "host_proof.h"
#include "host_util.h"
#include "host_vm.h"
#include "verify/host_verify.h"

using namespace dsth;
#include "host/steps_impl.h"    // the steps this file's drivers share with shard.hip's (host/steps.h), compiled with this unit
using step::wall_ms;
using step::event_ms;

static std::string g_create_error;

// periodic constants of the AIR over a cycle of 16*8 steps: interpolate each 16-entry row, evaluate at w_128^s
// (constraints/utils.rs:87-113; decoder/mod.rs:95-100,219-223; stack/mod.rs:67-70)
static std::vector<fe> build_periodic_table() {
    const size_t cyc = 128;
    std::vector<fe> out(cyc * AIR_PERIODIC_STRIDE);
    u128 w16 = fe_to_u128(h_root_of_unity(4)), w128 = fe_to_u128(h_root_of_unity(7));
    u128 w16_inv = hf_pow(w16, 15), inv16 = hf_pow(16, FIELD_P - 2);
    static const uint8_t masks[3][16] = {{0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0}, {0, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1}};
    for (int row = 0; row < 23; row++) {
        u128 vals[16], coef[16];
        for (int i = 0; i < 16; i++) vals[i] = row < 8 ? limbs(SPONGE_ARK[row][i]) : row < 20 ? limbs(HASHER_ARK[row - 8][i]) : (u128)masks[row - 20][i];
        for (int j = 0; j < 16; j++) {
            u128 acc = 0;
            for (int i = 0; i < 16; i++) acc = hf_add(acc, hf_mul(vals[i], hf_pow(w16_inv, (u128)((i * j) % 16))));
            coef[j] = hf_mul(acc, inv16);
        }
        for (size_t s = 0; s < cyc; s++) {
            u128 x = hf_pow(w128, s), acc = 0, pw = 1;
            for (int j = 0; j < 16; j++) { acc = hf_add(acc, hf_mul(coef[j], pw)); pw = hf_mul(pw, x); }
            out[s * AIR_PERIODIC_STRIDE + row] = fe_from_u128(acc);
        }
    }
    // columns 23..28: the cubes of the first hasher constants (rows 8..13) -- what (item + constant)^3 is for a stack item that is not
    // part of the trace (zero): the constraint kernel of a shallow stack reads them instead of cubing
    for (size_t s = 0; s < cyc; s++)
        for (int i = 0; i < 6; i++) { const u128 v = fe_to_u128(out[s * AIR_PERIODIC_STRIDE + 8 + i]); out[s * AIR_PERIODIC_STRIDE + 23 + i] = fe_from_u128(hf_mul(hf_mul(v, v), v)); }
    return out;
}

static int ctx_init(dst_ctx* c) {
    c->read_switches();                                  // the DISTAFF_* variables as they are NOW; nothing reads the environment after this
    const dst_params& p = c->prm;
    if (p.log_trace_length < 4 || p.log_trace_length > 24) { c->err = "log_trace_length must be in [4, 24]"; return DST_ERR_ARG; }      // lib.rs:82 MIN_TRACE_LENGTH = 16
    if (p.log_blowup < 4 || p.log_blowup > 8) { c->err = "extension factor must be in [16, 256]"; return DST_ERR_ARG; }
    if (p.ctx_depth > 16 || p.loop_depth > 8) { c->err = "context / loop depth out of range"; return DST_ERR_ARG; }
    if (p.width >= 128 || p.width <= 15 + p.ctx_depth + p.loop_depth) { c->err = "register count out of range"; return DST_ERR_ARG; }
    if (p.num_queries == 0 || p.num_queries > 128 || p.grinding_factor > 32) { c->err = "invalid proof options"; return DST_ERR_ARG; }
    if (p.world == 0 || p.rank >= p.world || (p.world & (p.world - 1)) || p.world > 8 || p.world > (1u << p.log_blowup) / 2) {
        // a rank needs >= 1 of the 8 evaluation cosets and >= 2 LDE cosets (one constraint-tree leaf = a pair of neighbouring cosets)
        c->err = "invalid rank / world: world must be a power of two <= min(8, blowup / 2)"; return DST_ERR_ARG;
    }
    if (p.log_trace_length + p.log_blowup > 40) { c->err = "LDE domain exceeds 2^40"; return DST_ERR_ARG; }
    c->log_n = p.log_trace_length; c->log_b = p.log_blowup; c->log_N = c->log_n + c->log_b;
    c->n = (size_t)1 << c->log_n; c->B = (size_t)1 << c->log_b; c->N = c->n * c->B; c->W = p.width;
    c->Bc = c->B / p.world; c->j0 = c->Bc * p.rank;
    c->stack_depth = p.width - 15 - p.ctx_depth - p.loop_depth;
    if (c->stack_depth > 32) { c->err = "user stack deeper than 32 registers"; return DST_ERR_ARG; }
    c->device = p.device;
    HIP_TRY(c, hipSetDevice(c->device));
    int r;
    if ((r = ctx_stream(c, &c->stream))) return r;
    if ((r = ctx_pinned(c, &c->h_stage, HS_TOTAL))) return r;
    for (hipEvent_t& e : c->ph_ev) if ((r = ctx_event(c, &e))) return r;

    // twiddle tables
    fe wN = h_root_of_unity(c->log_N), wN_inv = h_inv(wN);
    c->tw_lo_bits = (c->log_N + 1) / 2;
    uint32_t hi_bits = c->log_N - c->tw_lo_bits;
    if ((r = dev_upload(c, &c->tw_lo, h_powers(wN, (size_t)1 << c->tw_lo_bits)))) return r;
    if ((r = dev_upload(c, &c->tw_hi, h_powers(h_pow(wN, (u128)1 << c->tw_lo_bits), (size_t)1 << hi_bits)))) return r;
    if ((r = dev_upload(c, &c->itw_lo, h_powers(wN_inv, (size_t)1 << c->tw_lo_bits)))) return r;
    if ((r = dev_upload(c, &c->itw_hi, h_powers(h_pow(wN_inv, (u128)1 << c->tw_lo_bits), (size_t)1 << hi_bits)))) return r;
    if ((r = k_ntt_init(c))) return r;                   // transform plan, its tables and LDS limits (kernels_ntt.hip)
    if ((r = dev_upload(c, &c->periodic, build_periodic_table()))) return r;
    c->n_inv = fe_from_u128(hf_pow((u128)c->n, FIELD_P - 2));
    c->n_inv_tw = fe_tw_make(c->n_inv);
    c->eight_inv = fe_from_u128(hf_pow(8, FIELD_P - 2));
    c->four_inv = fe_from_u128(hf_pow(4, FIELD_P - 2));
    c->iota = h_root_of_unity(2);
    c->g_trace = h_root_of_unity(c->log_n);
    c->x_last = h_inv(c->g_trace);

    // data buffers
    const size_t n = c->n, Nl = c->Bc * n;
    // sharded contexts: the coefficient vectors are all-gathered in rounds of `world` registers (dst_prove_sharded), so the array holds
    // a whole number of rounds
    if ((r = dev_alloc(c, &c->polys, (c->W + c->prm.world - 1) / c->prm.world * c->prm.world * n))) return r;
    if (c->plan.coeff_tile_major && (r = dev_alloc(c, &c->polys_tm, c->W * n))) return r;      // the coefficients in the extension's tile order (ctx.h)
    if ((r = dev_alloc(c, &c->lde, c->W * Nl))) return r;
    if (c->j0 == 0 && c->Bc > 1 && !c->sw_is("DISTAFF_TRACE_BUFFER", "1")) { c->trace = c->lde; c->trace_stride = Nl; }     // see ctx.h; DISTAFF_TRACE_BUFFER=1: separate buffer + copy (tests)
    else { if ((r = dev_alloc(c, &c->trace, c->W * n))) return r; c->trace_stride = n; }
    // staging buffer of the two-pass transforms: tmp_regs registers x Bc cosets per pair of launches.  Every launch ends with a partly
    // filled last wave of workgroups (4 registers x 31 cosets at n = 2^20: 7.75 waves of 512 resident workgroups), so as many registers per
    // launch as 12 GiB of staging hold (all 20 at n = 2^20: 39.75 waves, one tail instead of five); at least 4.  DISTAFF_TMP_REGS overrides.
    // The cap follows the free memory of the device at creation (several contexts may share one GPU: thread-ranks, tests): at most 12 GiB
    // and at most a quarter of what is free after the buffers above.
    size_t stage_cap = (size_t)12 << 30;
    { size_t free_b = 0, total_b = 0; if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b / 4 < stage_cap) stage_cap = free_b / 4; }
    c->tmp_regs = 4;
    while (c->tmp_regs < c->W && (c->tmp_regs + 1) * (c->plan.count == 3 ? 2 : 1) * c->Bc * n * sizeof(fe) <= stage_cap) c->tmp_regs++;
    if (const char* e = c->sw("DISTAFF_TMP_REGS")) { const long k = atol(e); if (k >= 4 && k <= (long)c->W) c->tmp_regs = (size_t)k; }
    if ((r = dev_alloc(c, &c->tmp, c->Bc * c->tmp_regs * n))) return r;
    if (c->plan.count == 3 && (r = dev_alloc(c, &c->tmp2, c->Bc * c->tmp_regs * n))) return r;
    if ((r = dev_alloc(c, &c->trace_leaves, Nl))) return r;
    if ((r = dev_alloc(c, &c->trace_nodes, Nl))) return r;
    if ((r = dev_alloc(c, &c->ceval, 3 * 8 * n))) return r;
    if ((r = dev_alloc(c, &c->cwork, 8 * 8 * n))) return r;
    if (c->j0 == 0 && (r = dev_alloc(c, &c->check_partials, k_air_check_partials(c) * n))) return r;     // the owner of coset 0 checks the trace rows (kernels_air.hip k_air_check)
    if ((r = dev_alloc(c, &c->cpoly, 8 * n))) return r;
    if ((r = dev_alloc(c, &c->cevals, Nl))) return r;
    if ((r = dev_alloc(c, &c->cnodes, Nl / 2))) return r;
    if ((r = dev_alloc(c, &c->comp_poly, 8 * n))) return r;
    if ((r = dev_alloc(c, &c->comp, Nl))) return r;
    c->scratch_elems = (size_t)1 << 21;
    if ((r = dev_alloc(c, &c->scratch, c->scratch_elems))) return r;
    if ((r = dev_alloc(c, &c->d_u64, 64))) return r;
    if ((r = dev_alloc(c, &c->d_fri_chain, DST_MAX_FRI_LAYERS * 48))) return r;
    c->stage_bytes = (size_t)8 << 20;
    if ((r = dev_alloc(c, &c->d_stage, c->stage_bytes))) return r;
    // FRI layers: sizes N, N/4, ... while > 256; the last one (<= 256) is the remainder (fri/prover.rs:21, fri/mod.rs:13)
    size_t sz = c->N;
    int d = 0;
    for (;; d++) {
        if (d >= DST_MAX_FRI_LAYERS) { c->err = "too many FRI layers"; return DST_ERR_ARG; }
        c->fri_size[d] = sz;
        if (d == 0) c->fri_e[0] = c->comp;
        else if ((r = dev_alloc(c, &c->fri_e[d], sz))) return r;
        if ((r = dev_alloc(c, &c->fri_leaves[d], sz / 4))) return r;
        if ((r = dev_alloc(c, &c->fri_nodes[d], sz / 4))) return r;
        if (sz <= 256) break;
        sz /= 4;
    }
    c->num_fri_layers = d + 1;
    return DST_OK;
}

static const fe* as_fe(const uint8_t* p) { return reinterpret_cast<const fe*>(p); }
static std::vector<fe> copy_fe(const uint8_t* p, size_t count) { std::vector<fe> v(count); memcpy(v.data(), p, count * 16); return v; }

// How every upload entry point opens: an asynchronous upload still in flight writes the same buffer from upload_stream, so it is drained
// before another upload starts.  So is whatever else may still touch the trace buffer beside the main stream.
static int upload_begin(dst_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    { const int r = k_air_check_drain(c); if (r) return r; }    // a check of the trace rows on the side stream still reads that buffer
    if (c->upload_pending && c->upload_stream) HIP_TRY(c, hipStreamSynchronize(c->upload_stream));
    c->upload_pending = false;
    return DST_OK;
}
// ... and how it closes: where the trace is now, and that nothing has been derived from it yet
static int upload_end(dst_ctx* c, bool pending, bool owned_only) {
    c->upload_pending = pending; c->trace_owned_only = owned_only;
    c->have_trace = true; c->committed = c->constraints_done = c->composed = false;
    return DST_OK;
}

// The exported functions below have C linkage and default visibility through their declarations in include/distaff_hip.h; everything
// else in this file is ordinary C++ and stays inside the library.

int dst_ctx_create(const dst_params* params, dst_ctx** out) {
    if (!params || !out) { g_create_error = "null argument"; return DST_ERR_ARG; }
    dst_ctx* c = new dst_ctx();
    c->prm = *params;
    int r = ctx_init(c);
    if (r == DST_OK && c->prm.world > 1) r = ensure_shard_buffers(c);       // a rank can join every collective from its first proof on
    if (r != DST_OK) { g_create_error = c->err; free_all(c); delete c; *out = nullptr; return r; }
    *out = c;
    return DST_OK;
}
void dst_ctx_destroy(dst_ctx* c) { if (!c) return; hipSetDevice(c->device); (void)k_air_check_drain(c); free_all(c); delete c; }
int64_t dst_last_bad_step(const dst_ctx* c) { return (!c || c->air_flag_host == ~0ull) ? -1 : (int64_t)c->air_flag_host; }
const char* dst_last_error(const dst_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }
int dst_phase_ms(const dst_ctx* c, double out_ms[9]) { if (!c || !out_ms) return DST_ERR_ARG; for (int i = 0; i < 9; i++) out_ms[i] = c->phase_ms[i]; return DST_OK; }

int dst_trace_upload(dst_ctx* c, const uint8_t* const* cols) {
    if (!c || !cols) return DST_ERR_ARG;
    { const int r = upload_begin(c); if (r) return r; }
    for (size_t i = 0; i < c->W; i++) HIP_TRY(c, hipMemcpyAsync(c->trace + i * c->trace_stride, cols[i], c->n * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return upload_end(c, false, false);
}
// Sharded contexts: uploads only the registers this rank interpolates, r = rank (mod world) -- 1/world of the trace per GPU instead of
// all of it.  cols[r] of the other registers is not read (may be NULL).  Only dst_prove_sharded accepts a context in this state.
int dst_trace_upload_owned(dst_ctx* c, const uint8_t* const* cols) {
    if (!c || !cols) return DST_ERR_ARG;
    { const int r = upload_begin(c); if (r) return r; }
    for (size_t i = c->prm.rank; i < c->W; i += c->prm.world) {
        if (!cols[i]) { c->err = "dst_trace_upload_owned: register " + std::to_string(i) + " belongs to this rank but has no data"; return DST_ERR_ARG; }
        HIP_TRY(c, hipMemcpyAsync(c->trace + i * c->trace_stride, cols[i], c->n * 16, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return upload_end(c, false, c->prm.world > 1);
}
int dst_trace_upload_contiguous(dst_ctx* c, const uint8_t* cols) {
    if (!c || !cols) return DST_ERR_ARG;
    { const int r = upload_begin(c); if (r) return r; }
    for (size_t i = 0; i < c->W; i++) HIP_TRY(c, hipMemcpy(c->trace + i * c->trace_stride, cols + i * c->n * 16, c->n * 16, hipMemcpyHostToDevice));
    return upload_end(c, false, false);
}

// Pinned host memory for the trace: the reference hands stark::prove a host-resident TraceTable (prover.rs:17, trace_table.rs:10); from
// pinned memory the upload runs as asynchronous DMA and overlaps with the extension of the registers that have already arrived.
int dst_pinned_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return DST_ERR_ARG;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? DST_OK : DST_ERR_HIP;
}
int dst_pinned_free(void* p) { return (!p || hipHostFree(p) == hipSuccess) ? DST_OK : DST_ERR_HIP; }

// Starts the upload of the W register columns (host pointers, ideally from dst_pinned_alloc) on a copy stream and returns at once.  The
// next dst_commit_trace / dst_prove interpolates and extends the registers group by group as their copies complete, so only the first
// group's transfer is exposed.  The host buffers must stay valid until that call returns.
int dst_trace_upload_async(dst_ctx* c, const uint8_t* const* cols) {
    if (!c || !cols) return DST_ERR_ARG;
    { const int r = upload_begin(c); if (r) return r; }
    if (!c->upload_stream) { const int r = ctx_stream(c, &c->upload_stream, hipStreamNonBlocking); if (r) return r; }
    // the previous proof's kernels may still read the buffer on c->stream (coset 0 of the extension IS the trace buffer)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // groups of 4 registers (one extension launch, see k_lde_columns) -- except that the first group is ONE register: its transfer is the
    // only one nothing overlaps with
    c->upload_bounds.clear();
    for (size_t first = 0; first < c->W;) { c->upload_bounds.push_back(first); first += (first == 0 && c->W > 4) ? (c->W % 4 ? c->W % 4 : 1) : 4; }
    c->upload_bounds.push_back(c->W);
    const size_t groups = c->upload_bounds.size() - 1;
    while (c->upload_done.size() < groups) { hipEvent_t e; const int r = ctx_event(c, &e, hipEventDisableTiming); if (r) return r; c->upload_done.push_back(e); }
    for (size_t g = 0; g < groups; g++) {
        for (size_t i = c->upload_bounds[g]; i < c->upload_bounds[g + 1]; i++)
            HIP_TRY(c, hipMemcpyAsync(c->trace + i * c->trace_stride, cols[i], c->n * 16, hipMemcpyHostToDevice, c->upload_stream));
        HIP_TRY(c, hipEventRecord(c->upload_done[g], c->upload_stream));
    }
    return upload_end(c, true, false);
}

// ---- steps 1-2 ------------------------------------------------------------------------------------------------------------------
int dst_commit_trace(dst_ctx* c, uint8_t trace_root[32]) {
    if (!c || !trace_root) return DST_ERR_ARG;
    if (!c->have_trace) { c->err = "dst_commit_trace: no trace uploaded"; return DST_ERR_STATE; }
    if (c->trace_owned_only) { c->err = "dst_commit_trace: only this rank's registers were uploaded (dst_trace_upload_owned): use dst_prove_sharded"; return DST_ERR_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    c->sharded_layout = false;
    double t0 = wall_ms();
    HIP_TRY(c, hipEventRecord(c->ph_ev[4], c->stream));
    if (c->upload_pending) {
        // registers arrive in groups (dst_trace_upload_async): each group is interpolated and extended as soon as its copy has landed
        for (size_t g = 0; g + 1 < c->upload_bounds.size(); g++) {
            const size_t first = c->upload_bounds[g], cnt = c->upload_bounds[g + 1] - first;
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->upload_done[g], 0));
            k_intt_columns(c, c->trace + first * c->trace_stride, c->trace_stride, c->polys + first * c->n, cnt, polys_tm_at(c, first));
            k_lde_columns(c, c->polys + first * c->n, c->lde + first * c->Bc * c->n, cnt, polys_tm_at(c, first));
        }
        c->upload_pending = false;
    } else {
        k_intt_columns(c, c->trace, c->trace_stride, c->polys, c->W, c->polys_tm);   // interpolate_fft_twiddles (trace_table.rs:159)
        k_lde_columns(c, c->polys, c->lde, c->W, c->polys_tm);       // eval_fft_twiddles over the LDE domain (trace_table.rs:166)
    }
    HIP_TRY(c, hipEventRecord(c->ph_ev[5], c->stream));         // end of the extension: the host does not wait here
    k_trace_leaves(c);                                           // trace_table.rs:174-185
    k_merkle(c, c->trace_leaves, c->trace_nodes, c->Bc * c->n, 0);
    HIP_TRY(c, hipMemcpyAsync(c->trace_root, c->trace_nodes + 1, 32, hipMemcpyDeviceToHost, c->stream));
    // last state of the un-extended trace: op counter and program hash (evaluator.rs:37,73-74)
    fe last[3];
    for (int i = 0; i < 3; i++) HIP_TRY(c, hipMemcpyAsync(&last[i], c->trace + (size_t)i * c->trace_stride + (c->n - 1), 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    c->op_count = (uint64_t)fe_to_u128(last[0]); c->op_counter = last[0];
    c->program_hash[0] = last[1]; c->program_hash[1] = last[2];
    memcpy(trace_root, c->trace_root, 32);
    {
        // extension = what the stream spent up to the event; the rest of the call's wall time is the tree (and the host's share)
        const double total = wall_ms() - t0;
        double lde_ms = event_ms(c->ph_ev[4], c->ph_ev[5]);
        if (lde_ms < 0 || lde_ms > total) lde_ms = 0;
        c->phase_ms[0] = lde_ms; c->phase_ms[1] = total - lde_ms;
    }
    c->committed = true; c->constraints_done = c->composed = false;
    return DST_OK;
}

// ---- steps 3-5 ------------------------------------------------------------------------------------------------------------------
// (the evaluation and combine_polys are stated in host/steps_impl.h, for this driver and the sharded ones)
static int eval_constraints_phase(dst_ctx* c, const dst_public* pub, const uint8_t* coeffs, uint8_t constraint_root[32], int64_t* bad_step, bool check_here);
int dst_eval_constraints(dst_ctx* c, const dst_public* pub, const uint8_t* coeffs, uint8_t constraint_root[32], int64_t* bad_step) {
    return eval_constraints_phase(c, pub, coeffs, constraint_root, bad_step, true);
}
// check_here = false (dst_prove): the check of the trace rows is queued by the caller, who also reports its verdict
static int eval_constraints_phase(dst_ctx* c, const dst_public* pub, const uint8_t* coeffs, uint8_t constraint_root[32], int64_t* bad_step, bool check_here) {
    if (!c || !pub || !coeffs || !constraint_root) return DST_ERR_ARG;
    if (!c->committed) { c->err = "dst_eval_constraints: trace not committed"; return DST_ERR_STATE; }
    if (pub->num_inputs > 8 || pub->num_outputs > 8) { c->err = "too many public inputs / outputs"; return DST_ERR_ARG; }
    if (c->prm.world != 1) { c->err = "dst_eval_constraints: multi-GPU combination is driven by the host (see distaff_amd/sharded.py)"; return DST_ERR_ARG; }
    HIP_TRY(c, hipSetDevice(c->device));
    const double t0 = wall_ms();
    HIP_TRY(c, hipEventRecord(c->ph_ev[0], c->stream));
    // The host does not wait for the evaluation's verdict (evaluator.rs:152-158) before it queues the combination: the flag travels back
    // with the constraint root, and a trace that fails is reported then (the work queued behind it is wasted only in that case).
    const bool steps = dst_internal_combine_by_steps(c);
    int r = step::eval_constraints(c, pub, coeffs, bad_step, /*defer_check=*/!steps, check_here);
    if (r != DST_OK) return r;
    HIP_TRY(c, hipEventRecord(c->ph_ev[1], c->stream));
    if ((r = step::combine(c, 3))) return r;
    HIP_TRY(c, hipEventRecord(c->ph_ev[2], c->stream));
    // constraint_poly.eval + Merkle tree over raw evaluation pairs (prover.rs:82-86)
    k_lde_fold8(c, c->cpoly, c->cevals);
    k_constraint_tree(c);
    HIP_TRY(c, hipMemcpyAsync(c->constraint_root, c->cnodes + 1, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->ph_ev[3], c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (!steps && check_here) {
        c->air_flag_host = *reinterpret_cast<unsigned long long*>(c->h_stage + HS_AIR_FLAG);
        if ((r = k_constraint_check(c, bad_step)) != DST_OK) { c->err = "transition constraints were not satisfied"; return r; }
    }
    memcpy(constraint_root, c->constraint_root, 32);
    // phase times from the stream's own clock; what the host spent before the first and after the last event goes to the outer phases
    auto between = [&](int from, int to) { const double ms = event_ms(c->ph_ev[from], c->ph_ev[to]); return ms > 0 ? ms : 0.0; };     // unknown counts as nothing
    const double total = wall_ms() - t0, e1 = between(0, 1), e2 = between(1, 2), e3 = between(2, 3);
    const double rest = total > e1 + e2 + e3 ? total - (e1 + e2 + e3) : 0.0;
    c->phase_ms[2] = e1 + rest / 2; c->phase_ms[3] = e2; c->phase_ms[4] = e3 + rest / 2;
    c->constraints_done = true; c->composed = false;
    return DST_OK;
}

// ---- step 6 ---------------------------------------------------------------------------------------------------------------------
// the DeepValues land in page-locked memory; a caller that did not wait (dst_prove) picks them up at its next synchronisation
static void finish_deep_values(dst_ctx* c) {
    if (!c->deep_pending) return;
    const size_t W = c->W;
    c->deep_z1.assign(c->h_stage + HS_DEEP, c->h_stage + HS_DEEP + W * 16);
    c->deep_z2.assign(c->h_stage + HS_DEEP + HS_DEEP_HALF, c->h_stage + HS_DEEP + HS_DEEP_HALF + W * 16);
    c->deep_pending = false;
}
static int compose_impl(dst_ctx* c, const uint8_t* draws_bytes, uint8_t* trace_at_z1, uint8_t* trace_at_z2, bool wait);
int dst_compose(dst_ctx* c, const uint8_t* draws_bytes, uint8_t* trace_at_z1, uint8_t* trace_at_z2) {
    if (!c || !draws_bytes || !trace_at_z1 || !trace_at_z2) return DST_ERR_ARG;
    return compose_impl(c, draws_bytes, trace_at_z1, trace_at_z2, true);
}
static int compose_impl(dst_ctx* c, const uint8_t* draws_bytes, uint8_t* trace_at_z1, uint8_t* trace_at_z2, bool wait) {
    if (!c->constraints_done) { c->err = "dst_compose: constraints not evaluated"; return DST_ERR_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    double t0 = wall_ms();
    HIP_TRY(c, hipEventRecord(c->ph_ev[0], c->stream));         // device-side extent of the composition (dst_prove does not wait for it)
    const size_t n = c->n, D = 8 * n, W = c->W;
    std::vector<fe> draws = copy_fe(draws_bytes, 516);
    const fe z = draws[0];
    const fe next_z = fe_mul(z, c->g_trace);
    const fe k1 = draws[513], k2 = draws[514], k3 = draws[515];
    const step::ScratchTail tail(c);
    fe* d_draws = tail.draws(); fe* d_tz1 = tail.tz1(); fe* d_tz2 = tail.tz2(); fe* d_cz = tail.cz();
    {   // queued from the page-locked staging area: `draws` goes out of scope while the copy may still be pending (wait == false)
        fe* h_draws = reinterpret_cast<fe*>(c->h_stage + HS_COMPOSE);
        memcpy(h_draws, draws.data(), 516 * 16);
        HIP_TRY(c, hipMemcpyAsync(d_draws, h_draws, 516 * 16, hipMemcpyHostToDevice, c->stream));
    }
    // trace_table.rs:206-261
    const bool steps = dst_internal_combine_by_steps(c);
    const fe zz[2] = {z, next_z};
    k_horner(c, c->polys, W, n, z, d_tz1);
    k_horner(c, c->polys, W, n, next_z, d_tz2);
    fe* t1 = c->cwork; fe* t2 = c->cwork + n; fe* cp = c->cwork + D;
    k_lincomb2(c, c->polys, W, n, d_draws + 1, 256, t1, t2);          // both combinations in one pass over the trace polynomials
    const size_t inc = 6 * n + 1;                                // get_incremental_trace_degree (utils/mod.rs:20)
    if (steps) {
        k_sub_dot_at0(c, t1, d_tz1, d_draws + 1, W);
        k_sub_dot_at0(c, t2, d_tz2, d_draws + 257, W);
        k_syn_div(c, t1, n, z);
        k_syn_div(c, t2, n, next_z);
        k_add(c, t1, t2, n);
        HIP_TRY(c, hipMemsetAsync(c->comp_poly, 0, D * 16, c->stream));
        k_axpy(c, c->comp_poly, t1, k1, n);
        k_axpy(c, c->comp_poly + inc, t1, k2, n);
        // constraint_poly.rs:39-52 merge_into
        k_horner(c, c->cpoly, 1, D, z, d_cz);
        HIP_TRY(c, hipMemcpyAsync(cp, c->cpoly, D * 16, hipMemcpyDeviceToDevice, c->stream));
        k_sub_at0(c, cp, d_cz);
        k_syn_div(c, cp, D, z);
        k_axpy(c, c->comp_poly, cp, k3, D);
    } else {
        // The constant term of a dividend enters no coefficient of its quotient by (x - b), so the subtractions of T(z), T(z g) and C(z)
        // (trace_table.rs:226-233, constraint_poly.rs:44) need not be made -- and C(z) need not be evaluated.  The division of the
        // constraint polynomial writes the composition polynomial directly: k3 * quotient + (k1 + k2 x^inc) * t1.
        fe* both[2] = {t1, t2};
        k_syn_div_batch(c, both, zz, 2, n);
        k_add(c, t1, t2, n);
        k_syn_div_compose(c, c->cpoly, c->comp_poly, D, z, t1, n, inc, k1, k2, k3);
    }
    // evaluate over the LDE domain (prover.rs:98-101)
    k_lde_fold8(c, c->comp_poly, c->comp);
    HIP_TRY(c, hipEventRecord(c->ph_ev[1], c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->h_stage + HS_DEEP, d_tz1, W * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->h_stage + HS_DEEP + HS_DEEP_HALF, d_tz2, W * 16, hipMemcpyDeviceToHost, c->stream));
    c->deep_pending = true;
    if (wait) {
        CTX_SYNC(c, "the DEEP composition");
        HIP_TRY(c, hipGetLastError());
        finish_deep_values(c);
        memcpy(trace_at_z1, c->deep_z1.data(), W * 16);
        memcpy(trace_at_z2, c->deep_z2.data(), W * 16);
    }
    c->phase_ms[5] = wall_ms() - t0;        // without the wait: the host's share only; the first FRI layer's wait absorbs the rest (dst_prove adds it back)
    c->composed = true; c->fri_committed = 0; c->fri_folded = 0; c->fri_roots.clear(); c->fri_tail_pending = false;
    return DST_OK;
}

// ---- step 7 ---------------------------------------------------------------------------------------------------------------------
int dst_fri_commit_layer(dst_ctx* c, uint8_t layer_root[32], int* more) {
    if (!c || !layer_root || !more) return DST_ERR_ARG;
    if (!c->composed) { c->err = "dst_fri_commit_layer: composition not built"; return DST_ERR_STATE; }
    int d = c->fri_committed;
    if (d >= c->num_fri_layers || d != c->fri_folded) { c->err = "dst_fri_commit_layer: fold the previous layer first"; return DST_ERR_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    double t0 = wall_ms();
    if (d == 0) k_fri_leaves_layer0(c); else k_fri_leaves(c, d);
    k_merkle(c, c->fri_leaves[d], c->fri_nodes[d], c->fri_size[d] / 4, 0);
    uint8_t root[32];
    HIP_TRY(c, hipMemcpyAsync(root, c->fri_nodes[d] + 1, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    memcpy(layer_root, root, 32);
    step::fri_file_root(c, d, root);
    c->fri_committed = d + 1;
    *more = (d + 1 < c->num_fri_layers) ? 1 : 0;
    if (d == 0) c->phase_ms[6] = 0;
    c->phase_ms[6] += wall_ms() - t0;
    return DST_OK;
}
int dst_fri_fold(dst_ctx* c, const uint8_t special_x[16]) {
    if (!c || !special_x) return DST_ERR_ARG;
    int d = c->fri_folded;
    if (d + 1 != c->fri_committed || d + 1 >= c->num_fri_layers) { c->err = "dst_fri_fold: nothing to fold"; return DST_ERR_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    double t0 = wall_ms();
    k_fri_fold(c, d, fe_from_bytes(special_x));
    c->fri_folded = d + 1;
    c->phase_ms[6] += wall_ms() - t0;        // launch only; the next commit synchronises
    return DST_OK;
}

// ---- step 8 ---------------------------------------------------------------------------------------------------------------------
int dst_pow_grind(dst_ctx* c, const uint8_t seed[32], uint32_t grinding_factor, uint8_t out_seed[32], uint64_t* nonce) {
    if (!c || !seed || !out_seed || !nonce || grinding_factor > 64) return DST_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int r = k_pow(c, seed, grinding_factor, nonce);
    if (r != DST_OK) return r;
    uint8_t buf[64];
    memset(buf, 0, 64);
    memcpy(buf, seed, 32);
    memcpy(buf + 32, nonce, 8);
    blake3_short(buf, 64, out_seed);
    return DST_OK;
}

// ---- step 9 ---------------------------------------------------------------------------------------------------------------------
// (openings are planned, gathered and serialised in shard.hip: dst_shard_open / dst_shard_assemble)
int dst_build_proof(dst_ctx* c, const uint64_t* positions_in, uint32_t num_positions, uint64_t pow_nonce, uint8_t* out, size_t cap, size_t* out_len) {
    if (!c || !positions_in || !out_len) return DST_ERR_ARG;
    if (!c->composed || c->fri_committed != c->num_fri_layers) { c->err = "dst_build_proof: FRI commit phase not finished"; return DST_ERR_STATE; }
    if (c->prm.world != 1) { c->err = "dst_build_proof: single-GPU contexts only"; return DST_ERR_ARG; }
    HIP_TRY(c, hipSetDevice(c->device));
    double t0 = wall_ms();
    finish_deep_values(c);                                      // every FRI layer since has synchronised the stream
    // one plan, one batched device gather, one fill (shard.hip; the single-GPU case is the plan with every item local)
    std::vector<uint8_t> proof;
    int rc = build_proof_local(c, positions_in, num_positions, pow_nonce, proof);
    if (rc == DST_OK) {
        *out_len = proof.size();
        if (out) {
            if (cap < proof.size()) { c->err = "proof buffer too small"; rc = DST_ERR_ARG; }
            else memcpy(out, proof.data(), proof.size());
        }
    }
    c->phase_ms[8] = wall_ms() - t0;
    return rc;
}

// fri::reduce (fri/prover.rs:11-53) for dst_prove.  chained = true: no host round trip per layer (step::fri_commit_natural from layer 0).
// chained = false (DISTAFF_FRI_CHAIN=0, tests): one root read-back and one host draw per layer through the public phase calls, up to
// the single-launch tail.
static int fri_commit_all(dst_ctx* c, bool chained) {
    if (chained) {
        if (!c->composed || c->fri_committed != 0 || c->fri_folded != 0) { c->err = "dst_prove: FRI state"; return DST_ERR_STATE; }
        return step::fri_commit_natural(c, 0);
    }
    for (;;) {
        if (fri_tail_starts_at(c, c->fri_committed)) return step::fri_commit_natural(c, c->fri_committed);
        uint8_t root[32]; int more = 0, rc;
        if ((rc = dst_fri_commit_layer(c, root, &more))) return rc;
        if (!more) return DST_OK;
        fe sx = prng(root);
        if ((rc = dst_fri_fold(c, (const uint8_t*)&sx))) return rc;
    }
}

// ---- the whole prover -----------------------------------------------------------------------------------------------------------
// Where dst_prove queues the check of the trace rows (DISTAFF_AIR_CHECK, test build; the product library runs the default).  The verdict
// depends on the trace alone and nothing of the proof waits for it, so it need not stand on the main stream in the middle of the
// VALU-bound evaluation: on the side stream it runs beside the serial tail of the proof -- the small FRI layers, the proof of work, the
// openings -- where most of the device is idle.  profiles/air_trace_check.md has the measurements behind the default.
enum AirCheckPlace { AIR_CHECK_INLINE, AIR_CHECK_TRACE, AIR_CHECK_FRI, AIR_CHECK_POW, AIR_CHECK_OPEN };
static AirCheckPlace air_check_place(const dst_ctx* c) {
    if (c->sw_is("DISTAFF_AIR_CHECK", "inline")) return AIR_CHECK_INLINE;
    if (c->sw_is("DISTAFF_AIR_CHECK", "trace")) return AIR_CHECK_TRACE;
    if (c->sw_is("DISTAFF_AIR_CHECK", "fri")) return AIR_CHECK_FRI;
    if (c->sw_is("DISTAFF_AIR_CHECK", "open")) return AIR_CHECK_OPEN;
    return AIR_CHECK_POW;
}
static int prove_impl(dst_ctx* c, const dst_public* pub, uint8_t* proof_out, size_t cap, size_t* proof_len);
int dst_prove(dst_ctx* c, const dst_public* pub, uint8_t* proof_out, size_t cap, size_t* proof_len) {
    if (!c || !pub || !proof_len) return DST_ERR_ARG;
    int rc = prove_impl(c, pub, proof_out, cap, proof_len);
    // a check chain on the side stream: waited for on every path out of the proof, reported when nothing else failed first
    const bool aside = c->check_pending;
    const double t0 = wall_ms();
    const int rd = k_air_check_drain(c);
    if (aside) c->phase_ms[8] += wall_ms() - t0;
    if (rc == DST_OK && rd != DST_OK) rc = rd;
    if (rc == DST_OK && aside && k_constraint_check(c, nullptr) != DST_OK) { c->err = "transition constraints were not satisfied"; *proof_len = 0; rc = DST_ERR_AIR; }
    return rc;
}
static int prove_impl(dst_ctx* c, const dst_public* pub, uint8_t* proof_out, size_t cap, size_t* proof_len) {
    int rc;
    uint8_t trace_root[32], constraint_root[32];
    const AirCheckPlace place = air_check_place(c);
    if ((rc = dst_commit_trace(c, trace_root))) return rc;
    if (place == AIR_CHECK_TRACE && (rc = k_air_check_side(c))) return rc;          // the trace is all the check reads
    std::vector<fe> coef(344);
    prng_vector(trace_root, 344, coef.data());                   // ConstraintCoefficients::new (coefficients.rs:66)
    int64_t bad = -1;
    if ((rc = eval_constraints_phase(c, pub, (const uint8_t*)coef.data(), constraint_root, &bad, /*check_here=*/place == AIR_CHECK_INLINE))) return rc;
    std::vector<fe> draws(516);
    prng_vector(constraint_root, 516, draws.data());             // z = draw 0; CompositionCoefficients (coefficients.rs:82)
    // the DEEP values are not needed before the openings: the host queues the composition and goes on to the first FRI layer
    std::vector<uint8_t> z1(c->W * 16), z2(c->W * 16);
    const double t_compose = wall_ms();
    if ((rc = compose_impl(c, (const uint8_t*)draws.data(), z1.data(), z2.data(), false))) return rc;
    if (place == AIR_CHECK_FRI && (rc = k_air_check_side(c))) return rc;            // behind the composition, beside the commit phase that is queued next
    {
        const char* ce = c->sw("DISTAFF_FRI_CHAIN");
        if ((rc = fri_commit_all(c, !(ce && ce[0] == '0')))) return rc;
        // the commit phase's first wait covered the composition too: split at the device's own boundary (events of compose_impl)
        const double both = wall_ms() - t_compose, dev = event_ms(c->ph_ev[0], c->ph_ev[1]);
        if (dev > 0 && dev < both) { c->phase_ms[5] = dev; c->phase_ms[6] = both - dev; }
        else { c->phase_ms[6] = both > c->phase_ms[5] ? both - c->phase_ms[5] : 0.0; }
    }
    // the commit phase has been waited for: from here to the gather of the openings the device has the proof-of-work search and nothing else
    if (place == AIR_CHECK_POW && (rc = k_air_check_side(c))) return rc;
    double t0 = wall_ms();
    uint64_t nonce = 0;
    std::vector<uint64_t> positions;
    if ((rc = step::query_seed(c, &nonce, positions))) return rc;
    c->phase_ms[7] = wall_ms() - t0;
    if (place == AIR_CHECK_OPEN && (rc = k_air_check_side(c))) return rc;           // beside the host's opening plan
    return dst_build_proof(c, positions.data(), (uint32_t)positions.size(), nonce, proof_out, cap, proof_len);
}

// ---- host helpers ----------------------------------------------------------------------------------------------------------------
void dst_prng_vector(const uint8_t seed[32], uint32_t count, uint8_t* out) {
    std::vector<fe> v(count);
    prng_vector(seed, count, v.data());
    memcpy(out, v.data(), (size_t)count * 16);
}
int dst_query_positions(const uint8_t seed[32], uint64_t domain_size, uint32_t blowup, uint32_t num_queries, uint64_t* out) {
    // an error code, never an abort: a zero domain or extension factor would divide by zero, and the caller's buffer holds at most 128 positions
    if (!seed || !out || domain_size == 0 || blowup == 0 || num_queries == 0 || num_queries > 128) return DST_ERR_ARG;
    std::vector<uint64_t> p;
    if (query_positions(seed, domain_size, blowup, num_queries, p)) return DST_ERR_ARG;
    memcpy(out, p.data(), p.size() * 8);
    return (int)p.size();
}
void dst_blake3(const uint8_t* in, size_t len, uint8_t out[32]) { if (!blake3_short(in, len, out)) memset(out, 0, 32); }

int dst_fibonacci_trace(uint32_t log_n, uint8_t* cols, uint8_t program_hash[32], uint8_t result[16]) {
    if (!cols || !program_hash || !result || log_n < 7 || log_n > 26) return DST_ERR_ARG;
    u128 ph[2], res;
    int r = fibonacci_trace(log_n, (u128*)cols, ph, &res);
    if (r) return DST_ERR_ARG;
    memcpy(program_hash, ph, 32);
    memcpy(result, &res, 16);
    return DST_OK;
}

// ---- stark::verify on the host (verify/host_verify.h): no context, no HIP call --------------------------------------------------------
static void put_text(char* err, size_t err_cap, const std::string& s) { if (err && err_cap) snprintf(err, err_cap, "%s", s.c_str()); }
int dst_verify(const uint8_t program_hash[32], const dst_public* pub, const uint8_t* proof, size_t len, int* accepted, char* err, size_t err_cap) {
    if (accepted) *accepted = 0;
    put_text(err, err_cap, "");
    if (!program_hash || !pub || !accepted || pub->num_inputs > 8 || pub->num_outputs > 8) { put_text(err, err_cap, "invalid argument"); return DST_ERR_ARG; }
    hver::VProof p;
    std::string why;
    if (hver::parse_proof(proof, len, p, why)) { put_text(err, err_cap, why); return DST_ERR_ARG; }
    u128 in[8], out[8];
    memcpy(in, pub->inputs, sizeof(in)); memcpy(out, pub->outputs, sizeof(out));
    for (uint32_t i = 0; i < 8; i++)
        if ((i < pub->num_inputs && in[i] >= FIELD_P) || (i < pub->num_outputs && out[i] >= FIELD_P)) { put_text(err, err_cap, "public value not below the modulus"); return DST_ERR_ARG; }
    hver::VerifyResult r = hver::verify_proof(program_hash, in, pub->num_inputs, out, pub->num_outputs, p);
    *accepted = r.ok ? 1 : 0;
    put_text(err, err_cap, r.error);
    return DST_OK;
}
int dst_proof_info(const uint8_t* proof, size_t len, dst_proof_info_t* info) {
    if (!info) return DST_ERR_ARG;
    memset(info, 0, sizeof(*info));
    hver::VProof p;
    std::string why;
    if (hver::parse_proof(proof, len, p, why)) return DST_ERR_ARG;
    info->log_trace_length = (uint32_t)p.domain_depth - p.log_blowup;
    info->extension_factor = 1u << p.log_blowup; info->num_queries = p.num_queries; info->grinding_factor = p.grinding;
    info->ctx_depth = p.ctx_depth; info->loop_depth = p.loop_depth; info->stack_depth = p.stack_depth;
    info->register_count = 15u + p.ctx_depth + p.loop_depth + p.stack_depth;
    info->op_count = p.op_count;
    info->fri_layers = (uint32_t)p.layers.size(); info->remainder_length = (uint32_t)p.rem_values.size();
    info->security_level = hver::security_level(p, true); info->security_level_proven = hver::security_level(p, false);
    info->pow_nonce = p.pow_nonce;
    return DST_OK;
}

// ---- Rescue digests and Rescue Merkle trees (dst_rescue_digest_many, dst_rtree_*): no context, compiled with this unit ---------------------
#include "host/rtree_impl.h"
// ---- sparse Rescue Merkle trees: the same, over keys of up to 63 bits (dst_stree_*) and of up to 127 bits (dst_wtree_*) --------------------------
#include "host/stree_impl.h"
// ---- checking paths and the witnesses of ordered writes (dst_rescue_path_roots, dst_rescue_verify_*, their _w forms): no tree, no context -----
#include "host/path_verify_impl.h"
// ---- following ordered writes with held paths (dst_rescue_refresh_paths, its _w form): the same checks, then the paths under the new root ------
#include "host/path_refresh_impl.h"
// ---- compressed batch openings (dst_rescue_multiproof_*, dst_rtree_multiproof, dst_stree_multiproof): every shared ancestor once ------------
#include "host/multiproof_impl.h"

// ---- inspection --------------------------------------------------------------------------------------------------------------------
int dst_read_buffer(dst_ctx* c, uint32_t what, uint32_t arg, uint8_t* out, size_t cap, size_t* len) {
    if (!c || !len) return DST_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = c->n, Nl = c->Bc * n;
    const void* src = nullptr; size_t bytes = 0;
    const fe* coset_major = nullptr; size_t cosets = 0;
    switch (what) {
        case DST_BUF_POLYS: src = c->polys; bytes = c->W * n * 16; break;
        case DST_BUF_LDE: if (arg >= c->W) return DST_ERR_ARG; coset_major = c->lde + (size_t)arg * Nl; cosets = c->Bc; break;
        case DST_BUF_TRACE_LEAVES: src = c->trace_leaves; bytes = Nl * 32; break;
        case DST_BUF_TRACE_NODES: src = c->trace_nodes; bytes = Nl * 32; break;
        case DST_BUF_CEVAL_I: case DST_BUF_CEVAL_F: case DST_BUF_CEVAL_T: coset_major = c->ceval + (size_t)(what - DST_BUF_CEVAL_I) * 8 * n; cosets = 8; break;
        case DST_BUF_CPOLY: src = c->cpoly; bytes = 8 * n * 16; break;
        case DST_BUF_CEVALS: coset_major = c->cevals; cosets = c->Bc; break;
        case DST_BUF_CNODES: src = c->cnodes; bytes = Nl / 2 * 32; break;
        case DST_BUF_COMP_POLY: src = c->comp_poly; bytes = 8 * n * 16; break;
        case DST_BUF_COMP_EVALS: coset_major = c->comp; cosets = c->Bc; break;
        case DST_BUF_FRI_EVALS:
            if ((int)arg >= c->num_fri_layers) return DST_ERR_ARG;
            if (arg == 0) { coset_major = c->comp; cosets = c->Bc; } else { src = c->fri_e[arg]; bytes = c->fri_size[arg] * 16; }
            break;
        case DST_BUF_FRI_NODES: if ((int)arg >= c->num_fri_layers) return DST_ERR_ARG; src = c->fri_nodes[arg]; bytes = c->fri_size[arg] / 4 * 32; break;
        case DST_BUF_FRI_LEAVES: if ((int)arg >= c->num_fri_layers) return DST_ERR_ARG; src = c->fri_leaves[arg]; bytes = c->fri_size[arg] / 4 * 32; break;
        default: c->err = "unknown buffer id"; return DST_ERR_ARG;
    }
    if (coset_major) bytes = cosets * n * 16;
    *len = bytes;
    if (!out) return DST_OK;
    if (cap < bytes) { c->err = "output buffer too small"; return DST_ERR_ARG; }
    if (coset_major) {
        fe* tmp = nullptr;
        HIP_TRY(c, hipMalloc((void**)&tmp, bytes));
        k_coset_to_natural_len(c, coset_major, cosets, c->n, tmp);
        hipError_t e = hipMemcpyAsync(out, tmp, bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        hipFree(tmp);
        HIP_TRY(c, e);
    } else {
        HIP_TRY(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return DST_OK;
}

int dst_field_op(dst_ctx* c, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t count) {
    if (!c || !a || !b || !out) return DST_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return k_field_op(c, op, a, b, out, count);
}
int dst_set_profiling(dst_ctx* c, int level) { if (!c || level < 0 || level > 2) return DST_ERR_ARG; c->profile = level; return DST_OK; }
int dst_kernel_stats(dst_ctx* c, char* json_out, size_t cap, int reset) {
    if (!c || !json_out) return DST_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (auto& e : c->kpending) {
        const double ms = event_ms(e.e0, e.e1);
        if (ms >= 0) { auto& st = c->kstats[e.name]; st.launches++; st.ms += ms; st.bytes += e.bytes; st.mads += e.mads; }
        c->event_pool.push_back(e.e0); c->event_pool.push_back(e.e1);
    }
    c->kpending.clear();
    std::string js = "{";
    bool first = true;
    for (auto& kv : c->kstats) {
        char buf[256];
        snprintf(buf, sizeof(buf), "%s\"%s\": {\"launches\": %llu, \"ms\": %.6f, \"bytes\": %.0f, \"mads\": %.0f}", first ? "" : ", ", kv.first.c_str(),
                 (unsigned long long)kv.second.launches, kv.second.ms, kv.second.bytes, kv.second.mads);
        js += buf; first = false;
    }
    js += "}";
    if (reset) c->kstats.clear();
    if (js.size() + 1 > cap) { c->err = "stats buffer too small"; return DST_ERR_ARG; }
    memcpy(json_out, js.c_str(), js.size() + 1);
    return DST_OK;
}

// Calibration kernels (dependent multiplication chains, the multiply-add peak, the straight-line-code probe): laboratory instruments of
// bench.py and the tests, compiled only into the test / bench build (libdistaff_hip_hooks.so).  The product library keeps the entry
// points and answers DST_ERR_STATE.
#if DST_TEST_HOOKS
int dst_bench_mulmod(dst_ctx* c, uint64_t lanes, uint32_t iters, double* ms) {
    if (!c || !ms) return DST_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return k_bench_mulmod(c, lanes, iters, ms);
}
int dst_bench_code(dst_ctx* c, uint32_t code_kib, double* ms) {
    if (!c || !ms) return DST_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return k_bench_code(c, code_kib, ms);
}
int dst_bench_clock(dst_ctx* c, uint64_t lanes, uint32_t iters, double* mhz) {
    if (!c || !mhz) return DST_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return k_bench_clock(c, lanes, iters, mhz);
}
int dst_bench_mad(dst_ctx* c, uint64_t lanes, uint32_t iters, double* ms) {
    if (!c || !ms) return DST_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return k_bench_mad(c, lanes, iters, ms);
}
#else
static int no_hooks(dst_ctx* c) { if (c) c->err = "calibration kernels are part of the test / bench build (libdistaff_hip_hooks.so) only"; return c ? DST_ERR_STATE : DST_ERR_ARG; }
int dst_bench_mulmod(dst_ctx* c, uint64_t, uint32_t, double*) { return no_hooks(c); }
int dst_bench_code(dst_ctx* c, uint32_t, double*) { return no_hooks(c); }
int dst_bench_mad(dst_ctx* c, uint64_t, uint32_t, double*) { return no_hooks(c); }
int dst_bench_clock(dst_ctx* c, uint64_t, uint32_t, double*) { return no_hooks(c); }
#endif
// 1 when this is the test / bench build
int dst_test_hooks(void) { return DST_TEST_HOOKS; }

