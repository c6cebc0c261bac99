// Internal definitions shared by the kernel translation units and the C-ABI layer of libdistaff_hip.so.
//
// HBM layout (all field elements are 16-byte `fe`, digests 32-byte `digest`):
//   trace   [W][n]        register traces as uploaded (column-major, the reference's Vec<Vec<u128>>)
//   polys   [W][n]        the same registers in coefficient form (TraceTable.polys, trace_table.rs:11)
//   lde     [W][Bc][n]    "coset-major" low-degree extension: lde[c][j][k] = T_c(w_N^(B*k + j0 + j)), i.e. the value the
//                         reference keeps at registers[c][B*k + j0 + j].  A coset is a contiguous size-n array, so the
//                         size-n NTT that produces it, the constraint kernel (rows i and i+B are (j,k),(j,k+1)) and the
//                         FRI fold (i, i+N/4, ... share j) all stream with unit stride.
//   Merkle leaves / nodes are kept in the reference's natural leaf order (leaf i = B*k + j), heap-indexed
//   (nodes[1] = root, merkle.rs:269-294); kernels that read coset-major data and emit natural-order digests go
//   through an LDS tile transpose so that both sides are coalesced.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include <string>
#include <map>
#include <vector>
#include "fe.h"
#include "../../include/distaff_hip.h"

struct __attribute__((aligned(16))) digest { uint32_t w[8]; };
#define AIR_PERIODIC_STRIDE 29         // 8 sponge constants, 12 hasher constants, 3 cycle masks, the cubes of hasher constants 0..5

// Four-step twiddles are streamed from HBM once per element of every first pass: as plain elements (16 bytes, general multiplication,
// 71 VALU instructions) or as table pairs (32 bytes, fe_mul_tw, 55).  Measured on the 2^20 proof: first passes 13.1 ms with plain
// elements, 13.4 ms with pairs (the table is re-fetched per register: the four workgroups that share it drift apart by more than the
// 4 MiB L2 of their XCD holds), and half the table memory: plain elements are the default.
#ifndef NTT_TW4_PAIRS
#define NTT_TW4_PAIRS 0
#endif
#if NTT_TW4_PAIRS
typedef fe_tw tw4_t;
#else
typedef fe tw4_t;
#endif

#define DST_MAX_FRI_LAYERS 24

// Every DISTAFF_* variable the library looks at, in one place (INTEGRATION.md section 6 prints this table; a test keeps both in step).
// They are read ONCE per context, when it is created (dst_ctx_create -> dst_ctx::sw), never per call.  `product` switches are operational
// choices every build honours; the others select alternative formulations that exist for the tests to compare with the default ones and are
// honoured only by the test / bench build (libdistaff_hip_hooks.so, -DDISTAFF_TEST_HOOKS): the product library does not even read them.
// (DISTAFF_SHARD_DEBUG is also looked at by dst_comm_init*, which has no context: once, when the communicator is created; DISTAFF_COMM_TIMEOUT_S
// DISTAFF_LOCAL_TRANSPORT and the test build's DISTAFF_TEST_STALL_COLLECTIVE are communicator settings read at the same moment and nowhere else.)
struct dst_switch_def { const char* name; bool product; const char* values; const char* what; };
static const dst_switch_def DST_SWITCHES[] = {
    {"DISTAFF_SHARD_DEBUG",        true,  "1",               "stderr line per tree exchange on rank 0; communicators record the order of their collectives (dst_comm_trace)"},
    {"DISTAFF_SHARD_TREE_GATHER",  true,  "1",               "sharded Merkle trees: all-gather of all boundary nodes + upper levels repeated on every rank (BASELINE north_star's all-gather-only form) instead of the k-range all-to-all"},
    {"DISTAFF_SHARD_NO_OVERLAP",   true,  "1",               "sharded prover: every collective on the context's main stream (no second stream / events) also on a stream-ordered transport"},
    {"DISTAFF_COMM_TIMEOUT_S",     true,  "seconds",         "communicators: limit of every host wait behind a collective (default 60; <= 0: none); on expiry the rank aborts the communicator and returns DST_ERR_COMM (dst_comm_set_timeout changes it per handle)"},
    {"DISTAFF_LOCAL_TRANSPORT",    true,  "blocking",        "in-process transport (dst_comm_init_local, dst_prove_sharded_local): drain every rank's stream around each collective instead of the stream-ordered form (events between the ranks' streams, nothing waited for)"},
    {"DISTAFF_TMP_REGS",           true,  "4..W",            "registers per transform launch = size of the staging array (default: as many as 12 GiB hold, at most W)"},
    {"DISTAFF_AIR",                false, "small|deep|generic", "force a more general constraint-kernel instance set than the trace shape needs (generic = per-operation formulation)"},
    {"DISTAFF_AIR_CHECK",          false, "inline|trace|fri|pow|open", "dst_prove: where the check of the trace rows is queued -- inline: on the main stream behind the evaluation; else on the low-priority side stream, from the end of the trace commitment on (trace), from the first FRI layer on (fri), from the proof of work on (pow), from the openings on (open)"},
    {"DISTAFF_BOUNDARY",           false, "eval",            "boundary combinations by evaluation on the 8n domain (the reference's route) instead of coefficient form"},
    {"DISTAFF_COMBINE",            false, "steps",           "combine_polys / DEEP composition as the reference's sequence of whole-array steps instead of the fused passes"},
    {"DISTAFF_NTT",                false, "pre|pre_a|3pass|reg|lds|row", "force a transform plan family (pre_a: a register pre-stage in the first pass only; row: the default plan with row-major staging array and tables)"},
    {"DISTAFF_NTT_SHAPE",          false, "a,b",             "three-pass plans: log2 of the first two pass lengths"},
    {"DISTAFF_NTT_ORDER",          false, "0",               "first pass of an extension in coset-slow block order"},
    {"DISTAFF_NTT_WAVES",          false, "4|8",             "force the 512- or 1024-lane instances of the LDS passes"},
    {"DISTAFF_NTT_FIXED",          false, "0",               "use the any-shape instances where a shape-compiled one exists"},
    {"DISTAFF_NTT_DIF",            false, "0|1|2",           "first pass of an extension: coset DIT (0), pre-scale + DIF (1), DIT with last-stage twiddles from global memory (2)"},
    {"DISTAFF_NTT_DEBUG",          false, "1",               "print the occupancy of every transform launch shape once"},
    {"DISTAFF_LDE_BATCH",          false, "cols,cosets",     "registers x cosets per transform launch"},
    {"DISTAFF_FOLD8_DFT",          false, "0",               "8n-coefficient extensions without the fused fold + 8-point step"},
    {"DISTAFF_TRACE_BUFFER",       false, "1",               "give the trace its own buffer instead of coset 0 of the extension"},
    {"DISTAFF_MERKLE_LEVEL2_LOG",  false, "k",               "build two tree levels per launch from 2^k grandparents per launch on (default 2^19)"},
    {"DISTAFF_MERKLE_LEVELS",      false, "1",               "one launch per tree level"},
    {"DISTAFF_SYN_DIV_TABLES",     false, "1",               "synthetic division by power tables + scan instead of the blocked form"},
    {"DISTAFF_FRI_TAIL",           false, "0",               "no single-launch tail: every FRI layer by its own launches (the tail otherwise starts at the first layer of at most 2^13 elements)"},
    {"DISTAFF_FRI_CHAIN",          false, "0",               "FRI commit phase with a root read-back and a host draw per layer"},
    {"DISTAFF_FRI_REPLICATE_LOG",  false, "k",               "sharded prover: replicate FRI layers from 2^k elements on (default 2^17)"},
    {"DISTAFF_SHARD_FORCE_OVERLAP", false, "1",              "sharded prover: the two-stream choreography of a stream-ordered transport over a blocking one"},
    {"DISTAFF_TEST_STALL_COLLECTIVE", false, "k|k@r",        "communicators: fault injection -- before device collective number k (of rank r only) a kernel holds the stream until the communicator is aborted"},
};
// Layout of the page-locked staging area dst_ctx::h_stage (HS_TOTAL bytes): every small upload / read-back that must be QUEUED rather than
// waited for has its own region, so that the lifetime of the host side of an asynchronous copy is explicit (a pageable source would be
// staged by the runtime -- which makes the host wait for the stream -- or go out of scope).  Regions are reused per proof: the host
// synchronises the stream at least once between two uses of the same region.
enum : size_t {
    HS_WEIGHTS = 0,                    // boundary weights: 4 W + 4 elements                                   (host/steps_impl.h step::boundary_polys)
    HS_WEIGHTS_BYTES = (4 * 128 + 4) * 16,
    HS_DEEP = 32768,                   // read-back of T(z) at +0 and T(z g) at +HS_DEEP_HALF, W elements each   (api.hip compose_impl)
    HS_DEEP_HALF = 2048,
    HS_FRI_ROOTS = 40960,              // read-back of the FRI roots: 32 bytes per layer                          (host/steps_impl.h step::fri_commit_natural)
    HS_FRI_SLOTS = 45056,              // sharded FRI layers: deferred tree records, HS_FRI_SLOT_BYTES per layer  (shard.hip dst_prove_sharded)
    HS_FRI_SLOT_BYTES = 800,           //   G records of 96 bytes + the 32-byte root, G <= 8
    HS_AIR_FLAG = 65536 - 64,          // read-back of the failing step of the constraint check                   (kernels_air.hip)
    HS_DRAWS = 65536,                  // upload of the 344 constraint coefficients + the compacted transition coefficients (<= 156)   (host/steps_impl.h step::eval_constraints)
    HS_DRAWS_BYTES = (344 + 160) * 16,
    HS_COMPOSE = 65536 + 8192,         // upload of the 516 composition draws
    HS_COMPOSE_BYTES = 516 * 16,
    HS_STATUS = 65536 + 8192 + 8320,   // upload of this rank's status record of a tree exchange: a ring of HS_STATUS_SLOTS records of 64 bytes
    HS_STATUS_SLOTS = 32,
    // read-backs that sit BEHIND collectives of the sharded prover: into page-locked memory, because a device-to-host copy into pageable
    // memory blocks the host inside hipMemcpyAsync -- an unbounded wait in front of the bounded one (comm.h wait_stream)
    HS_TREE_READBACK = 65536 + 8192 + 8320 + 2048,     // tree exchange: G records of 96 bytes + the 32-byte root               (shard.hip tree_exchange)
    HS_TAIL_ROOTS = HS_TREE_READBACK + 1024,           // roots of the FRI layers committed in one launch, 32 bytes per layer     (kernels_poly.hip k_fri_tail)
    HS_POW = HS_TAIL_ROOTS + 1024,                     // the nonce found by the proof-of-work search                            (kernels_poly.hip k_pow)
    HS_TOTAL = 131072
};
static_assert(HS_WEIGHTS + HS_WEIGHTS_BYTES <= HS_DEEP, "boundary weights overlap the DEEP values");
static_assert(HS_DEEP_HALF >= 128 * 16 && HS_DEEP + 2 * HS_DEEP_HALF <= HS_FRI_ROOTS, "DEEP values: W <= 128 registers");
static_assert(HS_FRI_ROOTS + DST_MAX_FRI_LAYERS * 32 <= HS_FRI_SLOTS, "FRI roots overlap the layer slots");
static_assert(8 * 96 + 32 <= HS_FRI_SLOT_BYTES && HS_FRI_SLOTS + DST_MAX_FRI_LAYERS * HS_FRI_SLOT_BYTES <= HS_AIR_FLAG, "FRI layer slots: G <= 8 ranks, DST_MAX_FRI_LAYERS layers");
static_assert(HS_DRAWS + HS_DRAWS_BYTES <= HS_COMPOSE && HS_COMPOSE + HS_COMPOSE_BYTES <= HS_STATUS && HS_STATUS + HS_STATUS_SLOTS * 64 <= HS_TOTAL, "upload regions overlap");
static_assert(HS_STATUS_SLOTS >= 2 + DST_MAX_FRI_LAYERS, "one status slot per tree exchange of a proof");
static_assert(HS_STATUS + HS_STATUS_SLOTS * 64 <= HS_TREE_READBACK && 8 * 96 + 32 <= 1024 && DST_MAX_FRI_LAYERS * 32 <= 1024 && HS_POW + 64 <= HS_TOTAL, "read-back regions overlap");

#ifdef DISTAFF_TEST_HOOKS
#define DST_TEST_HOOKS 1
#else
#define DST_TEST_HOOKS 0
#endif

// ids for dst_read_buffer
enum {
    DST_BUF_POLYS = 0,        // [W][n]
    DST_BUF_LDE = 1,          // arg = register: natural order [N] (converted from coset-major on the device)
    DST_BUF_TRACE_LEAVES = 2, // [N] x 32
    DST_BUF_TRACE_NODES = 3,  // [N] x 32 (heap)
    DST_BUF_CEVAL_I = 4,      // combined boundary (first step) evaluations over the 8n domain, natural order
    DST_BUF_CEVAL_F = 5,
    DST_BUF_CEVAL_T = 6,
    DST_BUF_CPOLY = 7,        // constraint polynomial, 8n coefficients
    DST_BUF_CEVALS = 8,       // constraint polynomial over the LDE domain, natural order [N]
    DST_BUF_CNODES = 9,       // constraint tree nodes [N/2] x 32 (heap)
    DST_BUF_COMP_POLY = 10,   // composition polynomial, 8n coefficients
    DST_BUF_COMP_EVALS = 11,  // composition evaluations, natural order [N]
    DST_BUF_FRI_EVALS = 12,   // arg = layer: evaluations of that layer, natural order
    DST_BUF_FRI_NODES = 13,   // arg = layer: tree nodes (heap)
    DST_BUF_FRI_LEAVES = 14,  // arg = layer: hashed rows
};

// The transform plan of a context (kernels_ntt.hip: ntt_plan_derive, k_ntt_init): n = n1 * n2 in two HBM passes or n = n1 * nm * n3 in three, and
// everything about each pass that is fixed when the context is created.  The launch adds only what depends on (cosets, columns).
struct NttInstance;                                  // row of the table of compiled ntt_pass_a / ntt_pass_b instances
struct NttRegInstance;                               // the same for ntt_reg_kernel<LOGL>
enum NttKind : uint32_t { NTT_FIRST, NTT_MIDDLE, NTT_LAST };
struct NttPass {
    NttKind kind = NTT_FIRST;
    uint32_t log_len = 0;                            // length of the tile transform (half of the pass's with a register pre-stage)
    uint32_t log_tile = 0, pre = 0;                  // log2 of the columns per workgroup tile; register pre-stage 0 / 1 (see NttArgs)
    uint32_t dit = 0;                                // first pass of an extension: 0 pre-scale + DIF, 1 coset DIT, 2 DIT with the last-stage twiddles in global memory
    size_t lds = 0;                                  // dynamic LDS bytes: tile + stage twiddles
    const NttInstance* inst = nullptr;               // LDS family: the instance that runs the pass
    const NttRegInstance* reg = nullptr;             // register-radix family (tile lengths 2^6 .. 2^12) instead
    // views of the context's tables, [0] forward [1] inverse (k_ntt_init): stage twiddles w_len^t, pre-stage twiddles w_{2 len}^m, four-step twiddles
    const fe_tw* stage_tw[2] = {nullptr, nullptr}; const fe_tw* pre_tw[2] = {nullptr, nullptr}; const tw4_t* tw4[2] = {nullptr, nullptr};
};
struct NttPlan {
    uint32_t log_n1 = 0, log_n2 = 0;                 // n = n1 * n2: first pass length, rest
    uint32_t log_n3 = 0;                             // 0: two passes (second pass length n2); else three passes n = n1 * (n2/n3) * n3
    uint32_t count = 0;                              // 2 or 3
    bool coset_slow = false; uint32_t debug = 0;     // DISTAFF_NTT_ORDER=0, DISTAFF_NTT_DEBUG
    bool tile_major = false;                         // layout of the staging array and the four-step tables (kernels_ntt.hip: ntt_tile_major)
    // the interpolation also leaves the trace coefficients in the first pass's tile order (dst_ctx::polys_tm) and the extension reads them
    // there: tile-major plans whose first pass has no register pre-stage (n <= 2^20)
    bool coeff_tile_major = false;
    NttPass pass[3], first_lde;                     // first_lde: pass[0] as the first pass of an extension (its DIT mode, LDS bytes and instance differ)
    const NttPass& at(uint32_t i, bool lde) const { return (i == 0 && lde) ? first_lde : pass[i]; }
};

// Everything a context acquired from the runtime.  Only ctx_dev_bytes, ctx_pinned, ctx_event and ctx_stream (below) add to it, only free_all takes from
// it: the pointer members of dst_ctx that kernels and launchers read are views of these, and an alias (trace == lde, fri_e[0] == comp) is in here once.
struct dst_owned {
    std::vector<void*> dev, pinned;                  // hipMalloc, hipHostMalloc
    std::vector<hipEvent_t> events; std::vector<hipStream_t> streams;      // streams in order of creation: the main stream first
};

struct dst_ctx {
    dst_params prm{};
    std::string err;
    dst_owned own;
    // the DISTAFF_* switches as they were when the context was created (see DST_SWITCHES); sw() returns nullptr for an unset one
    std::map<std::string, std::string> sw_values;
    const char* sw(const char* name) const { auto it = sw_values.find(name); return it == sw_values.end() ? nullptr : it->second.c_str(); }
    bool sw_is(const char* name, const char* value) const { const char* v = sw(name); return v && !strcmp(v, value); }
    bool sw_flag(const char* name) const { const char* v = sw(name); return v && v[0] && v[0] != '0'; }
    void read_switches() {
        sw_values.clear();
        for (const dst_switch_def& d : DST_SWITCHES)
            if (d.product || DST_TEST_HOOKS) if (const char* v = getenv(d.name)) sw_values[d.name] = v;
    }
    int device = 0;
    hipStream_t stream = nullptr;

    // derived sizes
    uint32_t log_n = 0, log_b = 0, log_N = 0;
    size_t n = 0, B = 0, N = 0, W = 0;
    size_t Bc = 0, j0 = 0;              // local cosets
    size_t stack_depth = 0;
    NttPlan plan;
    std::vector<fe> air_draws;         // the 344 constraint coefficients of the current proof: step::eval_constraints keeps them for step::combine (host/steps_impl.h)
    std::shared_ptr<void> open_plan;   // shard.hip: plan of the last dst_shard_open, reused by dst_shard_assemble for the same positions
    std::vector<uint64_t> open_plan_positions;
    uint8_t open_plan_root[32] = {0};   // trace root the cached plan was built for
    int fri_rep_from = 0;               // sharded phases: FRI layers >= this one are replicated (natural order, full heaps on every rank), see shard.hip
    bool fri_tail_pending = false;      // dst_shard_fri_begin exported the evaluations of layer fri_rep_from; dst_shard_fri_end finishes the commit phase
    fe* fri_nat0 = nullptr;             // natural-order layer 0 when fri_rep_from == 0 (fri_e[0] is the rank's coset-major piece)
    bool sharded_layout = false;        // FRI layers >= 1 coset-major with per-rank tree heaps (dst_shard_* phases) instead of natural order / full heaps

    // tables (device)
    fe *tw_lo = nullptr, *tw_hi = nullptr;       // w_N^t, two-level: e = (hi << lo_bits) | lo
    fe *itw_lo = nullptr, *itw_hi = nullptr;     // w_N^-t
    uint32_t tw_lo_bits = 0;
    // every twiddle of the LDS-family transforms is a table pair (w, w * 2^64 mod p), see fe_mul_tw (fe.h)
    fe_tw *ntt_stage_tw[3][2] = {}, *ntt_pre_tw[3][2] = {};   // per pass of the plan, forward and inverse: stage twiddles w_len^t, t < len / 2; register pre-stage w_{2 len}^m, m < len
    fe_tw *prescale = nullptr;                   // w_{B*n1}^t, t < B*n1
    fe_tw *dit_last = nullptr;                   // [B][R][len/2], len = n1 / R, R = 2^pre_a: last-stage twiddles of every coset's (half-length) DIT, w_{B*n1}^(j + B*(h + R*k)) (the pre-scale table regrouped)
    // four-step twiddles of pass A as full tables in output order [k1][m2] (one multiplication per element instead of a two-level
    // lookup + two; the extra 16 B/element read is free: the pass runs at a tenth of the HBM bandwidth)
    tw4_t *tw4_lde = nullptr;                    // [Bc][n]: w_N^(m2 * (B*k1 + j)), local cosets j
    tw4_t *tw4_fwd = nullptr, *tw4_inv = nullptr;   // [n]: w_n^(m2*k1) and its inverse
    tw4_t *tw4_row_fwd = nullptr, *tw4_row_inv = nullptr;   // three-pass plans: [n2] twiddles w_{n2}^(k2*m3) of the middle pass and inverse
    fe *tmp2 = nullptr;                          // three-pass plans: second staging buffer
    fe *periodic = nullptr;                      // [128][AIR_PERIODIC_STRIDE] extended Rescue round constants + cycle masks + cubes of six of them
    void *air_consts = nullptr;                  // AirConsts (Rescue MDS matrices) in device memory
    fe c16f[8], c16i[8];                         // w_16^j and w_16^-j, j < 8 (passed to the NTT kernels by value)
    fe_tw n_inv_tw{};                            // 1/n as a table pair
    fe n_inv{}, eight_inv{}, four_inv{}, iota{}, g_trace{}, x_last{};   // 1/n, 1/8, 1/4, w_N^(N/4), w_n, w_n^(n-1)

    // data (device)
    fe *trace = nullptr, *polys = nullptr, *lde = nullptr, *tmp = nullptr;
    // [W][n] or nullptr (NttPlan::coeff_tile_major): the coefficients of `polys` once more, element (m1, m2) of a register (coefficient
    // m1 * n2 + m2) at ((m2 >> 2) * n1 + m1) * 4 + (m2 & 3) -- a first-pass tile of the extension (four adjacent m2, every m1) is one contiguous
    // block.  Written by k_intt_columns beside `polys`, read by k_lde_columns alone; everything else reads `polys` in natural order.
    fe *polys_tm = nullptr;
    size_t tmp_regs = 4;                // tmp (and tmp2) hold tmp_regs x Bc arrays of n elements
    // register r of the trace starts at trace + r * trace_stride.  A context that owns coset 0 of the extension keeps the trace IN the
    // coset-0 slots of `lde` (trace == lde, trace_stride == Bc * n): coset 0 of the extension is the trace itself, nothing is copied
    size_t trace_stride = 0;
    digest *trace_leaves = nullptr, *trace_nodes = nullptr;
    fe *ceval = nullptr;                // [3][8c][n] combined constraint evaluations (i, f, t), coset-major over the 8n domain
    fe *cwork = nullptr;                // scratch, 3 * 8n
    fe *cpoly = nullptr;                // [8n]
    fe *cevals = nullptr;               // [Bc][n]
    digest *cnodes = nullptr;           // [N/2]
    fe *comp_poly = nullptr;            // [8n]
    fe *comp = nullptr;                 // [Bc][n]
    fe *scratch = nullptr;              // misc scan / reduction scratch; its last 1024 elements: the small vectors of the phase in flight (host/steps.h ScratchTail)
    size_t scratch_elems = 0;
    int num_fri_layers = 0, fri_committed = 0, fri_folded = 0;
    fe *fri_e[DST_MAX_FRI_LAYERS] = {nullptr};       // evaluations of layer d (d = 0 aliases comp, coset-major)
    digest *fri_leaves[DST_MAX_FRI_LAYERS] = {nullptr};
    digest *fri_nodes[DST_MAX_FRI_LAYERS] = {nullptr};
    size_t fri_size[DST_MAX_FRI_LAYERS] = {0};       // N_d
    // coset-sharded mode (world > 1): replicated upper parts of the trees and the gather landing buffer
    digest *trace_upper = nullptr, *c_upper = nullptr, *fri_upper[DST_MAX_FRI_LAYERS] = {nullptr};
    uint8_t *gather_buf = nullptr; size_t gather_bytes = 0;
    // dst_prove_sharded: trees whose upper part is partitioned by k-ranges (rank g finishes the subtree over k in [g*K/G, (g+1)*K/G) from
    // an all-to-all of boundary nodes; `*_upper` then holds the replicated top heap [0, 2G) and this rank's subtree heap behind it)
    // instead of being rebuilt from an all-gather on every rank (the host-orchestrated dst_shard_import).  Index 0 trace, 1 constraint, 2 + d FRI layer d.
    bool tree_krange[2 + DST_MAX_FRI_LAYERS] = {false};
    uint64_t *d_u64 = nullptr;                        // small device scalars (pow result, AIR failure flag)
    uint8_t *d_fri_chain = nullptr;                   // dst_prove's FRI commit phase without host round trips: [24] roots (32 B) then [24] draws (16 B)
    uint8_t *h_stage = nullptr;                       // page-locked host staging (HS_TOTAL bytes, layout HS_* above): small uploads / read-backs that must not make the host wait
    unsigned long long air_flag_host = ~0ull;         // read-back of the AIR failure flag (deferred check)
    // The check of the trace rows (air_kernel.h air_check_kernel) beside the proof's later phases: dst_prove queues it on a stream of the
    // lowest priority behind an event of the main stream; the partial stack values of the chain have arrays of their own (nothing else
    // writes them).  While check_pending, the side stream may still READ the trace (coset 0 of `lde`): whoever writes or frees that buffer
    // drains it first (k_air_check_drain).
    hipStream_t check_stream = nullptr;
    hipEvent_t check_ev = nullptr;
    fe *check_partials = nullptr;                     // [k_air_check_partials][n]: 6 arrays for the depth-4 set (96 MiB at n = 2^20), 10 otherwise
    bool check_pending = false;
    hipEvent_t ph_ev[6] = {nullptr};                  // phase boundaries on the stream (phase times without host waits)
    uint8_t *d_stage = nullptr;                       // staging buffer for gathers
    size_t stage_bytes = 0;

    // host copies kept for proof assembly
    dst_public pub{};
    uint8_t trace_root[32] = {0}, constraint_root[32] = {0};
    std::vector<uint8_t> deep_z1, deep_z2;
    bool deep_pending = false;          // the DEEP values of the last composition are still in the page-locked staging area
    std::vector<std::vector<uint8_t>> fri_roots;
    uint64_t op_count = 0;              // op counter of the last trace row as the proof header carries it
    fe op_counter{};                    // the same register as the field element it is (an arbitrary table may hold any value below p): what the last-step boundary constraint subtracts
    fe program_hash[2] = {};
    bool have_trace = false, committed = false, constraints_done = false, composed = false;
    // asynchronous upload (dst_trace_upload_async): column group g is complete when upload_done[g] has fired on upload_stream
    hipStream_t upload_stream = nullptr;
    std::vector<hipEvent_t> upload_done;
    std::vector<size_t> upload_bounds;  // group g holds registers [upload_bounds[g], upload_bounds[g + 1])
    bool upload_pending = false;
    // dst_trace_upload_owned: only the registers r = rank (mod world) of the trace are on this device (the sharded prover interpolates
    // exactly those and all-gathers the coefficient vectors)
    bool trace_owned_only = false;
    // dst_prove_sharded: the gathered transition evaluations in `ceval` are already inverse-transformed per coset (every rank did its own
    // cosets before the exchange); dst_shard_combine then only runs the 8-point step across cosets
    bool ceval_inverted = false;
    // dst_prove_sharded: collectives that overlap with compute run on their own stream, ordered by events; status records of all ranks
    hipStream_t comm_stream = nullptr;
    std::vector<hipEvent_t> comm_events;
    uint8_t* d_status = nullptr;
    double phase_ms[9] = {0};
    double shard_ms[2] = {0, 0};           // dst_prove_sharded: host milliseconds inside the transport's calls / waiting for tree roots
    uint32_t shard_trees = 0;              // tree exchanges of the last sharded proof
    // dst_prove_sharded: the communicator whose collectives may sit on this context's streams.  While it is set, every host wait of the
    // prover is the communicator's bounded poll (ctx_sync below, comm.h) instead of hipStreamSynchronize
    struct dst_comm* wait_comm = nullptr;
    hipEvent_t sh_ev[8] = {nullptr};       // phase boundaries of dst_prove_sharded on the stream (created on first use)
    struct CollEv { hipEvent_t e0, e1; int kind; };
    std::vector<CollEv> coll_ev;           // events around the collectives of the last sharded proof (the first coll_used of them)
    size_t coll_used = 0;
    double exchange_ms[8] = {0};           // dst_shard_exchange_ms

    // optional per-kernel timing with HIP events recorded on `stream` (dst_set_profiling / dst_kernel_stats)
    int profile = 0;                       // dst_set_profiling: 0 off, 1 every kernel launch, 2 only the heavy kernels (NTT passes, constraint kernel, leaf hashing)
    struct KEvent { hipEvent_t e0, e1; std::string name; double bytes, mads; };
    std::vector<KEvent> kpending;
    std::vector<hipEvent_t> event_pool;    // recycled profiling events
    struct KStat { uint64_t launches = 0; double ms = 0, bytes = 0, mads = 0; };
    std::map<std::string, KStat> kstats;
};

#define HIP_TRY(ctx, expr)                                                                          \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                          \
            return DST_ERR_HIP;                                                                     \
        }                                                                                           \
    } while (0)

// ---- the only places that acquire a runtime resource for a context, and the one that releases them.  Each helper fails the way HIP_TRY
//      does (c->err, DST_ERR_HIP) and leaves its target null then; what it made is the context's until free_all ---------------------------
inline int ctx_dev_bytes(dst_ctx* c, void** p, size_t bytes) {
    void* q = *p = nullptr;
    HIP_TRY(c, hipMalloc(&q, bytes));
    c->own.dev.push_back(*p = q);
    return DST_OK;
}
template <class T> static int dev_alloc(dst_ctx* c, T** p, size_t count) { return ctx_dev_bytes(c, (void**)p, count * sizeof(T) > 0 ? count * sizeof(T) : 16); }
template <class T> static int dev_upload(dst_ctx* c, T** p, const std::vector<T>& v) {
    if (const int r = dev_alloc(c, p, v.size())) return r;
    HIP_TRY(c, hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return DST_OK;
}
inline int ctx_pinned(dst_ctx* c, uint8_t** p, size_t bytes) {              // a page-locked host block
    void* q = *p = nullptr;
    HIP_TRY(c, hipHostMalloc(&q, bytes, hipHostMallocDefault));
    c->own.pinned.push_back(q); *p = (uint8_t*)q;
    return DST_OK;
}
inline int ctx_event(dst_ctx* c, hipEvent_t* e, unsigned flags = 0) {
    hipEvent_t q = *e = nullptr;
    HIP_TRY(c, hipEventCreateWithFlags(&q, flags));
    c->own.events.push_back(*e = q);
    return DST_OK;
}
// lowest: at the lowest priority the device has (the host build of the tests: launches are synchronous there, its runtime has no priorities)
inline int ctx_stream(dst_ctx* c, hipStream_t* s, unsigned flags = 0, bool lowest = false) {
    hipStream_t q = *s = nullptr;
#ifndef DISTAFF_EMULATED
    int least = 0, greatest = 0;
    if (lowest) { HIP_TRY(c, hipDeviceGetStreamPriorityRange(&least, &greatest)); HIP_TRY(c, hipStreamCreateWithPriority(&q, flags, least)); } else
#endif
    HIP_TRY(c, hipStreamCreateWithFlags(&q, flags));
    c->own.streams.push_back(*s = q);
    return DST_OK;
}
inline void free_all(dst_ctx* c) {            // allocations and events before the streams, the main stream last
    for (void* p : c->own.dev) (void)hipFree(p);
    for (void* p : c->own.pinned) (void)hipHostFree(p);
    for (hipEvent_t e : c->own.events) (void)hipEventDestroy(e);
    for (auto s = c->own.streams.rbegin(); s != c->own.streams.rend(); ++s) (void)hipStreamDestroy(*s);
    c->own = dst_owned{};
}
// A timing event from the pool of recycled profiling events (dst_kernel_stats refills it), made when the pool is empty: creating two per
// launch would be host time inside a timed region.  TimerPair: two of them for one function's own measurement, back in the pool on every way out.
inline int ctx_timer_event(dst_ctx* c, hipEvent_t* e) {
    if (c->event_pool.empty()) return ctx_event(c, e);
    *e = c->event_pool.back(); c->event_pool.pop_back();
    return DST_OK;
}
struct TimerPair {
    dst_ctx* c; hipEvent_t e0 = nullptr, e1 = nullptr; int rc;
    explicit TimerPair(dst_ctx* ctx) : c(ctx) { rc = ctx_timer_event(c, &e0); if (!rc) rc = ctx_timer_event(c, &e1); }
    ~TimerPair() { for (hipEvent_t e : {e0, e1}) if (e) c->event_pool.push_back(e); }
};

// brackets one kernel launch with events when profiling is on; `bytes` = algorithmic HBM bytes of that launch, `mads` = 32x32+64
// multiply-adds (v_mad_u64_u32) the launch executes per the kernel's arithmetic (0 where not counted)
struct KScope {
    dst_ctx* c; bool on;
    hipStream_t s;                         // the stream the launch goes to: the context's, unless the caller names another (the check chain's)
    dst_ctx::KEvent ev;
    KScope(dst_ctx* ctx, const char* name, double bytes, bool heavy = false, double mads = 0.0, hipStream_t stream = nullptr)
        : c(ctx), on(ctx->profile == 1 || (ctx->profile == 2 && heavy)), s(stream ? stream : ctx->stream) {
        if (!on) return;
        ev.name = name; ev.bytes = bytes; ev.mads = mads;
        if (ctx_timer_event(c, &ev.e0) || ctx_timer_event(c, &ev.e1)) { on = false; return; }     // (a lone first event stays the context's: released with it)
        (void)hipEventRecord(ev.e0, s);
    }
    ~KScope() { if (on) { (void)hipEventRecord(ev.e1, s); c->kpending.push_back(ev); } }
};

// host wait for the context's stream: bounded while a communicator is attached (comm.hip), hipStreamSynchronize otherwise
int ctx_sync(dst_ctx* c, const char* what);
#define CTX_SYNC(ctx, what) do { const int _r = ctx_sync((ctx), (what)); if (_r) return _r; } while (0)

// ---- which formulation of a step a context runs: asked by the constraint launchers (kernels_air*.hip) and by the steps themselves
//      (host/steps.h, host/steps_impl.h) ----------------------------------------------------------------------------------------------
// DISTAFF_BOUNDARY=eval (test build only): the boundary combinations by evaluation on the 8n domain, the reference's route
inline bool dst_internal_boundary_by_evaluation(const dst_ctx* c) { return DST_TEST_HOOKS && c->sw_is("DISTAFF_BOUNDARY", "eval"); }
// DISTAFF_COMBINE=steps (test build only): combine_polys and the DEEP composition as the reference's sequence of whole-array steps
// (boundary polynomials of 8n coefficients, their divisions, additions; copy / division / multiply-adds of the composition) instead of
// the fused passes.  Tests run both; the boundary-by-evaluation route implies it.
inline bool dst_internal_combine_by_steps(const dst_ctx* c) { return DST_TEST_HOOKS && (c->sw_is("DISTAFF_COMBINE", "steps") || dst_internal_boundary_by_evaluation(c)); }
// Step 7: does the single-launch tail (k_fri_tail: rows hashed, trees built, x drawn from every root and the folds done by one workgroup)
// start at layer d?  From the first layer after layer 0 of at most 2^13 evaluations on; DISTAFF_FRI_TAIL=0 (test build only): never.
inline bool fri_tail_starts_at(const dst_ctx* c, int d) {
    if (d < 1 || d >= c->num_fri_layers || c->fri_size[d] > ((size_t)1 << 13)) return false;
    const char* e = c->sw("DISTAFF_FRI_TAIL");
    return !(e && e[0] == '0');
}
// ---- kernel launchers (kernels_*.hip) ------------------------------------------------------------------------------------
// NTT / LDE
int k_ntt_init(dst_ctx* c);                                                             // context creation: derives c->plan, builds every table of it, raises the LDS limits
// size-n inverse NTT of ncols columns src_stride apart -> contiguous columns; dst_tm (a view of c->polys_tm at the same registers, or nullptr):
// the same coefficients once more in the extension's tile order
void k_intt_columns(dst_ctx* c, const fe* src, size_t src_stride, fe* dst, size_t ncols, fe* dst_tm = nullptr);
// n coefficients -> coset-major [Bc][n] per column; polys_tm: what k_intt_columns wrote beside THESE columns -- the first pass reads it instead.
// A caller whose coefficients came another way (all-gathered pieces) hands none and the first pass reads `polys` row-major.
void k_lde_columns(dst_ctx* c, const fe* polys, fe* lde, size_t ncols, const fe* polys_tm = nullptr);
// the registers from `first` on of c->polys_tm, or nullptr where the plan keeps no such copy
static inline fe* polys_tm_at(dst_ctx* c, size_t first) { return c->polys_tm ? c->polys_tm + first * c->n : nullptr; }
void k_lde_fold8(dst_ctx* c, const fe* poly8n, fe* out);                                // 8n coefficients -> coset-major [Bc][n]
void k_intt8_cosets(dst_ctx* c, fe* vals /* [8][n] coset-major, in place scratch */, fe* out8n, fe* work);
void k_coset_to_natural_len(dst_ctx* c, const fe* src, size_t cosets, size_t len, fe* dst);   // [cosets][len] -> natural [len*cosets]
void k_fri_leaves_at(dst_ctx* c, const fe* e, digest* leaves, size_t R);
void k_fri_fold_at(dst_ctx* c, const fe* e, fe* out, size_t R, int layer, fe special_x, const fe* alpha_dev = nullptr);   // alpha_dev: x read from device memory instead
// hashing
void k_trace_leaves(dst_ctx* c);
// the levels of a BLAKE3 tree above `count` children -- `leaves`, or with leaves = nullptr the filled level nodes[count .. 2*count) -- down to the
// level of stop_count nodes; stop_count = 0: down to the root nodes[1] (host/merkle_plan.h chooses the kernels)
void k_merkle(dst_ctx* c, const digest* leaves, digest* nodes, size_t count, size_t stop_count);
void k_constraint_tree(dst_ctx* c);                                                     // k_constraint_level1 and the levels above it, down to the root
void k_fri_leaves_layer0(dst_ctx* c);
void k_fri_leaves(dst_ctx* c, int layer);
// AIR
// defer_check: no host wait; k_constraint_check reads the flag later.  check_here = false: the evaluation alone -- the caller queues the check of
// the trace rows, which is where the verdict comes from, itself (k_air_check_side)
int k_eval_constraints(dst_ctx* c, const fe* coeffs_dev, const fe* tc_dev, int64_t* bad_step, bool defer_check = false, bool check_here = true);
int k_air_check(dst_ctx* c, hipStream_t stream);                                       // queues the check chain and the read-back of its verdict on `stream` (the context's, or k_air_check_side's)
int k_air_check_side(dst_ctx* c);                                                      // the same on the side stream, behind everything queued on the main stream so far
size_t k_air_check_partials(const dst_ctx* c);                                         // arrays of n elements the chain of this context's instance set needs for its partial stack values
int k_air_check_drain(dst_ctx* c);                                                     // host wait for a check chain on the side stream, if one is pending
int k_constraint_check(dst_ctx* c, int64_t* bad_step);                                  // after a stream synchronisation: the failing step recorded by the last evaluation, if any
// polynomial helpers
void k_syn_div(dst_ctx* c, fe* a, size_t len, fe b);                                    // polynom.rs:190 semantics, in place
void k_syn_div_batch(dst_ctx* c, fe* const* a, const fe* b, int count, size_t len);                 // a[k] <- a[k] / (x - b[k]) in place, count <= 4 arrays of `len` coefficients, one set of launches
void k_syn_div_compose(dst_ctx* c, const fe* a, fe* out, size_t len, fe b, const fe* t, size_t tn, size_t inc, fe k1, fe k2, fe k3);   // out = k3 * a / (x - b) + (k1 + k2 x^inc) * t
void k_combine_fused(dst_ctx* c, const fe* work, const fe* q4, size_t q_stride, fe* cpoly);   // kernels_ntt.hip: 8-point step + division + boundary quotients -> constraint polynomial
void k_syn_div_expanded(dst_ctx* c, const fe* a, fe* out, size_t len, size_t degree, fe exception);
void k_horner(dst_ctx* c, const fe* polys, size_t ncols, size_t len, fe x, fe* out_dev);
void k_lincomb2(dst_ctx* c, const fe* cols, size_t ncols, size_t len, const fe* coeffs_dev, size_t coef_stride, fe* out0, fe* out1);
void k_lincomb4(dst_ctx* c, const fe* cols, size_t ncols, size_t len, const fe* coeffs_dev, fe* out0, fe* out1, fe* out2, fe* out3);   // four combinations, one pass over the columns
void k_axpy(dst_ctx* c, fe* y, const fe* x, fe a, size_t len);                           // y += a * x
void k_add(dst_ctx* c, fe* y, const fe* x, size_t len);                                  // y += x
void k_sub_dot_at0(dst_ctx* c, fe* y, const fe* values_dev, const fe* coeffs_dev, size_t count);   // y[0] -= sum values[k]*coeffs[k]
void k_sub_at0(dst_ctx* c, fe* y, const fe* v_dev);                                                   // y[0] -= v[0]
// FRI
void k_fri_fold(dst_ctx* c, int layer, fe special_x);
void k_fri_fold_dev(dst_ctx* c, int layer, const fe* alpha_dev);                        // the same with x read from device memory
void k_fri_draw(dst_ctx* c, int layer, fe* alpha_out, digest* root_out);                // x = prng(root of `layer`) on the device; files the root
void k_intt_cosets_local(dst_ctx* c, fe* vals, fe* out, size_t cosets);
void k_cross8(dst_ctx* c, const fe* work, fe* out8n);
int k_fri_tail(dst_ctx* c, int first, uint8_t* roots_out);       // natural-order layers first .. last in one launch (kernels_poly.hip)
// PoW
int k_pow(dst_ctx* c, const uint8_t seed[32], uint32_t grinding, uint64_t* nonce);
// gathers for openings
void k_gather(dst_ctx* c, const void* src, size_t item_bytes, const uint64_t* idx_dev, size_t count, void* dst);
void k_gather_rows(dst_ctx* c, const uint64_t* positions_dev, size_t count, fe* out);
void k_gather_pieces(dst_ctx* c, const uint64_t* addr_dev, size_t count, void* dst);          // dst[t] = the 16 bytes at device address addr[t]
int k_bench_mulmod(dst_ctx* c, uint64_t lanes, uint32_t iters, double* ms);
int k_bench_mad(dst_ctx* c, uint64_t lanes, uint32_t iters, double* ms);
int k_bench_clock(dst_ctx* c, uint64_t lanes, uint32_t iters, double* mhz);          // shader clock (MHz) sustained under four fe_mul chains per lane on `lanes` lanes
int k_bench_code(dst_ctx* c, uint32_t code_kib, double* ms);      // kernels_probe.hip
// coset-sharded (multi-GPU) helpers
void k_upper_tree(dst_ctx* c, const digest* gathered, digest* upper, size_t nb, uint32_t G);      // the ranks' boundary nodes interleaved into upper[nb G ..), then the tree above them
void k_digests_from_records(dst_ctx* c, const void* recs, size_t stride, digest* dst, size_t count);   // dst[i] = first 32 bytes of record i (count <= 8)
void k_constraint_level1(dst_ctx* c);                                                    // first node level of the constraint tree over this context's cosets
void k_fri_leaves_cm(dst_ctx* c, const fe* e, digest* leaves, size_t nd);
void k_fri_fold_cm(dst_ctx* c, const fe* e, fe* out, size_t nd, int layer, fe special_x, const fe* alpha_dev = nullptr);
void k_fri_draw_at(dst_ctx* c, const digest* nodes, fe* alpha_out, digest* root_out);    // x = prng(nodes[1]) on the device
void k_copy(dst_ctx* c, void* dst, const void* src, size_t bytes);
int k_field_op(dst_ctx* c, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t count);
// Rescue digests / trees (kernels_hash.hip, rescue_dev.h): no context, the caller's stream; -1 when a launch fails; *bad = 1 for an input element >= p
int k_rescue_digests(hipStream_t stream, const fe* in /* 4 per digest */, fe* out /* 2 per digest */, size_t count, uint32_t* bad);
int k_rescue_tree(hipStream_t stream, fe* nodes /* 2 elements per node, leaf level in place */, size_t leaves, uint32_t* bad);
// dirty parents only: level l (2^l parents) recomputes the cnt[l] node positions at lists[off[l] ..); cnt[l] == 2^l: the whole level, no list
int k_rescue_tree_update(hipStream_t stream, fe* nodes, uint32_t log_leaves, const uint32_t* lists /* device */, const size_t* off, const size_t* cnt);
int k_rescue_tree_scatter(hipStream_t stream, fe* nodes, const uint32_t* pos /* device */, const fe* vals /* 2 per node */, size_t count);   // nodes[pos[i]] = vals[i]
int k_rescue_tree_gather(hipStream_t stream, const fe* nodes, const uint32_t* pos /* device */, fe* out /* 2 per node */, size_t count);       // out[i] = nodes[pos[i]]
// sparse trees (host/stree_levels.h): all levels in one node array and one prefix array (device), indexed by flat positions.  One level: the `count`
// parents at list[..] (device; nullptr: pstart + [0, count)) from the child level [cstart, cstart + ccnt); empty = the value of an empty child (host)
// Every launcher that reads prefixes or indices has a second form over stree_wide, the 16-byte keys of the wide trees (dst_wtree_*, dst_rescue_*_w):
// the same kernel body instantiated over the key type
struct stree_wide;
int k_rescue_stree_level(hipStream_t stream, fe* nodes, const stree_wide* pref, const uint32_t* list, size_t count, size_t pstart, size_t cstart, size_t ccnt, const fe* empty);
int k_rescue_stree_open(hipStream_t stream, const fe* nodes, const stree_wide* pref, const uint64_t* levels, const fe* empties, const stree_wide* indices, fe* out, size_t count, uint32_t depth);
int k_rescue_stree_lookup(hipStream_t stream, const fe* nodes, const stree_wide* pref, const uint64_t* levels, const fe* empties, const stree_wide* prefix, const uint32_t* level, fe* out, size_t count);
int k_rescue_stree_get(hipStream_t stream, const fe* nodes, const stree_wide* pref, size_t lstart, size_t lcnt, const fe* empty, const stree_wide* indices, fe* out, uint8_t* stored, size_t count);
int k_rescue_stree_level(hipStream_t stream, fe* nodes, const uint64_t* pref, const uint32_t* list, size_t count, size_t pstart, size_t cstart, size_t ccnt, const fe* empty);
int k_rescue_stree_carry(hipStream_t stream, fe* dst, const fe* src, const uint32_t* from /* device */, size_t count);     // dst[j] = src[from[j]] unless from[j] == STREE_NEW
// out[(i * (depth + 1) + k) ..] = node k of the path of indices[i], stored or empty; levels = (start, length) per level, empties = 2 elements per level (device)
int k_rescue_stree_open(hipStream_t stream, const fe* nodes, const uint64_t* pref, const uint64_t* levels, const fe* empties, const uint64_t* indices, fe* out, size_t count, uint32_t depth);
// out[2 s ..] = the node (level[s], prefix[s]), stored or the empty subtree of its level (all device): the nodes of a multiproof
int k_rescue_stree_lookup(hipStream_t stream, const fe* nodes, const uint64_t* pref, const uint64_t* levels, const fe* empties, const uint64_t* prefix, const uint32_t* level, fe* out, size_t count);
// out[2 i ..] = the leaf at indices[i] and stored[i] = 1, or the empty leaf and 0: one search of the leaf level [lstart, lstart + lcnt); empty on the host
int k_rescue_stree_get(hipStream_t stream, const fe* nodes, const uint64_t* pref, size_t lstart, size_t lcnt, const fe* empty, const uint64_t* indices, fe* out, uint8_t* stored, size_t count);
// the compact multiproof of a wide tree: flat[s] = the flat position of the node (level[s], prefix[s]) or STREE_NEW when it is not stored, rank[s] = the
// stored nodes of its block of 256 before it, totals[b] = those of block b; then out = the stored nodes alone, packed in the order of s (all device)
#define RESCUE_LOCATE_BLOCK 256u
int k_rescue_stree_locate(hipStream_t stream, const stree_wide* pref, const uint64_t* levels, const stree_wide* prefix, const uint32_t* level, uint32_t* flat, uint32_t* rank, uint32_t* totals,
                          size_t count);
int k_rescue_stree_pack(hipStream_t stream, const fe* nodes, const uint32_t* flat, const uint32_t* rank, const uint32_t* totals, fe* out, size_t count);
// flags[i] = whether leaves[i] (2 elements) is the empty leaf (host)
int k_rescue_stree_empty_leaves(hipStream_t stream, const fe* leaves, const fe* empty, uint8_t* flags, size_t count);
// ordered writes (host/tree_sequence.h): the versions vin of one level -> vout, those of the level above, for `count` operations; src / own = this
// level's source words, idx = the operations' indices, paths = count paths of n nodes or nullptr (all device); k = the path node the siblings
// are; nodes = the tree before the call; empty = the value of an empty child (host)
int k_rescue_seq_level(hipStream_t stream, const fe* nodes, const fe* vin, fe* vout, const uint32_t* src, const uint32_t* own, const uint64_t* idx, fe* paths, size_t count, uint32_t k, uint32_t n,
                       const fe* empty);
int k_rescue_tree_scatter_from(hipStream_t stream, fe* nodes, const uint32_t* pos, const fe* vals, const uint32_t* from /* device */, size_t count);      // nodes[pos[i]] = vals[from[i]]
// compute_merkle_root (src/examples/merkle.rs:112-145) of `count` paths of n nodes (all device): ONE launch for every level of every chain.  mode:
// the paths with their own leaves, with alt_leaves[i] as the first node instead, or both -- 2 count chains over one copy of the paths, out[0 .. count)
// the own-leaf roots and out[count .. 2 count) the substitute-leaf roots
enum { RESCUE_PATH_OWN = 0, RESCUE_PATH_ALT = 1, RESCUE_PATH_BOTH = 2 };
int k_rescue_path_roots(hipStream_t stream, const fe* paths, uint32_t n, const uint64_t* indices, size_t count, const fe* alt_leaves, uint32_t mode, fe* out /* 2 per chain */, uint32_t* bad);
// multiproofs (host/multiproof_plan.h): one level of `count` jobs over the pool, pool[out] = digest(pool[left], pool[right]) with the three pool
// indices of job j at jobs[3 j ..) (device); *bad = 1 for an element >= p in a pool node below `inputs` (the leaves and the supplied nodes)
int k_rescue_multiproof_level(hipStream_t stream, fe* pool, const uint32_t* jobs, size_t count, uint32_t inputs, uint32_t* bad);
// audits: ONE launch over every parent of every level; *first_bad (device, set to all ones by the caller) receives by atomicMin the first parent
// that is not the digest of its children -- dense: its heap position in [1, leaves); sparse: (level << 32) | index within the level, for the
// `count` >= 1 parents at the flat positions first + [0, count) = every level above the leaf level; levels / empties as k_rescue_stree_open
int k_rescue_tree_audit(hipStream_t stream, const fe* nodes, size_t leaves, unsigned long long* first_bad);
int k_rescue_stree_audit(hipStream_t stream, const fe* nodes, const uint64_t* pref, const uint64_t* levels, const fe* empties, uint32_t depth, size_t first, size_t count,
                         unsigned long long* first_bad);
int k_rescue_path_roots(hipStream_t stream, const fe* paths, uint32_t n, const stree_wide* indices, size_t count, const fe* alt_leaves, uint32_t mode, fe* out /* 2 per chain */, uint32_t* bad);
// following writes (host/path_refresh.h): the 2 count chains of RESCUE_PATH_BOTH in ONE launch, the substitute-leaf chains also storing their node after
// every level k = 1 .. n - 2: out = the 2 count roots, then mid[k - 1][i], n - 2 levels of count nodes.  Then the refreshed paths in one launch: out[j][k] =
// sel[j][k] < 0 ? held[j][k] : the node of write sel[j][k] for position k (its leaf for k <= 1, mid[k - 2][sel] above).  All device
int k_rescue_path_chains(hipStream_t stream, const fe* paths, uint32_t n, const uint64_t* indices, size_t count, const fe* leaves, fe* out /* 2 count roots | (n - 2) count nodes */, uint32_t* bad);
int k_rescue_path_chains(hipStream_t stream, const fe* paths, uint32_t n, const stree_wide* indices, size_t count, const fe* leaves, fe* out, uint32_t* bad);
int k_rescue_path_refresh(hipStream_t stream, const fe* held, const int32_t* sel, const fe* leaves, const fe* mid, size_t count, uint32_t n, size_t held_paths, fe* out, uint32_t* bad);
int k_rescue_stree_audit(hipStream_t stream, const fe* nodes, const stree_wide* pref, const uint64_t* levels, const fe* empties, uint32_t depth, size_t first, size_t count,
                         unsigned long long* first_bad);
