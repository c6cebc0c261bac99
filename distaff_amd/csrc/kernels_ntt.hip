// NTT / low-degree-extension kernels for gfx950.
//
// Replaces the recursive radix-2 `fft_in_place` (+ `permute`) of /root/reference/src/math/fft.rs:16-108 as it is used by
// TraceTable::extend (src/stark/trace/trace_table.rs:143-169), ConstraintTable::combine_polys (constraint_table.rs:54-88),
// ConstraintPoly::eval (constraint_poly.rs:28-37) and the composition evaluation (prover.rs:98-101).  Field results are
// unique, so the algorithm is free: every transform here is a "four-step" NTT in HBM passes over LDS tiles,
//   two passes (n = n1*n2, n < 2^21):
//     pass A: for a tile of T adjacent columns m2, the n1-point NTT over the stride-n2 dimension, in LDS, with the four-step
//             twiddle w_N^(m2*(B*k1+j)) on store (streamed from a table).  For an extension the transform is a coset DIT whose
//             stage twiddles carry the coset pre-scale w_N^(j*n2*m1); otherwise a DIF; two radix-2 stages per LDS round trip;
//     pass B: for a tile of T adjacent rows k1, the n2-point NTT over the contiguous dimension, in LDS, stored as
//             X[k1 + n1*k2] so that the output is in natural order;
//   three passes (n = n1*nm*n3, n >= 2^21): pass A, pass A again on every row of n/n1 points, pass B with tiles of adjacent k1.
// Workgroups are persistent over adjacent tiles; the 512-lane instances prefetch the next tile into registers while the current one
// is in LDS, the 1024-lane instances of 1024-point tiles (8 waves per SIMD) leave the overlap to the CU's other workgroup.
// The low-degree extension never materialises the zero-padded size-N input of the reference: the N = B*n evaluations
// are B coset transforms of size n (coset j holds the reference's indices B*k + j), stored coset-major; coset 0 of the trace
// extension is the trace itself and is copied.  The staging array between the passes and the four-step table are private to the
// transforms: two-pass plans up to n = 2^21 whose tiles are four columns wide in both passes keep them TILE-MAJOR (NttArgs::tile_major)
// -- a first-pass tile stores one contiguous block of 16 * n1 * 4 bytes and reads its twiddles from one, a second-pass tile reads
// 256-byte runs; every other plan keeps them row-major in T*16-byte segments (T = 16 for the 256-point tiles of three-pass plans).
// A second, register-radix kernel family (ntt_reg_kernel) is kept as an independent
// implementation that the tests run at every tile length.
// The host side is in this file too ("launch layer" below): the table of compiled instances, the plan of a context (ntt_plan_derive: passes, tile
// shapes, kernel family and instance per pass), its tables (k_ntt_init, called by dst_ctx_create) and ONE function that launches a pass (ntt_run_pass).
#include "ctx.h"
#include "host/ctx_tables.h"     // k_ntt_init builds the tables of the plan
#include <mutex>
#include <type_traits>
#include "ntt_lds.h"

#if defined(NTT_NO_ROTATE)
#define NTT_NO_ROTATE_DEFINED 1
#else
#define NTT_NO_ROTATE_DEFINED 0
#endif
#define NTT_TILE_ELEMS 4096      // elements of an LDS tile (64 KiB); a workgroup of 512 lanes holds 8 per lane, one of 1024 lanes 4

struct NttArgs {
    const fe* src; fe* dst;
    size_t src_col_stride, src_coset_stride;   // elements
    size_t dst_col_stride, dst_coset_stride;
    const fe_tw* stage_tw;     // w_len^t, t < len/2 (forward or inverse), as table pairs
    const fe_tw* prescale;     // w_{B*n1}^t or nullptr
    const fe_tw* dit_last;     // coset DIT whose last-stage twiddles stay in global memory: [B][n1/2] pairs w_{B*n1}^(j + B*k), else nullptr
    const tw4_t* tw4;          // four-step twiddles in the order of the first pass's output (coset stride tw4_coset_stride)
    size_t tw4_coset_stride;
    // Layout of the array between the two passes and of the four-step table.  0: row-major, element (k1, m2) at (k1 << log_n2) + m2.
    // 1 (ntt_tile_major: two-pass plans with four-column tiles in both passes): tile-major, [m2 >> 2][k1][m2 & 3] -- element (k1, m2) at
    // (((m2 >> 2) << log2(number of k1)) + k1) * 4 + (m2 & 3).  The block of a first-pass tile (four adjacent m2, every k1) is contiguous and
    // in the order the tile leaves LDS; a second-pass tile (four adjacent k1, every m2) reads runs of 16 elements (256 bytes), one per group
    // of four m2.  Plans whose SECOND pass has a register pre-stage (n = 2^22) stay row-major: there the second pass lost 1.3 ms of 42 to the
    // runs and the first pass, whose two halves of the frequencies interleave in 64-byte segments, gained nothing (profiles/ntt_tile_major.md).
    // Every instance whose tiles can be four columns wide reads the flag (uniform): the 1024 x 4 second pass also serves row-major plans
    // (DISTAFF_NTT=lds at 2^21: 2048 x 2 first pass).
    uint32_t tile_major;
    // The trace coefficients in the same tile-major map (dst_ctx::polys_tm; n1, n2 of the plan: element (m1, m2) = coefficient m1 * n2 + m2).
    // src_tile_major (first pass of an extension, four-column tiles, no pre-stage): `src` is that array -- a tile is one contiguous block of
    // 16 * n1 * 4 bytes instead of n1 64-byte segments a row apart, each sharing its 128-byte line with the neighbouring tile.  dst_tm (last pass of
    // the interpolation, or nullptr): where the pass stores every result once more in that order, beside the natural-order `dst`.
    uint32_t src_tile_major;
    fe* dst_tm;
    uint32_t log_n1, log_n2, tile /* log2 of the tile width */, log_N, log_b;
    uint32_t j0;               // global index of the first local coset
    uint32_t has_scale;        // 1: multiply the result by `scale` (1/n of inverse transforms)
    uint32_t tiles_per_block;  // adjacent tiles one workgroup walks through
    uint32_t debug;            // DISTAFF_NTT_DEBUG (test build): 1 = report the occupancy of every launch shape once
    // pass B addressing (two-pass plans: row stride n2, frequency stride n1, no batch); three-pass plans run the last pass once per
    // middle frequency k2 (batch index = low bits of the tile-group index): source rows (k1, k2, .) and destination k1 + n1 * (k2 + n2' * k3)
    size_t src_row_stride, dst_k_stride, src_batch_stride, dst_batch_stride;
    uint32_t batch_log;
    uint32_t dit;              // pass A of an extension: coset DIT (pre-scale folded into the stage twiddles, taken from `prescale`)
    uint32_t groups, cosets, cols;   // extent of the linear block index: tile groups x cosets x columns (registers)
    uint32_t coset_fast;       // block order of first passes over several cosets, see ntt_block
    // Register pre-stage (instances with PRE = 1): the pass's transform has TWICE the length of its LDS tile.  A workgroup owns one half h
    // of the frequencies (k = 2 k' + h; h = upper half of the tile-group index): it loads the elements m and m + len of a column,
    // forms u_h[m] in registers and runs the len-point LDS transform on it --
    //   coset DIT (extension):  u_h = x[m] + (-1)^h c x[m + len], c = g^len, followed by the coset transform with shift g * w^h
    //                           (virtual coset j + B h of the same pre-scale table);
    //   DIF (everything else):  u_0 = x[m] + x[m + len],  u_1 = (x[m] - x[m + len]) * w_{2 len}^m  (pre_tw).
    // n = 2^21 and 2^22 then stay on the two-pass plan with 1024 x 4 tiles (a third HBM pass costs more than the extra stage).
    uint32_t pre;              // 0 / 1 (read by the PRE instances only)
    const fe_tw* pre_tw;       // w_{2 len}^m, m < len (forward or inverse), DIF pre-stage
    fe_tw scale;
};

__device__ __forceinline__ fe load_fe(const fe* p) { return *p; }

__device__ __forceinline__ fe dom_pow(const fe* lo, const fe* hi, uint32_t lo_bits, uint64_t e) {
    uint32_t l = (uint32_t)e & ((1u << lo_bits) - 1u), h = (uint32_t)(e >> lo_bits);
    fe a = lo[l];
    if (h == 0) return a;
    return fe_mul(a, hi[h]);
}

// Linear block index -> (tile group, local coset, column).  Block b runs on XCD b % 8.  The COLUMN (register) is the fastest dimension and
// the blocks that differ only in it carry the same index modulo 8: the four-step twiddles of a (coset, tile) - the same for every
// register - are served to the other registers by that XCD's L2.  (Round 1 had the register as the slowest grid dimension: the table was
// streamed once per register.)  coset_fast (first passes of an extension): the coset is the next dimension and an XCD finishes a tile
// group before it starts the next, so the coefficient tiles of the group are shared by the cosets as well.
__device__ __forceinline__ void ntt_block(const NttArgs& a, uint32_t& group, uint32_t& jl, uint32_t& col) {
    const uint32_t b = blockIdx.x, units = a.groups * a.cosets;
    uint32_t u;
    if (a.coset_fast) {        // XCD x works through the tile groups x, x + 8, ...; within a group every (coset, register) pair before the next group,
        // the registers in chunks of four: the 64 workgroups resident on an XCD are then 16 cosets x 4 registers of one tile group (a chunk of all
        // 20 registers would leave 3 cosets to share a coefficient tile: measured 41 against 33 GB of L2 misses per proof in the first passes)
        const uint32_t s = b >> 3, pairs = a.cosets * a.cols, pair = s % pairs;
        group = (s / pairs) * 8u + (b & 7u);
        const uint32_t chunk = pair / (4u * a.cosets), in_chunk = pair - chunk * 4u * a.cosets;
        const uint32_t width = (chunk * 4u + 4u <= a.cols) ? 4u : a.cols - chunk * 4u;              // the last chunk may be narrower
        col = chunk * 4u + in_chunk % width; jl = in_chunk / width;
        return;
    }
    if ((units & 7u) == 0) { const uint32_t s = b >> 3; col = s % a.cols; u = (s / a.cols) * 8u + (b & 7u); }
    else { col = b % a.cols; u = b / a.cols; }
    jl = u / a.groups; group = u % a.groups;
}

// consumer of the last butterfly round of the second passes (ntt_lds.h): the results leave for HBM without another pass over LDS
struct OutB {                                          // natural-order store X[k1 + n1 * k2] from the last round, 1/n of inverse transforms on the way
    static constexpr bool active = true;
    fe* __restrict__ dst /* at the tile's first k1 */; uint32_t k_stride, log_n2; bool scale; fe_tw s;
    uint32_t pre_shift, h;                             // register pre-stage: the tile holds the frequencies k2 = (k' << pre_shift) + h
    // NttArgs::dst_tm (uniform; nullptr in every launch but the interpolation's): the array's start, the tile's first k1 and the plan's log2 n1, log2 n2
    fe* __restrict__ dst_tm; uint32_t k0, log_rows, log_cols;
    struct Tok {};
    __device__ __forceinline__ Tok pre(uint32_t, uint32_t) const { return Tok{}; }
    __device__ __forceinline__ void put(uint32_t row, uint32_t t, const fe& v, const Tok&) const {
        const uint32_t k2 = ((log_n2 ? (__brev(row) >> (32 - log_n2)) : 0u) << pre_shift) + h;
        const fe r = scale ? fe_mul_tw(v, s) : v;
#if NTT_STREAM_B_STORE
        fe_store_stream(dst + (k2 * k_stride + t), r);
#else
        dst[k2 * k_stride + t] = r;                                      // uniform base + 32-bit lane offset (at most 2^24 points)
#endif
        if (dst_tm != nullptr) {                                         // coefficient m = m1 * n2 + m2 of the natural order, tile-major (NttArgs)
            const uint32_t m = k0 + t + k2 * k_stride, m2 = m & ((1u << log_cols) - 1u), m1 = m >> log_cols;
            dst_tm[((((m2 >> 2) << log_rows) + m1) << 2) + (m2 & 3u)] = r;      // read next by every coset of the extension: no streaming hint
        }
    }
};

// Streaming hints on the arrays a pass touches exactly once (fe_store_stream / fe_load_stream, fe.h): the staging array between the passes
// (written by the first, read by the second) and the finished extension (read next by the leaf hashing).  Measured on one lease, four
// alternating rounds of the 2^20 proof (tools/ab_multi.sh, round 5): none 35.63 ms, first-pass stores 35.30, + second-pass stores 35.16,
// + second-pass loads 35.15 (first passes 11.84 -> 11.41 ms).  FETCH_SIZE of the first passes does not move (10.3 -> 10.1 GB raw per proof):
// what they re-read is not pushed out by their own output, it is the four-step table and the coefficient tiles in 64-byte row segments.
#ifndef NTT_STREAM_STORE
#define NTT_STREAM_STORE 1
#endif
#ifndef NTT_STREAM_B_STORE
#define NTT_STREAM_B_STORE 1
#endif
#ifndef NTT_STREAM_B_LOAD
#define NTT_STREAM_B_LOAD 1
#endif
// Laboratory switches of the first pass (tools/r6_lde_lab.sh; WRONG results on purpose, never defined in a build that ships): each takes one
// of the pass's three global streams out of the memory system while every instruction stays -- the bound of anything that could be done
// about that stream.  NTT_LAB_SRC_SMALL=1: the coefficient loads of every workgroup fall into a 64 KiB window (cache hits); =2: only those
// of the odd-half workgroups of a register pre-stage pass (the upper bound of SHARING the loads between the halves);
// NTT_LAB_TW4_SMALL: the four-step twiddles come from a 64 KiB window per coset.  (A third switch stored a tile as one contiguous 64 KiB
// block instead of 64-byte row segments a row stride apart: that is what the tile-major layout now does with right results.)
// (the window is indexed by (row, column) of the tile, so every row still carries different data: a window indexed by the masked ARRAY offset
// would make the columns periodic, their spectra sparse -- and the kernels measurably faster for that alone, their time depends on the data)
#if defined(NTT_LAB_SRC_SMALL)
#define NTT_LAB_SRC(row, t, off) ((((NTT_LAB_SRC_SMALL) == 1) || hh) ? ((((row) & 1023u) << 2) + ((t) & 3u)) : (off))
#else
#define NTT_LAB_SRC(row, t, off) (off)
#endif
#if defined(NTT_LAB_TW4_SMALL)
#define NTT_LAB_TW(row, t, off) ((((row) & 1023u) << 2) + ((t) & 3u))
#else
#define NTT_LAB_TW(row, t, off) (off)
#endif
#if defined(NTT_LAB_STAMPS)
// [pass 0/1][workgroup slot 256][wave 16][tile 2][stamp 16]: written by lane 0 of every wave of the workgroups blockIdx.x = 61 * slot
#define NTT_LAB_WG_STRIDE 61u
__device__ unsigned long long ntt_lab_buf[2 * 256 * 16 * 2 * 16];
extern "C" __attribute__((visibility("default"))) int dst_lab_stamps(unsigned long long* out, size_t count, int clear) {
    if (count > sizeof(ntt_lab_buf) / 8) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ntt_lab_buf), count * 8) != hipSuccess) return -2;
    if (clear) { static unsigned long long zero[2 * 256 * 16 * 2 * 16]; if (hipMemcpyToSymbol(HIP_SYMBOL(ntt_lab_buf), zero, sizeof zero) != hipSuccess) return -3; }
    return 0;
}
#define NTT_LAB_FLUSH(pass, it, st, nst) do { \
    if ((blockIdx.x % NTT_LAB_WG_STRIDE) == 0u && blockIdx.x / NTT_LAB_WG_STRIDE < 256u && (it) < 2u && (threadIdx.x & 63u) == 0u) { \
        unsigned long long* o_ = ntt_lab_buf + ((((size_t)(pass) * 256u + blockIdx.x / NTT_LAB_WG_STRIDE) * 16u + (threadIdx.x >> 6)) * 2u + (it)) * 16u; \
        for (int k_ = 0; k_ < (nst); k_++) o_[k_] = (st)[k_]; } } while (0)
#else
#define NTT_LAB_FLUSH(pass, it, st, nst) ((void)0)
#endif
// One-sided lazy butterflies in the coset DIT of a first pass (ntt_lds.h LAZY, fe_addsub_lazy).  The invariant: every sum and difference of a
// DIT round is u +- v * w, and v * w leaves fe_mul_tw canonical; so u may be ANY 128-bit value, one wrap by 2^128 -> C128 keeps the sum below
// 2^128, fe_sub is right as it is, and the next round's fe_mul_tw takes what comes.  The lazy values end in the read-out of ntt_pass_a, which
// multiplies EVERY element by its four-step twiddle (fe_mul / fe_mul_tw: any 128-bit operand) and so stores canonical values; nothing else
// reads the tile.  The register pre-stage's own fe_add / fe_sub, the pre-scale + DIF mode and every second pass (stores without a
// multiplication behind it, and both operands of its sums are sums) keep the canonical form.  -DNTT_DIT_LAZY=0: canonical rounds (A/B).
#ifndef NTT_DIT_LAZY
#define NTT_DIT_LAZY 1
#endif
// -DNTT_COEFF_TILE_MAJOR=0: no copy of the trace coefficients in tile order (NttArgs::src_tile_major), the extension reads `polys` row-major (A/B)
#ifndef NTT_COEFF_TILE_MAJOR
#define NTT_COEFF_TILE_MAJOR 1
#endif
extern __shared__ __attribute__((aligned(16))) unsigned char ntt_smem[];

// Both passes are persistent over `tiles_per_block` adjacent tiles.  PREFETCH instances (WPE = 4 waves per SIMD, 128 registers): the
// tile's elements for the NEXT iteration are fetched from HBM into registers before the butterfly stages of the current one start, so
// the HBM latency and most of the transfer overlap with the arithmetic (measured: a block of this occupancy that loads, computes and
// stores in sequence pays HBM time + ALU time, not their maximum).  <1024, 8, false>: two workgroups of 1024 lanes per CU, 8 waves per
// SIMD in 64 registers, no prefetch -- while one workgroup loads, the other one's 16 waves keep the SIMDs busy (ntt_select picks it for
// 1024-point tiles).  The stage twiddles live in LDS behind the tile as table pairs (32 bytes each), so the stages issue no global loads
// that would have to wait behind the prefetch.  A 1024-point coset DIT with its whole table in LDS needs 64 KiB of tile + 32 KiB of
// twiddles: that instance runs as ONE workgroup of 1024 lanes per CU; everything that fits 80 KiB runs as two workgroups per CU.
// LOG_LEN / LOG_T != 0: the instance of ONE tile shape (2^LOG_LEN points x 2^LOG_T columns) -- its rounds are separate code with literal
// strides (ntt_lds.h) and the tile index arithmetic folds into immediates; 0: any shape, from the arguments.
template <int THREADS, int WPE = 4, bool PREFETCH = true, int LOG_LEN = 0, int LOG_T = 0, int PRE = 0>
__global__ void __launch_bounds__(THREADS, WPE) ntt_pass_a(NttArgs a, const fe* __restrict__ src_base, fe* __restrict__ dst_base) {
    constexpr int EPT = NTT_TILE_ELEMS / THREADS;
    fe* L = reinterpret_cast<fe*>(ntt_smem);
    const uint32_t log_n1 = LOG_LEN ? (uint32_t)LOG_LEN : a.log_n1;          // length of the LDS transform (half of the pass's with PRE)
    const uint32_t log_t = LOG_T ? (uint32_t)LOG_T : a.tile, T = 1u << log_t, n1 = 1u << log_n1;
    fe_tw* TW = reinterpret_cast<fe_tw*>(L + n1 * T);
    uint32_t group, jl, col;
    ntt_block(a, group, jl, col);
    uint32_t hh = 0;                                       // PRE: which half of the frequencies this workgroup produces
    if (PRE) { const uint32_t half = a.groups >> 1; hh = group >= half ? 1u : 0u; group -= hh * half; }
    const uint32_t jg = a.j0 + jl;
    const fe* __restrict__ src0 = src_base + (size_t)col * a.src_col_stride + (size_t)jl * a.src_coset_stride;
    fe* __restrict__ dst0 = dst_base + (size_t)col * a.dst_col_stride + (size_t)jl * a.dst_coset_stride;
    const uint32_t pmask = (1u << (a.log_b + log_n1 + PRE)) - 1u;
    // layout of dst and tw4 (NttArgs); the 16-column instances exist in row-major plans only
    const bool tile_major = (LOG_T != 0 && LOG_T != 2) ? false : a.tile_major != 0;
    const uint32_t jv = jg + (hh << a.log_b);              // PRE: the half-length transform of frequencies 2k' + h is the coset transform with shift g * w^h
    if (a.dit) {
        // stage twiddles of this coset: g^(n1/B) * w_B^k = w_{B_lde*n1}^((j + B_lde*k) * n1/B) straight from the pre-scale table
        const uint32_t in_lds = a.dit_last ? n1 / 2 : n1;                                     // entries + 1
        for (uint32_t i = threadIdx.x; i + 1 < in_lds; i += THREADS) {
            const uint32_t lb = 31u - (uint32_t)__clz(i + 1), k = i + 1 - (1u << lb);         // entry i: block size B = 2^(lb+1), index k
            TW[i] = a.prescale[((jv + (k << (a.log_b + PRE))) << (log_n1 - lb - 1)) & pmask];
        }
    } else
    for (uint32_t i = threadIdx.x; i < n1 / 2; i += THREADS) TW[dif_tw_slot(i)] = a.stage_tw[i];
    const bool scaled = !a.dit && a.prescale != nullptr && jg != 0;
    fe pre0 = fe_zero(), pre1 = fe_zero(), pre2 = fe_zero(), pre3 = fe_zero(), pre4 = fe_zero(), pre5 = fe_zero(), pre6 = fe_zero(), pre7 = fe_zero();
    const uint32_t count = n1 * T;
    // named registers, not an array: the prefetched elements must stay in VGPRs across the butterfly stages.  Branch-free fetch: a
    // lane past the tile re-reads element 0.
#define NTT_EACH(M) { M(0, pre0) M(1, pre1) M(2, pre2) M(3, pre3) M(4, pre4) M(5, pre5) M(6, pre6) M(7, pre7) }
    // uniform base (scalar registers) + 32-bit lane offset: the transform has at most 2^24 points
    // Element (row, column) of the tile that lane index idx carries.  A coset DIT enters LDS bit-reversed: the rows r .. r + 3 of one LDS
    // access group land 256-byte multiples apart, i.e. on the same banks; rotating the column by the row spreads them (the 64-byte HBM
    // segment of a row is read by the same four lanes as before, in another order).
    const bool rot_a = a.dit && log_t == 2 && !NTT_NO_ROTATE_DEFINED;
#define NTT_COL_A(idx) (rot_a ? (((idx) + ((idx) >> log_t)) & (T - 1)) : ((idx) & (T - 1)))
    // PRE: the element is formed from the rows m and m + n1 of the column as it arrives (see NttArgs)
    const fe_tw pre_c = (PRE && a.dit) ? a.prescale[(jg << log_n1) & pmask] : fe_tw{};       // c = g^len
    auto pre_stage_a = [&](const fe& x0, const fe& x1, uint32_t row) -> fe {
        if (a.dit) { const fe t = fe_mul_tw(x1, pre_c); return hh ? fe_sub(x0, t) : fe_add(x0, t); }
        return hh ? fe_mul_tw(fe_sub(x0, x1), a.pre_tw[row]) : fe_add(x0, x1);
    };
#define NTT_FETCH_A1(e, var) if constexpr ((e) < EPT) { uint32_t idx = lane + (e) * THREADS; idx = idx < count ? idx : 0u; \
        if constexpr (PRE != 0) { const uint32_t row_ = idx >> log_t; const fe x0_ = src[NTT_LAB_SRC(row_, NTT_COL_A(idx), (row_ << a.log_n2) + NTT_COL_A(idx))], x1_ = src[NTT_LAB_SRC(row_ + 512u, NTT_COL_A(idx), ((row_ + n1) << a.log_n2) + NTT_COL_A(idx))]; var = pre_stage_a(x0_, x1_, row_); } \
        else var = src[NTT_LAB_SRC(idx >> log_t, NTT_COL_A(idx), ((idx >> log_t) << src_row_shift) + NTT_COL_A(idx))]; }
    // tile-major coefficients (NttArgs::src_tile_major): the tile is the block at tile * count and a row is T elements long -- the lane index
    // with its column rotated; row-major: the tile's first column, rows n2 apart
#define NTT_FETCH_A(tile) { const fe* __restrict__ src = src0 + (src_tm ? (size_t)(tile) * count : (size_t)(tile) * T); NTT_EACH(NTT_FETCH_A1) }
    const bool src_tm = (PRE || (LOG_T != 0 && LOG_T != 2)) ? false : a.src_tile_major != 0;
    const uint32_t src_row_shift = src_tm ? log_t : a.log_n2;
    const tw4_t* __restrict__ tw4 = a.tw4 + (size_t)jl * a.tw4_coset_stride;
    const uint32_t tile0 = group * a.tiles_per_block;
    uint32_t lane = threadIdx.x;
    if (PREFETCH) NTT_FETCH_A(tile0)
    for (uint32_t it = 0; it < a.tiles_per_block; it++) {
        const uint32_t tile = tile0 + it;
        unsigned long long st[16]; (void)st;               // laboratory stamps (NTT_STAMP: nothing in the product build)
        NTT_STAMP_REAL(st, 14);
        NTT_STAMP(st, 8);
        lane = lds_opaque_lane();                          // per-tile index arithmetic is recomputed, not kept live (and spilled) across the loop
        if (!PREFETCH) NTT_FETCH_A(tile)
        NTT_STAMP(st, 9);
        __syncthreads();                                   // the previous tile has left LDS (and TW is complete)
        NTT_STAMP(st, 10);
        // DISTAFF_NTT_DIF: pre-scale + DIF instead of the coset DIT
#define NTT_PUT_A(e, var) if constexpr ((e) < EPT) { const uint32_t idx = lane + (e) * THREADS; if (idx < count) { if (a.dit) L[lds_slot(__brev(idx >> log_t) >> (32 - log_n1), NTT_COL_A(idx), log_t)] = var; else L[lds_slot(idx >> log_t, idx & (T - 1), log_t)] = scaled ? fe_mul_tw(var, a.prescale[(jg * (idx >> log_t)) & pmask]) : var; } }
        NTT_EACH(NTT_PUT_A)
#undef NTT_PUT_A
        NTT_STAMP(st, 11);
        __syncthreads();
        NTT_STAMP(st, 12);
        if (PREFETCH && it + 1 < a.tiles_per_block) NTT_FETCH_A(tile + 1)
        if constexpr (LOG_LEN != 0) {
            if (a.dit) lds_ntt_dit_fixed<THREADS, LOG_LEN, LOG_T, NttKeepInLds, NTT_DIT_LAZY != 0>(L, TW, a.dit_last ? a.dit_last + (size_t)((jg << PRE) + hh) * (n1 / 2) : nullptr, NttKeepInLds(), st);
            else lds_ntt_dif_fixed<THREADS, LOG_LEN, LOG_T>(L, TW, NttKeepInLds(), st);
        } else {
            if (a.dit) lds_ntt_dit<THREADS, NttKeepInLds, NTT_DIT_LAZY != 0>(L, TW, log_n1, log_t, 1u, log_n1 + 1u, a.dit_last ? a.dit_last + (size_t)((jg << PRE) + hh) * (n1 / 2) : nullptr);
            else lds_ntt_dif<THREADS>(L, TW, log_n1, log_t, 1u, log_n1 + 1u);
        }
        // read-out in batches of RB elements per lane: the twiddle loads of a batch are in flight together (the 512-lane instance also
        // holds eight prefetched elements: a batch of four would spill).  The second passes store from their last butterfly round instead
        // (OutB); here that does not pay: in the 128-register instances the four-step twiddles (and the last-stage pairs from global memory)
        // live in the last round spill (13.15 / 13.3 against 13.05 ms), in the spill-free fixed-shape instance it is within the noise
        // (18.85 against 18.95 ms of extension, with the twiddle requested before or after the butterfly).
        constexpr int RB = WPE > 4 ? 1 : THREADS == 512 ? 2 : 4;
        // tile-major: the tile's block of the staging array and of the table, count << PRE elements each; row-major: its first column
        const size_t tile_at = tile_major ? (size_t)tile * (count << PRE) : (size_t)tile * T;
        fe* __restrict__ dst = dst0 + tile_at;           // uniform bases, 32-bit lane offsets
        const tw4_t* __restrict__ tw = tw4 + tile_at;
        for (uint32_t base = 0; base < count; base += RB * THREADS) {
            fe v[RB]; tw4_t w[RB]; uint32_t off[RB]; bool ok[RB];
            static_for<0, RB>([&](auto q_) {
                constexpr int q = decltype(q_)::value;
                uint32_t idx = base + q * THREADS + lane;
                ok[q] = idx < count;
                idx = ok[q] ? idx : 0u;
                const uint32_t t = idx & (T - 1), r = idx >> log_t;
                if (tile_major && a.dit && !PRE) off[q] = idx;                                      // the block is the tile as it lies in LDS
                else {
                    const uint32_t k1 = ((a.dit ? r : __brev(r) >> (32 - log_n1)) << PRE) + hh;    // DIT leaves the tile in natural order; PRE: frequencies 2 k' + h
                    off[q] = tile_major ? (k1 << log_t) + t : (k1 << a.log_n2) + t;
                }
                v[q] = L[idx];
                w[q] = tw[NTT_LAB_TW(r, t, off[q])];
            });
            static_for<0, RB>([&](auto q_) {
                constexpr int q = decltype(q_)::value;
#if NTT_TW4_PAIRS
                const fe out_q = fe_mul_tw(v[q], w[q]);
#else
                const fe out_q = fe_mul(v[q], w[q]);
#endif
#if NTT_STREAM_STORE
                if (ok[q]) fe_store_stream(dst + off[q], out_q);          // the staging array: read next by the second pass, not by this one
#else
                if (ok[q]) dst[off[q]] = out_q;
#endif
            });
        }
        NTT_STAMP(st, 13);
        NTT_STAMP_REAL(st, 15);
        NTT_LAB_FLUSH(0, it, st, 16);
    }
}

// WPE: waves per SIMD the instance is compiled for (its register budget); PREFETCH: the next tile travels in registers during the rounds
template <int THREADS, int WPE = 4, bool PREFETCH = true, int LOG_LEN = 0, int LOG_T = 0, int PRE = 0>
__global__ void __launch_bounds__(THREADS, WPE) ntt_pass_b(NttArgs a, const fe* __restrict__ src_base, fe* __restrict__ dst_base) {
    constexpr int EPT = NTT_TILE_ELEMS / THREADS;
    fe* L = reinterpret_cast<fe*>(ntt_smem);
    const uint32_t log_n2 = LOG_LEN ? (uint32_t)LOG_LEN : a.log_n2;          // length of the LDS transform (half of the pass's with PRE)
    const uint32_t log_t = LOG_T ? (uint32_t)LOG_T : a.tile, T = 1u << log_t, n2 = 1u << log_n2;
    fe_tw* TW = reinterpret_cast<fe_tw*>(L + n2 * T);
    uint32_t g, jl, col;
    ntt_block(a, g, jl, col);
    uint32_t hh = 0;                                       // PRE: which half of the frequencies this workgroup produces (two-pass plans: no batches)
    if (PRE) { const uint32_t half = a.groups >> 1; hh = g >= half ? 1u : 0u; g -= hh * half; }
    const uint32_t batch = g & ((1u << a.batch_log) - 1u), group = g >> a.batch_log;
    const fe* __restrict__ src = src_base + (size_t)col * a.src_col_stride + (size_t)jl * a.src_coset_stride + (size_t)batch * a.src_batch_stride;
    fe* __restrict__ dst = dst_base + (size_t)col * a.dst_col_stride + (size_t)jl * a.dst_coset_stride + (size_t)batch * a.dst_batch_stride;
    for (uint32_t i = threadIdx.x; i < n2 / 2; i += THREADS) TW[dif_tw_slot(i)] = a.stage_tw[i];
    fe pre0 = fe_zero(), pre1 = fe_zero(), pre2 = fe_zero(), pre3 = fe_zero(), pre4 = fe_zero(), pre5 = fe_zero(), pre6 = fe_zero(), pre7 = fe_zero();
    const uint32_t count = n2 * T;
    // contiguous along m2
    // Four-column tiles: lane index = (m2, row), row fastest -- a wavefront reads 16 consecutive elements (256 bytes) of each of the four
    // rows and writes 64 consecutive LDS slots.  (With m2 fastest the slots of neighbouring lanes are 64 bytes apart: the 16 lanes of an
    // access group share their banks four times over.)  Wider tiles keep m2 fastest.
    // Tile-major source (NttArgs): the four rows of a group of four m2 are one run of 16 elements, the runs of a tile are run_stride = 4 * (number
    // of k1) elements apart.  Lane index = (group of four m2, row, m2 & 3): the 16 lanes of an access group read one run in address order and
    // write its 4 x 4 transpose into 16 distinct LDS slots of one 256-byte line.  A second pass with a pre-stage always reads row-major.
    const bool tile_major = (PRE || (LOG_T != 0 && LOG_T != 2)) ? false : a.tile_major != 0;
    const uint32_t run_shift = a.log_n1 + 2u;
    const bool colfast_b = log_t == 2 && !NTT_NO_ROTATE_DEFINED;
#define NTT_ROW_B(idx) (tile_major ? (((idx) >> 2) & 3u) : colfast_b ? ((idx) & (T - 1)) : ((idx) >> log_n2))
#define NTT_M2_B(idx) (tile_major ? ((((idx) >> 4) << 2) + ((idx) & 3u)) : colfast_b ? ((idx) >> log_t) : ((idx) & (n2 - 1)))
#define NTT_OFF_B(idx) (tile_major ? ((((idx) >> 4) << run_shift) + ((idx) & 15u)) : (NTT_ROW_B(idx) * row_stride + NTT_M2_B(idx)))
    // PRE (DIF pre-stage, see NttArgs): u_0 = y[m] + y[m + n2], u_1 = (y[m] - y[m + n2]) * w_{2 n2}^m
#if NTT_STREAM_B_LOAD
#define NTT_LOAD_B(p) fe_load_stream(p)
#else
#define NTT_LOAD_B(p) (*(p))
#endif
#define NTT_FETCH_B1(e, var) if constexpr ((e) < EPT) { uint32_t idx = lane + (e) * THREADS; idx = idx < count ? idx : 0u; \
        if constexpr (PRE != 0) { const uint32_t m_ = NTT_M2_B(idx); const fe* p_ = srct + NTT_OFF_B(idx); const fe x0_ = p_[0], x1_ = p_[n2]; \
                                  var = hh ? fe_mul_tw(fe_sub(x0_, x1_), a.pre_tw[m_]) : fe_add(x0_, x1_); } \
        else var = NTT_LOAD_B(srct + NTT_OFF_B(idx)); }
#define NTT_FETCH_B(tile) { const fe* __restrict__ srct = src + (tile_major ? (size_t)(tile) * (T * T) : (size_t)((tile) * T) * a.src_row_stride); NTT_EACH(NTT_FETCH_B1) }
    const uint32_t row_stride = (uint32_t)a.src_row_stride;
    const uint32_t tile0 = group * a.tiles_per_block;
    uint32_t lane = threadIdx.x;
    if (PREFETCH) NTT_FETCH_B(tile0)
    for (uint32_t it = 0; it < a.tiles_per_block; it++) {
        const uint32_t k1_0 = (tile0 + it) * T;
        unsigned long long st[16]; (void)st;               // laboratory stamps (NTT_STAMP: nothing in the product build)
        NTT_STAMP_REAL(st, 14);
        NTT_STAMP(st, 8);
        lane = lds_opaque_lane();
        if (!PREFETCH) NTT_FETCH_B(tile0 + it)
        NTT_STAMP(st, 9);
        __syncthreads();
        NTT_STAMP(st, 10);
#define NTT_PUT_B(e, var) if constexpr ((e) < EPT) { const uint32_t idx = lane + (e) * THREADS; if (idx < count) L[lds_slot(NTT_M2_B(idx), NTT_ROW_B(idx), log_t)] = var; }
        NTT_EACH(NTT_PUT_B)
#undef NTT_PUT_B
        NTT_STAMP(st, 11);
        __syncthreads();
        NTT_STAMP(st, 12);
        if (PREFETCH && it + 1 < a.tiles_per_block) NTT_FETCH_B(tile0 + it + 1)
        const OutB out{dst + k1_0, (uint32_t)a.dst_k_stride, log_n2, a.has_scale != 0, a.scale, (uint32_t)PRE, hh,
                       (PRE || a.dst_tm == nullptr) ? nullptr : a.dst_tm + (size_t)col * a.dst_col_stride, k1_0, a.log_n1, a.log_n2};
        const fe_tw* Wuse = TW;
        if constexpr (LOG_LEN != 0) lds_ntt_dif_fixed<THREADS, LOG_LEN, LOG_T, OutB>(L, Wuse, out, st);
        else lds_ntt_dif<THREADS, OutB>(L, Wuse, log_n2, log_t, 1u, log_n2 + 1u, out);
        NTT_STAMP(st, 13);
        NTT_STAMP_REAL(st, 15);
        NTT_LAB_FLUSH(1, it, st, 16);
    }
}

// ---- register-radix transform (tile lengths 2^6 .. 2^12) -----------------------------------------------------------------------
// The same two passes, but every lane keeps 16 points in registers and runs 3-4 butterfly stages on them before the tile is
// exchanged through LDS, so a 1024-point tile needs two LDS exchanges and two barriers instead of ten.  Mixed-radix
// Cooley-Tukey over the digits (r1, r2[, r3]) of the tile length L = 2^(r1+r2+r3): with the time index written
// m = (m1, m2, m3) (m1 most significant) and the frequency k = k1 + R1*k2 + R1*R2*k3,
//   round i: for fixed other digits, the R_i-point DFT over m_i (radix-2 DIF in registers, roots w_16^j from the kernel
//            arguments, i.e. scalar registers), then the twiddle w_{L_i}^(k_i * mlow) from the stage table (L_i = remaining
//            length, mlow = the digits below i); the slot (.., m_i, ..) of the tile now holds (.., k_i, ..).
// Round 1 reads straight from HBM and the last round writes straight to HBM; lanes run over the T tile columns first, so
// every HBM access is a T*16-byte segment as before.  LDS slot = digits * T + t with an XOR swizzle that moves the 8-lane
// groups of the last round (stride R_q*T slots) onto distinct banks.
template <int LOGL> struct NttDigits;
template <> struct NttDigits<6>  { static constexpr int r1 = 3, r2 = 3, r3 = 0, log_t = 2; };
template <> struct NttDigits<7>  { static constexpr int r1 = 4, r2 = 3, r3 = 0, log_t = 2; };
template <> struct NttDigits<8>  { static constexpr int r1 = 4, r2 = 4, r3 = 0, log_t = 2; };
template <> struct NttDigits<9>  { static constexpr int r1 = 3, r2 = 3, r3 = 3, log_t = 2; };
template <> struct NttDigits<10> { static constexpr int r1 = 4, r2 = 3, r3 = 3, log_t = 2; };
template <> struct NttDigits<11> { static constexpr int r1 = 4, r2 = 4, r3 = 3, log_t = 2; };
template <> struct NttDigits<12> { static constexpr int r1 = 4, r2 = 4, r3 = 4, log_t = 1; };

struct NttRegArgs {
    const fe* src; fe* dst;
    size_t src_col_stride, src_coset_stride, dst_col_stride, dst_coset_stride;
    size_t in_stride_m, in_stride_t;    // element strides of the time index and of the tile column on input
    size_t out_stride_k;                // element stride of the frequency index on output (tile columns are contiguous)
    const fe_tw* stage_tw;              // w_L^t, t < L/2 (table pairs)
    const fe* tw_lo; const fe* tw_hi;   // two-level table of w_N (pass A four-step twiddle) or nullptr
    const fe_tw* prescale;              // w_{B*L}^t or nullptr
    uint32_t lo_bits, log_N, log_b, j0, coset_twiddle, has_scale;
    fe scale;
    fe c16[8];                          // w_16^j (forward or inverse), j < 8
};

constexpr __host__ __device__ int ntt_brev(int v, int bits) { int r = 0; for (int i = 0; i < bits; i++) r |= ((v >> i) & 1) << (bits - 1 - i); return r; }

// One out-of-line copy of the 128-bit modular multiplication for the register-radix kernels: with every call site inlined a
// 1024-point kernel is ~190 KB of straight-line code, several times the 64 KB instruction cache a CU pair shares, and the waves
// stall on instruction fetch; as a call the kernel is a few thousand instructions.
__device__ __attribute__((noinline)) fe fe_mul_call(fe a, fe b) { return fe_mul(a, b); }
__device__ __attribute__((noinline)) fe fe_mul_tw_call(fe a, fe p, fe q) { return fe_mul_tw(a, p, q); }

// radix-2 DIF over x[0 .. 2^r): x[rho] <- X[brev_r(rho)]
template <int r>
__device__ __forceinline__ void dft_regs(fe* x, const fe* c16) {
    constexpr int R = 1 << r;
    static_for<0, r>([&](auto s_) {
        constexpr int s = decltype(s_)::value, half = R >> (s + 1);
        static_for<0, R / 2>([&](auto i_) {
            constexpr int i = decltype(i_)::value, b = (i / half) * 2 * half, j = i % half;
            fe u = x[b + j], v = x[b + j + half];
            x[b + j] = fe_add(u, v);
            fe d = fe_sub(u, v);
            if constexpr (j == 0) x[b + j + half] = d;
            else x[b + j + half] = fe_mul_call(d, c16[(j << s) << (4 - r)]);
        });
    });
}

// v * w_L^e from the half table: w_L^(e + L/2) = -w_L^e
template <int LOGL>
__device__ __forceinline__ fe mul_stage_twiddle(const fe& v, const fe_tw* __restrict__ tw, uint32_t e) {
    constexpr uint32_t H = 1u << (LOGL - 1);
    const fe_tw w = tw[e & (H - 1)];
    const fe r = fe_mul_tw_call(v, w.p, w.q);
    return (e & H) ? fe_neg(r) : r;
}

template <int LOGL>
__global__ void __launch_bounds__((1 << (LOGL + NttDigits<LOGL>::log_t)) / 16, (LOGL + NttDigits<LOGL>::log_t >= 13) ? 1 : 2) ntt_reg_kernel(NttRegArgs a) {
    using D = NttDigits<LOGL>;
    constexpr int r1 = D::r1, r2 = D::r2, r3 = D::r3, LT = D::log_t, T = 1 << LT;
    constexpr int rq = r3 ? r3 : r2;                               // last digit
    constexpr int L = 1 << LOGL, E = 16, NT = L * T / E;
    constexpr int SWZ_SHIFT = LT + rq, SWZ_MASK = 8 / T - 1;
    __shared__ fe tile[L * T];
    auto phys = [](uint32_t s) -> uint32_t { return s ^ (((s >> SWZ_SHIFT) & SWZ_MASK) << LT); };
    const uint32_t tid = threadIdx.x;
    const uint32_t jl = blockIdx.y, jg = a.j0 + jl;
    const fe* src = a.src + (size_t)blockIdx.z * a.src_col_stride + (size_t)jl * a.src_coset_stride + (size_t)blockIdx.x * T * a.in_stride_t;
    fe* dst = a.dst + (size_t)blockIdx.z * a.dst_col_stride + (size_t)jl * a.dst_coset_stride + (size_t)blockIdx.x * T;
    fe x[E];

    // ---- round 1: HBM -> registers -> LDS
    {
        constexpr int R = 1 << r1, LO = L >> r1, SETS = E / R;
        static_for<0, E>([&](auto i_) {
            constexpr int i = decltype(i_)::value, u = i / R, d = i % R;
            const uint32_t w = tid + NT * u, t = w & (T - 1), p = w >> LT;
            x[i] = src[(size_t)(d * LO + p) * a.in_stride_m + (size_t)t * a.in_stride_t];
        });
        if (a.prescale != nullptr && jg != 0) {
            const uint32_t pmask = (1u << (a.log_b + LOGL)) - 1u;
            static_for<0, E>([&](auto i_) {
                constexpr int i = decltype(i_)::value, u = i / R, d = i % R;
                const uint32_t p = (tid + NT * u) >> LT;
                const fe_tw w = a.prescale[(jg * (uint32_t)(d * LO + p)) & pmask];
                x[i] = fe_mul_tw_call(x[i], w.p, w.q);
            });
        }
        static_for<0, SETS>([&](auto u_) {
            constexpr int u = decltype(u_)::value;
            const uint32_t w = tid + NT * u, t = w & (T - 1), p = w >> LT;
            dft_regs<r1>(x + u * R, a.c16);
            static_for<0, R>([&](auto rho_) {
                constexpr int rho = decltype(rho_)::value, k = ntt_brev(rho, r1);
                fe v = x[u * R + rho];
                if constexpr (k != 0) v = mul_stage_twiddle<LOGL>(v, a.stage_tw, (uint32_t)k * p);
                tile[phys((((uint32_t)k * LO + p) << LT) + t)] = v;
            });
        });
    }
    __syncthreads();
    // ---- round 2 of 3: LDS -> registers -> LDS (slots are owned by one lane, so only the rounds are separated by barriers)
    if constexpr (r3 != 0) {
        constexpr int R = 1 << r2, LO = L >> (r1 + r2), SETS = E / R;
        static_for<0, SETS>([&](auto u_) {
            constexpr int u = decltype(u_)::value;
            const uint32_t w = tid + NT * u, t = w & (T - 1), rest = w >> LT, low = rest & (LO - 1), high = rest / LO;
            const uint32_t base = (high * (R * LO) + low);
            static_for<0, R>([&](auto d_) {
                constexpr int d = decltype(d_)::value;
                x[u * R + d] = tile[phys(((base + d * LO) << LT) + t)];
            });
            dft_regs<r2>(x + u * R, a.c16);
            static_for<0, R>([&](auto rho_) {
                constexpr int rho = decltype(rho_)::value, k = ntt_brev(rho, r2);
                fe v = x[u * R + rho];
                if constexpr (k != 0) v = mul_stage_twiddle<LOGL>(v, a.stage_tw, ((uint32_t)k * low) << r1);
                tile[phys(((base + k * LO) << LT) + t)] = v;
            });
        });
        __syncthreads();
    }
    // ---- last round: LDS -> registers -> HBM
    {
        constexpr int R = 1 << rq, SETS = E / R;
        const uint64_t nmask = (1ull << a.log_N) - 1ull;
        static_for<0, SETS>([&](auto u_) {
            constexpr int u = decltype(u_)::value;
            const uint32_t w = tid + NT * u, t = w & (T - 1), high = w >> LT;
            static_for<0, R>([&](auto d_) {
                constexpr int d = decltype(d_)::value;
                x[u * R + d] = tile[phys(((high * R + d) << LT) + t)];
            });
            dft_regs<rq>(x + u * R, a.c16);
            // frequency of the digits above: k1 + R1 * k2 (three rounds: high = k1 * R2 + k2) or k1 (two rounds)
            const uint32_t klow = r3 ? ((high >> r2) + ((high & ((1u << r2) - 1u)) << r1)) : high;
            const uint32_t m2 = blockIdx.x * T + t;
            static_for<0, R>([&](auto rho_) {
                constexpr int rho = decltype(rho_)::value;
                const uint32_t k = klow + ((uint32_t)ntt_brev(rho, rq) << (LOGL - rq));
                fe v = x[u * R + rho];
                if (a.tw_lo != nullptr) {
                    uint64_t e = ((uint64_t)m2 * (((uint64_t)k << a.log_b) + (a.coset_twiddle ? jg : 0u))) & nmask;
                    if (e != 0) {
                        const uint32_t el = (uint32_t)e & ((1u << a.lo_bits) - 1u), eh = (uint32_t)(e >> a.lo_bits);
                        v = fe_mul_call(v, a.tw_lo[el]);
                        if (eh != 0) v = fe_mul_call(v, a.tw_hi[eh]);
                    }
                }
                if (a.has_scale) v = fe_mul_call(v, a.scale);
                dst[(size_t)k * a.out_stride_k + t] = v;
            });
        });
    }
}

// ---- launch layer: instance tables, the plan, one function per pass ---------------------------------------------------------------------
// Every compiled instance of the two LDS passes and of the register-radix kernel is named HERE and nowhere else: the LDS-limit raise, the
// selection, the launch, the occupancy report (DISTAFF_NTT_DEBUG) and dst_ntt_describe all work on a row of these tables.
struct NttInstance { bool pass_b; int threads, wpe; bool prefetch; int log_len, log_t, pre; void (*kernel)(NttArgs, const fe*, fe*); };
#define NTT_INSTANCE(PASS_B, KERNEL, ...) {PASS_B, __VA_ARGS__, KERNEL<__VA_ARGS__>}
static const NttInstance NTT_INSTANCES[] = {
    // any shape, from the arguments: 512 lanes + prefetch (two workgroups per CU), 1024 lanes for tiles whose twiddles exceed 80 KiB (one per CU),
    // 1024 lanes at 8 waves per SIMD without prefetch for 1024-point tiles
    NTT_INSTANCE(false, ntt_pass_a, 512, 4, true, 0, 0, 0),  NTT_INSTANCE(true, ntt_pass_b, 512, 4, true, 0, 0, 0),
    NTT_INSTANCE(false, ntt_pass_a, 1024, 4, true, 0, 0, 0), NTT_INSTANCE(true, ntt_pass_b, 1024, 4, true, 0, 0, 0),
    NTT_INSTANCE(false, ntt_pass_a, 1024, 8, false, 0, 0, 0), NTT_INSTANCE(true, ntt_pass_b, 1024, 8, false, 0, 0, 0),
    // 1024 x 4 tiles (n = 2^20).  The second pass needs 44 registers: its 60-register form with the register prefetch still runs at 8 waves (9.03 ->
    // 8.85 ms per proof); the first pass with the prefetch spills (12.0 -> 12.3 ms) and stays without
    NTT_INSTANCE(false, ntt_pass_a, 1024, 8, false, 10, 2, 0), NTT_INSTANCE(true, ntt_pass_b, 1024, 8, true, 10, 2, 0),
    // 256 x 16 tiles (n = 2^16, the first two passes of three-pass plans)
    NTT_INSTANCE(false, ntt_pass_a, 1024, 8, false, 8, 4, 0), NTT_INSTANCE(true, ntt_pass_b, 1024, 8, false, 8, 4, 0),
    NTT_INSTANCE(false, ntt_pass_a, 512, 4, true, 8, 4, 0),   NTT_INSTANCE(true, ntt_pass_b, 512, 4, true, 8, 4, 0),
    // register pre-stage (NttArgs::pre): the 1024 x 4 shape of n = 2^21 / 2^22 compiled for the shape, any other shape (tests) from the arguments
    NTT_INSTANCE(false, ntt_pass_a, 1024, 8, false, 10, 2, 1), NTT_INSTANCE(true, ntt_pass_b, 1024, 8, false, 10, 2, 1),
    NTT_INSTANCE(false, ntt_pass_a, 512, 4, true, 0, 0, 1),   NTT_INSTANCE(true, ntt_pass_b, 512, 4, true, 0, 0, 1),
};
struct NttRegInstance { int log_len, log_t, threads; void (*kernel)(NttRegArgs); };
#define NTT_REG_INSTANCE(L) {L, NttDigits<L>::log_t, (1 << (L + NttDigits<L>::log_t)) / 16, ntt_reg_kernel<L>}
static const NttRegInstance NTT_REG_INSTANCES[] = {NTT_REG_INSTANCE(6), NTT_REG_INSTANCE(7), NTT_REG_INSTANCE(8), NTT_REG_INSTANCE(9), NTT_REG_INSTANCE(10), NTT_REG_INSTANCE(11), NTT_REG_INSTANCE(12)};

// the DISTAFF_NTT_* switches (ctx.h DST_SWITCHES) as the plan reads them, parsed once
struct NttSwitches {
    enum Force { NONE, OTHER, PRE, PRE_A, THREE, REG, LDS } force = NONE;   // DISTAFF_NTT (OTHER: set to something else -- no plan family forced, but not the default either)
    unsigned shape_a = 0, shape_b = 0;     // DISTAFF_NTT_SHAPE
    int waves = 0;                         // DISTAFF_NTT_WAVES: 0 unset, else 4 / 8
    int dif = -1;                          // DISTAFF_NTT_DIF: -1 unset, else the first-pass mode it forces
    bool any_shape = false, coset_slow = false;   // DISTAFF_NTT_FIXED=0, DISTAFF_NTT_ORDER=0
    bool row_major = false;                // DISTAFF_NTT=row: the default plan with the row-major layout where it would be tile-major (tests)
    uint32_t debug = 0;                    // DISTAFF_NTT_DEBUG
};
static NttSwitches ntt_switches(const dst_ctx* c) {
    NttSwitches s;
    if (c->sw_is("DISTAFF_NTT", "row")) s.row_major = true;
    else if (const char* e = c->sw("DISTAFF_NTT")) s.force = !strcmp(e, "pre") ? s.PRE : !strcmp(e, "pre_a") ? s.PRE_A : !strcmp(e, "3pass") ? s.THREE : !strcmp(e, "reg") ? s.REG : !strcmp(e, "lds") ? s.LDS : s.OTHER;
    if (const char* e = c->sw("DISTAFF_NTT_SHAPE")) if (sscanf(e, "%u,%u", &s.shape_a, &s.shape_b) != 2) s.shape_a = s.shape_b = 0;
    if (const char* e = c->sw("DISTAFF_NTT_WAVES")) s.waves = e[0] == '8' ? 8 : 4;
    if (const char* e = c->sw("DISTAFF_NTT_DIF")) s.dif = e[0] == '0' ? 1 : e[0] == '2' ? 2 : 0;
    s.any_shape = c->sw_is("DISTAFF_NTT_FIXED", "0");
    if (const char* e = c->sw("DISTAFF_NTT_ORDER")) s.coset_slow = e[0] == '0';
    if (const char* e = c->sw("DISTAFF_NTT_DEBUG")) s.debug = (uint32_t)atoi(e);
    return s;
}

// two workgroups of 512 lanes per CU while tile + twiddles fit 80 KiB, else one of 1024 lanes (same waves per SIMD)
#define NTT_LDS_TWO_PER_CU (80 * 1024)
// The LDS-family instance of a pass.  1024-point tiles (five LDS rounds per tile): two workgroups of 1024 lanes = 8 waves per SIMD, 64 registers, no
// register prefetch -- the other workgroup's rounds cover a workgroup's loads (measured 20.2 against 20.55 ms of extension per 2^20 proof, same box);
// shorter tiles stay with 512 lanes + prefetch (2^16: 0.96 against 1.03 ms).  DISTAFF_NTT_WAVES=4|8 forces one (the tests run both).  A shape-compiled
// instance where there is one for the lanes chosen, unless DISTAFF_NTT_FIXED=0; a pre-stage pass has its own instances and ignores the lanes.
static const NttInstance* ntt_select(bool pass_b, uint32_t log_len, uint32_t log_tile, uint32_t pre, size_t lds, const NttSwitches& sw) {
    const bool two = lds <= NTT_LDS_TWO_PER_CU, eight = two && (sw.waves ? sw.waves == 8 : log_len >= 10);
    const bool fixed = log_len == 10 && log_tile == 2 && !sw.any_shape, fixed84 = log_len == 8 && log_tile == 4 && !sw.any_shape;
    const bool wide8 = pre ? fixed : eight, shaped = pre ? fixed : two && ((eight && fixed) || fixed84);
    const int threads = (wide8 || (!pre && !two)) ? 1024 : 512, wpe = wide8 ? 8 : 4, len = shaped ? (int)log_len : 0, t = shaped ? (int)log_tile : 0;
    for (const NttInstance& r : NTT_INSTANCES)
        if (r.pass_b == pass_b && r.threads == threads && r.wpe == wpe && r.log_len == len && r.log_t == t && r.pre == (int)pre) return &r;
    return nullptr;
}
// First pass of an extension: coset DIT (the pre-scale costs nothing, but the workgroup holds n1 - 1 twiddle pairs of ITS coset) while
// tile + pairs fit the 80 KiB that let two workgroups share a CU; otherwise pre-scale + DIF with the n1/2 shared stage twiddles (one
// more multiplication per element, two workgroups per CU: measured 14.5 against 15.0 ms per proof for the 1024-point tiles of n = 2^20).
// DISTAFF_NTT_DIF=1 / 0 forces one or the other (the tests run both).
// returns 0: pre-scale + DIF, 1: coset DIT with the whole table in LDS, 2: coset DIT whose last-stage twiddles (half of the table) are read
// from global memory (tile + the other half fit 80 KiB)
static uint32_t ntt_first_pass_mode(const NttSwitches& sw, size_t n1, size_t tile) {
    if (sw.dif >= 0) return (uint32_t)sw.dif;
    if (n1 * tile * sizeof(fe) + n1 * sizeof(fe_tw) <= NTT_LDS_TWO_PER_CU) return 1;
    if (n1 * tile * sizeof(fe) + (n1 / 2) * sizeof(fe_tw) <= NTT_LDS_TWO_PER_CU) return 2;
    return 0;
}

// The ONE place that decides the layout of the staging array and of the four-step tables (NttPlan::tile_major -> NttArgs::tile_major): tile-major for two-pass plans of
// the LDS family whose tiles are four columns wide in both passes and whose second pass has no register pre-stage (n = 2^4 .. 2^21; a pre-stage
// in the first pass alone, n = 2^21, is included).  Three-pass plans (16-column tiles: 256-byte segments as they are), the register-radix family,
// tiles of one or two columns and n = 2^22 (measured slower, NttArgs) keep the row-major layout.
static bool ntt_tile_major(const NttPlan& pl) {
    return pl.count == 2 && !pl.pass[0].reg && !pl.first_lde.reg && !pl.pass[1].reg && pl.pass[0].log_tile == 2 && pl.first_lde.log_tile == 2 && pl.pass[1].log_tile == 2
           && !pl.pass[1].pre;
}
// The plan, a pure function of the transform length and the switches.  n = n1 * n2 in two HBM passes, tiles bounded by 64 KiB of LDS; from n = 2^21
// (measured cross-over) three passes n = n1 * nm * n3 with 16-column tiles (256-byte HBM segments) instead of 4096-point tiles that hold one or two
// columns -- except n = 2^21, 2^22: still two passes, their 2048-point factors run as a register pre-stage + 1024-point LDS tiles (NttArgs::pre).
// DISTAFF_NTT=pre forces the pre-stages onto smaller transforms (tests; pre_a: onto the first pass only), DISTAFF_NTT=3pass the three-pass plan from 2^12 on.
static NttPlan ntt_plan_derive(uint32_t log_n, const NttSwitches& sw) {
    NttPlan pl;
    const bool force_pre = sw.force == sw.PRE && log_n >= 10 && log_n <= 22;
    const bool force_pre_a = sw.force == sw.PRE_A && log_n >= 10 && log_n <= 21;      // a pre-stage in the first pass only, as n = 2^21 has by itself
    const bool pre_plan = force_pre || force_pre_a || ((log_n == 21 || log_n == 22) && sw.force == sw.NONE);
    const bool three = !pre_plan && ((log_n >= 21 && sw.force != sw.REG && sw.force != sw.LDS) || (sw.force == sw.THREE && log_n >= 12));
    uint32_t pre_a = 0, pre_b = 0;
    if (three) {
        // shape n1 * nm * n3 with n1 >= nm >= n3 as balanced as possible, at most 2^8 each; DISTAFF_NTT_SHAPE=a,b overrides n1, nm (tests)
        uint32_t a = (log_n + 2) / 3, b = (log_n - a + 1) / 2;
        if (a > 8) { a = 8; b = 8; }
        const unsigned x = sw.shape_a, y = sw.shape_b;
        if (x >= 4 && y >= 4 && x <= 8 && y <= 8 && x + y + 4 <= log_n && log_n - x - y <= 8) { a = x; b = y; }
        pl.log_n1 = a; pl.log_n2 = log_n - a; pl.log_n3 = log_n - a - b;
    }
    else { pl.log_n1 = (log_n + 1) / 2; pl.log_n2 = log_n / 2; }
    if (pre_plan) { pre_a = (force_pre || force_pre_a || pl.log_n1 > 10) ? 1u : 0u; pre_b = (force_pre || pl.log_n2 > 10) ? 1u : 0u; }
    // kernel family per pass (measured): the LDS radix-2 kernels win while a tile holds >= 2 columns in 64 KiB of LDS; the
    // register-radix kernels take over for 4096-point tiles.  DISTAFF_NTT=reg|lds forces one two-pass family (tests run both); a 4096-point
    // coset DIT (64 KiB tile + 128 KiB of twiddle pairs) does not fit LDS, so `lds` leaves those to the register family
    const bool reg_ok = !three && !pre_plan && pl.log_n2 >= 6 && pl.log_n1 <= 12, reg_all = reg_ok && sw.force == sw.REG;
    const bool reg_a = reg_ok && (pl.log_n1 >= 12 || reg_all), reg_b = reg_ok && (pl.log_n2 >= 12 || reg_all);
    // a pass: `cap` columns per tile while the tile fits 64 KiB and the other dimension has that many
    auto pass = [&](NttKind kind, uint32_t log_len, uint32_t other_len_log, uint32_t cap, uint32_t pre, bool reg, bool lde) {
        NttPass P;
        uint32_t t = cap;
        while (t > 1 && (((size_t)1 << log_len) * t * sizeof(fe) > 65536 || t > (1u << other_len_log))) t >>= 1;
        P.kind = kind; P.log_len = log_len; P.log_tile = (uint32_t)__builtin_ctz(t); P.pre = pre;
        const size_t len = (size_t)1 << log_len;
        if (lde && !reg) { P.dit = ntt_first_pass_mode(sw, len, t); if (pre && P.dit == 0) P.dit = 2; }   // the pre-stage is written for the coset DIT (tiles of at most 1024 x 4: always fits)
        P.lds = len * t * sizeof(fe) + (P.dit == 1 ? len : len / 2) * sizeof(fe_tw);
        if (reg) { for (const NttRegInstance& r : NTT_REG_INSTANCES) if (r.log_len == (int)log_len) P.reg = &r; }
        else P.inst = ntt_select(kind == NTT_LAST, log_len, P.log_tile, pre, P.lds, sw);
        return P;
    };
    const uint32_t cap = three ? 16 : 4;
    pl.pass[0] = pass(NTT_FIRST, pl.log_n1 - pre_a, pl.log_n2, cap, pre_a, reg_a, false);
    pl.first_lde = pass(NTT_FIRST, pl.log_n1 - pre_a, pl.log_n2, cap, pre_a, reg_a, true);
    if (three) pl.pass[1] = pass(NTT_MIDDLE, pl.log_n2 - pl.log_n3, pl.log_n3, cap, 0, false, false);
    pl.pass[three ? 2 : 1] = three ? pass(NTT_LAST, pl.log_n3, pl.log_n1, cap, 0, false, false) : pass(NTT_LAST, pl.log_n2 - pre_b, pl.log_n1, cap, pre_b, reg_b, false);
    pl.count = three ? 3 : 2; pl.coset_slow = sw.coset_slow; pl.debug = sw.debug;
    pl.tile_major = ntt_tile_major(pl) && !sw.row_major;
    // the coefficient copy in tile order: its writer is the interpolation's second pass, its reader the extension's first; neither may have a pre-stage
    // (a pre-stage first pass reads the rows m and m + len of a column: two blocks, nothing gained -- profiles/ntt_tile_major.md on the same shape of store)
    pl.coeff_tile_major = NTT_COEFF_TILE_MAJOR && pl.tile_major && !pl.first_lde.pre && !pl.pass[1].pre;
    return pl;
}
static int ntt_plan_set(dst_ctx* c) {                 // c->plan from the context's size and switches; every pass must have found its compiled instance
    NttPlan& pl = c->plan = ntt_plan_derive(c->log_n, ntt_switches(c));
    for (uint32_t i = 0; i < 2 * pl.count; i++)
        if (!pl.at(i % pl.count, i >= pl.count).inst && !pl.at(i % pl.count, i >= pl.count).reg) { c->err = "transform plan: no compiled instance for pass " + std::to_string(i % pl.count); return DST_ERR_STATE; }
    return DST_OK;
}

// tiles a workgroup walks through: as many as keep >= 2048 workgroups in the launch (8 per CU), at most 8
static uint32_t ntt_tiles_per_block(uint32_t tiles, size_t arrays) {
    uint32_t k = 1;
    while (k < 8 && tiles % (2 * k) == 0 && (size_t)(tiles / (2 * k)) * arrays >= 2048) k *= 2;
    return k;
}
// DISTAFF_NTT_DEBUG=1 prints, once per distinct launch shape, how many workgroups of the instance that runs are resident per CU
static void ntt_report_occupancy(const char* name, const NttInstance& I, size_t lds) {
    static std::mutex mu;
    static std::map<std::string, bool> seen;
    char key[128]; snprintf(key, sizeof key, "%s/%d/%d/%d/%d/%d/%zu", name, I.threads, I.wpe, I.log_len, I.log_t, I.pre, lds);
    std::lock_guard<std::mutex> lock(mu);
    if (seen[key]) return; seen[key] = true;
    int nb = -1;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, I.kernel, I.threads, lds);
    fprintf(stderr, "[distaff] %s<%d,%d,%d,%d,%d,%d>: %d lanes, %zu B LDS -> %d workgroups per CU (%s)\n", name, I.threads, I.wpe, (int)I.prefetch, I.log_len, I.log_t, I.pre, I.threads, lds, nb, hipGetErrorString(e));
}

// strides in elements.  src_tile_major / dst_tm: the coefficient copy in tile order (NttArgs) as the source of an extension's first pass / as the second
// destination of an interpolation's last pass; the passes in between never see either
struct NttIo { const fe* src; size_t src_col_stride, src_coset_stride; fe* dst; size_t dst_col_stride, dst_coset_stride; bool src_tile_major = false; fe* dst_tm = nullptr; };

// One pass of a transform over `cosets` x `cols` arrays: the kernel arguments from the pass description, then the launch -- or, with `describe`, a
// line about the launch instead of it (dst_ntt_describe).  Two-pass plans (n = n1 * n2): the first pass runs the n1-point transforms over the
// stride-n2 dimension, the last the n2-point transforms over the contiguous one, natural-order output.  Three-pass plans (n = n1 * nm * n3):
//   first  (shape n1 x n/n1): as in a two-pass plan (coset pre-scale, twiddle w_N^(m'*(B*k1+j)));
//   middle (ntt_pass_a, shape nm x n3 on each of the cosets * n1 rows of n/n1 points): twiddle w_{n/n1}^(k2*m3);
//   last   (n3 points, tile = adjacent k1, one batch per k2): natural-order store at k1 + n1*(k2 + nm*k3).
static void ntt_run_pass(dst_ctx* c, const NttPass& P, const NttIo& io, size_t cosets, size_t cols, bool inverse, bool lde, uint32_t skip, std::string* describe) {
    const NttPlan& p = c->plan;
    const bool first = P.kind == NTT_FIRST, last = P.kind == NTT_LAST;
    const size_t n = c->n, n1 = (size_t)1 << p.log_n1, nrow = (size_t)1 << p.log_n2;
    const char* name = first ? "ntt_pass_a" : last ? "ntt_pass_b" : "ntt_pass_mid";
    double bytes = 16.0 * n * cols * ((first && lde) ? 1 + cosets : 2 * cosets);           // an extension reads its coefficients once for all cosets
    const uint32_t j0 = lde ? (uint32_t)c->j0 + skip : 0u, has_scale = (last && inverse) ? 1u : 0u;   // 1/n leaves with the last pass
    char line[384];
    if (P.reg) {
        const NttRegInstance& R = *P.reg;
        NttRegArgs a{};
        a.log_N = c->log_N; a.log_b = c->log_b; a.lo_bits = c->tw_lo_bits; a.j0 = j0; a.coset_twiddle = lde ? 1u : 0u;
        for (int j = 0; j < 8; j++) a.c16[j] = inverse ? c->c16i[j] : c->c16f[j];
        a.src = io.src; a.src_col_stride = io.src_col_stride; a.src_coset_stride = io.src_coset_stride;
        a.dst = io.dst; a.dst_col_stride = io.dst_col_stride; a.dst_coset_stride = io.dst_coset_stride;
        a.scale = c->n_inv; a.has_scale = has_scale; a.stage_tw = P.stage_tw[inverse];
        if (first) {
            a.in_stride_m = nrow; a.in_stride_t = 1; a.out_stride_k = nrow;
            a.tw_lo = inverse ? c->itw_lo : c->tw_lo; a.tw_hi = inverse ? c->itw_hi : c->tw_hi;
            a.prescale = lde ? c->prescale : nullptr;
        } else { a.in_stride_m = 1; a.in_stride_t = nrow; a.out_stride_k = n1; }
        const dim3 g((unsigned)((first ? nrow : n1) >> R.log_t), (unsigned)cosets, (unsigned)cols);
        if (describe) {
            snprintf(line, sizeof line, "%s reg LOGL=%d block=%d grid=%ux%ux%u lds=0 dit=0 pre=0 log_len=%d log_tile=%d tiles_per_block=1 coset_fast=0 has_scale=%u bytes=%.0f mads=0\n",
                     name, R.log_len, R.threads, g.x, g.y, g.z, R.log_len, R.log_t, has_scale, bytes);
            *describe += line; return;
        }
        KScope ks_(c, name, bytes, true);
        hipLaunchKernelGGL(R.kernel, g, dim3(R.threads), 0, c->stream, a);
        return;
    }
    NttArgs a{};
    a.log_N = c->log_N; a.log_b = c->log_b; a.scale = c->n_inv_tw; a.has_scale = has_scale; a.debug = p.debug;
    a.src = io.src; a.src_col_stride = io.src_col_stride; a.src_coset_stride = io.src_coset_stride;
    a.dst = io.dst; a.dst_col_stride = io.dst_col_stride; a.dst_coset_stride = io.dst_coset_stride;
    a.stage_tw = P.stage_tw[inverse]; a.tile = P.log_tile; a.pre = P.pre; a.pre_tw = P.pre_tw[inverse];
    a.log_n1 = p.log_n1; a.log_n2 = p.log_n2;
    a.tile_major = p.tile_major ? 1u : 0u;
    // the plan keeps the copy (ntt_plan_derive: four-column tiles, no pre-stage in either pass concerned), or the caller has none to offer
    a.src_tile_major = (first && lde && io.src_tile_major && p.coeff_tile_major) ? 1u : 0u;
    a.dst_tm = (last && inverse && !lde && p.coeff_tile_major) ? io.dst_tm : nullptr;
    if (a.dst_tm) bytes += 16.0 * n * cols;            // the second store
    size_t units = cosets;             // what the coset dimension of the block index runs over
    uint32_t tiles, batch_log = 0;     // tiles of an array; three-pass last pass: one batch of tile groups per middle frequency
    if (first) {
        a.log_n1 = P.log_len; a.j0 = j0;
        a.prescale = lde ? c->prescale : nullptr;
        a.dit = P.dit ? 1u : 0u; a.dit_last = P.dit == 2 ? c->dit_last : nullptr;
        a.tw4 = !lde ? P.tw4[inverse] : describe ? nullptr : c->tw4_lde + (size_t)skip * n; a.tw4_coset_stride = lde ? n : 0;
        tiles = (uint32_t)(nrow >> P.log_tile);
    } else if (!last) {                // every (coset, k1) row of nrow points is an array of its own
        a.log_n1 = P.log_len; a.log_n2 = p.log_n3; a.tw4 = P.tw4[inverse];
        a.src_coset_stride = a.dst_coset_stride = nrow; units = cosets * n1;
        tiles = (1u << p.log_n3) >> P.log_tile;
    } else {
        a.log_n2 = P.log_len;
        a.src_row_stride = nrow; a.dst_k_stride = n1;
        if (p.log_n3) { batch_log = p.log_n2 - p.log_n3; a.src_batch_stride = (size_t)1 << p.log_n3; a.dst_k_stride = n1 << batch_log; a.dst_batch_stride = n1; }
        a.batch_log = batch_log;
        tiles = (uint32_t)(n1 >> P.log_tile);
    }
    const uint32_t spread = P.pre + batch_log;         // a pre-stage pass has two tile groups per tile (one per half of the frequencies), a batched one a group per batch
    a.tiles_per_block = ntt_tiles_per_block(tiles, (units * cols) << spread);
    const size_t groups = (size_t)(tiles / a.tiles_per_block) << spread;
    // Block order of a first pass over several cosets (ntt_block): every (coset, register) of a tile group before the next group, so that the
    // coefficient tiles (the same for every coset) and the four-step twiddles (the same for every register) are re-read while they are still
    // in the XCD's L2: FETCH_SIZE of the 2^20 launches 1.29 against 1.57 GB, time unchanged.  DISTAFF_NTT_ORDER=0: coset-slow order (tests).
    a.coset_fast = (first && cosets > 1 && groups % 8 == 0 && !p.coset_slow) ? 1u : 0u;
    a.groups = (uint32_t)groups; a.cosets = (uint32_t)units; a.cols = (uint32_t)cols;
    // multiply-adds of the launch: 18 per table-pair multiplication (fe_mul_tw); multiplications per element: every DIT stage 1/2, DIF
    // two-stage rounds 1 each except the last (1/4: the distance-1 stage has no twiddles), plus four-step twiddle / pre-scale / 1/n
    const uint32_t stages = P.log_len;
    double mults = a.dit ? 0.5 * stages : ((stages & 1u) ? 0.5 * (stages - 1) : (stages >= 2 ? 0.5 * stages - 0.75 : 0.0));
    if (!last) mults += ((first && lde && !a.dit) ? 1.0 : 0.0) + (NTT_TW4_PAIRS ? 1.0 : 21.0 / 18.0); else if (has_scale) mults += 1.0;     // the four-step product: 18 or 21 mads
    if (P.pre) mults += a.dit ? 1.0 : 0.5;             // register pre-stage: c * x[m + len] in both halves of a coset DIT, the twiddle of the odd half otherwise
    const double elements = (double)groups * a.tiles_per_block * ((size_t)1 << a.tile) * ((size_t)1 << stages) * units * cols;
    const NttInstance& I = *P.inst;
    const unsigned grid = (unsigned)(groups * units * cols);
    if (describe) {
        snprintf(line, sizeof line, "%s lds %c<%d,%d,%d,%d,%d,%d> block=%d grid=%u lds=%zu dit=%u pre=%u log_len=%u log_tile=%u tiles_per_block=%u coset_fast=%u has_scale=%u bytes=%.0f mads=%.0f\n",
                 name, I.pass_b ? 'b' : 'a', I.threads, I.wpe, (int)I.prefetch, I.log_len, I.log_t, I.pre, I.threads, grid, P.lds, P.dit, P.pre, P.log_len, P.log_tile,
                 a.tiles_per_block, a.coset_fast, has_scale, bytes, 18.0 * mults * elements);
        *describe += line; return;
    }
    KScope ks_(c, name, bytes, true, 18.0 * mults * elements);
    if (a.debug & 1u) ntt_report_occupancy(name, I, P.lds);
    hipLaunchKernelGGL(I.kernel, dim3(grid), dim3(I.threads), P.lds, c->stream, a, a.src, a.dst);
}

// A whole transform: the plan's passes in turn, through the staging buffers [column][coset][n] between them.
// skip: number of leading local cosets left out (their outputs are produced elsewhere); io.dst points at the first coset computed
static void ntt_transform(dst_ctx* c, const NttIo& io, size_t cosets, size_t cols, bool inverse, bool lde, uint32_t skip = 0, std::string* describe = nullptr) {
    const NttPlan& p = c->plan;
    fe* const stage[2] = {c->tmp, c->tmp2};
    for (uint32_t i = 0; i < p.count; i++) {
        NttIo s = io;
        if (i > 0) { s.src = stage[i - 1]; s.src_col_stride = c->n * cosets; s.src_coset_stride = c->n; s.src_tile_major = false; }
        if (i + 1 < p.count) { s.dst = stage[i]; s.dst_col_stride = c->n * cosets; s.dst_coset_stride = c->n; s.dst_tm = nullptr; }
        ntt_run_pass(c, p.at(i, lde), s, cosets, cols, inverse, lde, skip, describe);
    }
}

// ---- four-step twiddle tables -------------------------------------------------------------------------------------------------------
// out[coset][k1][m2] = w_N^(m2 * ((k1 << log_b) + j)) for a transform of 2^log_n points whose inner dimension has 2^log_n2 points;
// a sub-transform of length n' = n / 2^s is expressed with log_b + s (its root is w_N^(B * 2^s)).  tile_major: the same values as
// out[coset][m2 >> 2][k1][m2 & 3] (NttArgs::tile_major)
__global__ void twiddle_table_kernel(tw4_t* out, const fe* tw_lo, const fe* tw_hi, uint32_t lo_bits, uint32_t log_n2, uint32_t log_n, uint32_t log_b,
                                     uint32_t log_N, uint32_t j0, uint32_t coset_twiddle, uint32_t tile_major) {
    const size_t n = (size_t)1 << log_n;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t log_n1 = log_n - log_n2;
    const uint64_t k1 = tile_major ? (i >> 2) & (((size_t)1 << log_n1) - 1) : i >> log_n2;
    const uint64_t m2 = tile_major ? ((i >> (log_n1 + 2)) << 2) + (i & 3) : i & (((size_t)1 << log_n2) - 1);
    const uint64_t jg = coset_twiddle ? j0 + blockIdx.y : 0;
    const uint64_t e = (m2 * ((k1 << log_b) + jg)) & (((uint64_t)1 << log_N) - 1);
#if NTT_TW4_PAIRS
    out[(size_t)blockIdx.y * n + i] = fe_tw_make(dom_pow(tw_lo, tw_hi, lo_bits, e));
#else
    out[(size_t)blockIdx.y * n + i] = dom_pow(tw_lo, tw_hi, lo_bits, e);
#endif
}
// Context creation: the plan, the LDS limits of its kernels and every table the passes read.  The tables stay the context's (ctx.h); the
// pass descriptions hold views of them.
int k_ntt_init(dst_ctx* c) {
    int r = ntt_plan_set(c);
    if (r) return r;
    NttPlan& pl = c->plan;
    {   // tile + stage twiddles exceed the 64 KiB default.  Contexts of several ranks may run as threads of one process
        // (dst_prove_sharded_local): the once-per-device marks are guarded
        static std::mutex mu;
        static bool raised[64] = {};
        std::lock_guard<std::mutex> lock(mu);
        if (c->device >= 0 && c->device < 64 && !raised[c->device]) {
            for (const NttInstance& I : NTT_INSTANCES) HIP_TRY(c, hipFuncSetAttribute((const void*)I.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            raised[c->device] = true;
        }
    }
    {
        const fe w16 = h_root_of_unity(4);
        const std::vector<fe> f = h_powers(w16, 8), b = h_powers(h_inv(w16), 8);
        for (int j = 0; j < 8; j++) { c->c16f[j] = f[j]; c->c16i[j] = b[j]; }
    }
    for (uint32_t i = 0; i < pl.count; i++) {
        NttPass& P = pl.pass[i];
        const fe w = h_root_of_unity(P.log_len), wp = h_root_of_unity(P.log_len + 1);
        for (int inv = 0; inv < 2; inv++) {
            if ((r = dev_upload(c, &c->ntt_stage_tw[i][inv], h_powers_tw(inv ? h_inv(w) : w, (size_t)1 << (P.log_len - 1))))) return r;
            if (P.pre && (r = dev_upload(c, &c->ntt_pre_tw[i][inv], h_powers_tw(inv ? h_inv(wp) : wp, (size_t)1 << P.log_len)))) return r;
            P.stage_tw[inv] = c->ntt_stage_tw[i][inv]; P.pre_tw[inv] = c->ntt_pre_tw[i][inv];
        }
    }
    {
        const std::vector<fe_tw> pre = h_powers_tw(h_root_of_unity(c->log_b + pl.log_n1), (size_t)1 << (c->log_b + pl.log_n1));
        if ((r = dev_upload(c, &c->prescale, pre))) return r;
        // last-stage twiddles of the (half-length, with a pre-stage) coset DITs: [B][R][len / 2] entries pre[j + B * (h + R * k)]
        const size_t R = (size_t)1 << pl.pass[0].pre, half = (size_t)1 << (pl.pass[0].log_len - 1);
        std::vector<fe_tw> last(c->B * R * half);
        for (size_t j = 0; j < c->B; j++) for (size_t h = 0; h < R; h++) for (size_t k = 0; k < half; k++) last[(j * R + h) * half + k] = pre[j + c->B * (h + R * k)];
        if ((r = dev_upload(c, &c->dit_last, last))) return r;
    }
    if ((r = dev_alloc(c, &c->tw4_lde, c->Bc * c->n))) return r;
    if ((r = dev_alloc(c, &c->tw4_fwd, c->n))) return r;
    if ((r = dev_alloc(c, &c->tw4_inv, c->n))) return r;
    pl.pass[0].tw4[0] = c->tw4_fwd; pl.pass[0].tw4[1] = c->tw4_inv;
    dim3 g((unsigned)((c->n + 255) / 256), (unsigned)c->Bc);
    const uint32_t tm = pl.tile_major ? 1u : 0u;
    hipLaunchKernelGGL(twiddle_table_kernel, g, dim3(256), 0, c->stream, c->tw4_lde, c->tw_lo, c->tw_hi, c->tw_lo_bits, pl.log_n2, c->log_n, c->log_b, c->log_N, (uint32_t)c->j0, 1u, tm);
    g.y = 1;
    hipLaunchKernelGGL(twiddle_table_kernel, g, dim3(256), 0, c->stream, c->tw4_fwd, c->tw_lo, c->tw_hi, c->tw_lo_bits, pl.log_n2, c->log_n, c->log_b, c->log_N, 0u, 0u, tm);
    hipLaunchKernelGGL(twiddle_table_kernel, g, dim3(256), 0, c->stream, c->tw4_inv, c->itw_lo, c->itw_hi, c->tw_lo_bits, pl.log_n2, c->log_n, c->log_b, c->log_N, 0u, 0u, tm);
    if (pl.count == 3) {  // middle pass of a three-pass plan: rows of n' = n2 points, w_{n'}^(k2*m3) = w_N^(m3 * (k2 << (log_b + log_n1)))
        if ((r = dev_alloc(c, &c->tw4_row_fwd, (size_t)1 << pl.log_n2))) return r;
        if ((r = dev_alloc(c, &c->tw4_row_inv, (size_t)1 << pl.log_n2))) return r;
        pl.pass[1].tw4[0] = c->tw4_row_fwd; pl.pass[1].tw4[1] = c->tw4_row_inv;
        dim3 gr((unsigned)((((size_t)1 << pl.log_n2) + 255) / 256), 1u);
        hipLaunchKernelGGL(twiddle_table_kernel, gr, dim3(256), 0, c->stream, c->tw4_row_fwd, c->tw_lo, c->tw_hi, c->tw_lo_bits, pl.log_n3, pl.log_n2, c->log_b + pl.log_n1, c->log_N, 0u, 0u, 0u);
        hipLaunchKernelGGL(twiddle_table_kernel, gr, dim3(256), 0, c->stream, c->tw4_row_inv, c->itw_lo, c->itw_hi, c->tw_lo_bits, pl.log_n3, pl.log_n2, c->log_b + pl.log_n1, c->log_N, 0u, 0u, 0u);
    }
    for (int inv = 0; inv < 2; inv++) { pl.first_lde.stage_tw[inv] = pl.pass[0].stage_tw[inv]; pl.first_lde.pre_tw[inv] = pl.pass[0].pre_tw[inv]; }   // its four-step table is tw4_lde
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return DST_OK;
}

#if DST_TEST_HOOKS
// Test build only: the launches a transform of this size and shape would make under the current DISTAFF_NTT_* switches, one line each.  The plan comes
// from ntt_plan_derive and the lines from ntt_run_pass itself with launching turned off; no device is touched and nothing is allocated.
extern "C" __attribute__((visibility("default"))) int dst_ntt_describe(uint32_t log_n, uint32_t log_blowup, int inverse, int lde, uint32_t cosets, uint32_t cols, uint32_t skip, char* out, size_t cap) {
    if (!out || log_n < 4 || log_n > 24 || log_blowup < 4 || log_blowup > 8 || !cosets || !cols) return DST_ERR_ARG;
    dst_ctx c;
    c.read_switches();
    c.log_n = log_n; c.log_b = log_blowup; c.log_N = log_n + log_blowup;
    c.n = (size_t)1 << log_n; c.B = c.Bc = (size_t)1 << log_blowup; c.N = c.n * c.B;
    if (int r = ntt_plan_set(&c)) return r;
    std::string text;
    ntt_transform(&c, NttIo{}, cosets, cols, inverse != 0, lde != 0, skip, &text);
    if (text.size() + 1 > cap) return DST_ERR_ARG;
    memcpy(out, text.c_str(), text.size() + 1);
    return DST_OK;
}
#endif

// how many (coset x column) size-n arrays fit in c->tmp
static size_t tmp_capacity_arrays(const dst_ctx* c) { return c->Bc * c->tmp_regs; }

void k_intt_columns(dst_ctx* c, const fe* src, size_t src_stride, fe* dst, size_t ncols, fe* dst_tm) {
    size_t cap = tmp_capacity_arrays(c);
    for (size_t done = 0; done < ncols;) {
        size_t cols = ncols - done < cap ? ncols - done : cap;
        ntt_transform(c, {src + done * src_stride, src_stride, 0, dst + done * c->n, c->n, 0, false, dst_tm ? dst_tm + done * c->n : nullptr}, 1, cols, true, false);
        done += cols;
    }
}

void k_lde_columns(dst_ctx* c, const fe* polys, fe* lde, size_t ncols, const fe* polys_tm) {
    // coset 0 of the extension is the trace itself (T(w_n^k) for the interpolant T): when this rank owns it and the polynomials are
    // the interpolated trace, it is copied instead of transformed (1/B of the extension work)
    const bool of_trace = polys >= c->polys && polys < c->polys + c->W * c->n;          // a group of the interpolated trace registers
    const uint32_t skip = (c->j0 == 0 && of_trace && c->Bc > 1 && !c->trace_owned_only) ? 1u : 0u;      // owned-only: this rank holds 1/world of the trace registers, coset 0 is transformed like the others
    if (skip && c->trace != c->lde)         // a context that owns coset 0 normally keeps the trace in those slots already (ctx.h: trace_stride)
        (void)hipMemcpy2DAsync(lde, c->Bc * c->n * sizeof(fe), c->trace + ((polys - c->polys) / c->n) * c->trace_stride, c->trace_stride * sizeof(fe), c->n * sizeof(fe), ncols, hipMemcpyDeviceToDevice, c->stream);
    // launch granularity: `bcols` registers x `bcos` cosets per pair of passes (the staging buffer holds tmp_capacity_arrays arrays)
    size_t bcols = tmp_capacity_arrays(c) / c->Bc, bcos = c->Bc - skip;
    if (const char* e = c->sw("DISTAFF_LDE_BATCH")) { unsigned x = 0, y = 0; if (sscanf(e, "%u,%u", &x, &y) == 2 && x >= 1 && y >= 1 && (size_t)x * y <= tmp_capacity_arrays(c)) { bcols = x; bcos = y; } }
    for (size_t done = 0; done < ncols;) {
        const size_t cols = ncols - done < bcols ? ncols - done : bcols;
        for (size_t s = skip; s < c->Bc;) {
            const size_t cc = c->Bc - s < bcos ? c->Bc - s : bcos;
            const bool tm = polys_tm != nullptr && c->plan.coeff_tile_major;
            ntt_transform(c, {(tm ? polys_tm : polys) + done * c->n, c->n, 0, lde + done * c->Bc * c->n + s * c->n, c->Bc * c->n, c->n, tm}, cc, cols, false, true, (uint32_t)s);
            s += cc;
        }
        done += cols;
    }
}

// ---- 8n coefficients -> coset-major evaluations -------------------------------------------------------------------------
// d_j[m0] = w_N^(j*m0) * sum_{m1<8} c[m0 + n*m1] * w_B^(j*m1); followed by a plain size-n NTT per coset.
// one lane per m0 walks through all local cosets: the eight coefficients are read once, the factors w_B^(j*m1) of every coset come
// from LDS, and w_N^(j*m0) advances by one multiplication per coset
__global__ void __launch_bounds__(256) fold8_kernel(const fe* __restrict__ poly, fe* __restrict__ out, const fe* tw_lo, const fe* tw_hi, uint32_t lo_bits,
                                                    uint32_t log_n, uint32_t log_N, uint32_t j0, uint32_t cosets) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fold_smem[];
    fe* cj = reinterpret_cast<fe*>(fold_smem);                      // [cosets][8]
    const size_t n = (size_t)1 << log_n;
    const uint64_t nmask = ((uint64_t)1 << log_N) - 1;
    for (uint32_t i = threadIdx.x; i < cosets * 8; i += blockDim.x)
        cj[i] = dom_pow(tw_lo, tw_hi, lo_bits, ((uint64_t)(j0 + (i >> 3)) * (i & 7) << log_n) & nmask);
    __syncthreads();
    const size_t m0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m0 >= n) return;
    fe c[8];
#pragma unroll
    for (int m1 = 0; m1 < 8; m1++) c[m1] = poly[m0 + n * m1];
    const fe step = dom_pow(tw_lo, tw_hi, lo_bits, m0 & nmask);                         // w_N^m0
    fe t = dom_pow(tw_lo, tw_hi, lo_bits, ((uint64_t)j0 * m0) & nmask);                 // w_N^(j*m0) for the first local coset
    for (uint32_t jl = 0; jl < cosets; jl++) {
        fe_acc A; fe_acc_zero(A);                        // eight products, one reduction
        fe_acc_add(A, c[0]);
#pragma unroll
        for (int m1 = 1; m1 < 8; m1++) fe_acc_mac(A, c[m1], cj[jl * 8 + m1]);
        out[(size_t)jl * n + m0] = fe_mul(fe_acc_reduce(A), t);
        t = fe_mul(t, step);
    }
}

// The same folding when a context owns ALL B = 8 S cosets (one GPU): with j = j1 S + js, w_B^(j m1) = w_8^(j1 m1) * w_B^(js m1), so for each of the
// S residues js the eight coefficients are scaled by w_B^(js m1) and ONE 8-point DFT over m1 gives the sums of the eight cosets j1 S + js:
// 5 + 7 multiplications per eight cosets instead of 56 multiply-accumulates and 8 reductions (fold8_kernel 0.44 -> 0.26 ms at 2^20, blowup 32).
template <int S>
__global__ void __launch_bounds__(256) fold8_dft_kernel(const fe* __restrict__ poly, fe* __restrict__ out, const fe* tw_lo, const fe* tw_hi, uint32_t lo_bits,
                                                        uint32_t log_n, uint32_t log_N) {
    __shared__ fe pre[S * 8];                                        // w_B^(js * m1) = w_N^(n * js * m1)
    const size_t n = (size_t)1 << log_n;
    const uint64_t nmask = ((uint64_t)1 << log_N) - 1;
    for (uint32_t i = threadIdx.x; i < S * 8; i += blockDim.x) pre[i] = dom_pow(tw_lo, tw_hi, lo_bits, ((uint64_t)(i >> 3) * (i & 7) << log_n) & nmask);
    __syncthreads();
    const size_t m0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m0 >= n) return;
    fe c[8];
#pragma unroll
    for (int m1 = 0; m1 < 8; m1++) c[m1] = poly[m0 + n * m1];
    const fe r1 = dom_pow(tw_lo, tw_hi, lo_bits, (uint64_t)1 << (log_N - 3));          // w_8
    const fe r2 = fe_sqr(r1), r3 = fe_mul(r2, r1);
    const fe step = dom_pow(tw_lo, tw_hi, lo_bits, m0 & nmask);                         // w_N^m0
    const fe step_s = dom_pow(tw_lo, tw_hi, lo_bits, ((uint64_t)S * m0) & nmask);       // w_N^(S m0): from coset j to j + S
    fe t_js = fe_one();                                                                 // w_N^(js m0)
#pragma unroll 1
    for (uint32_t js = 0; js < S; js++) {
        fe x[8];
        x[0] = c[0];
#pragma unroll
        for (int m1 = 1; m1 < 8; m1++) x[m1] = js ? fe_mul(c[m1], pre[js * 8 + m1]) : c[m1];
        // 8-point DFT with root w_8, radix-2 DIF: X[j1] = sum_m1 x[m1] w_8^(j1 m1); stage outputs in bit-reversed positions
        fe a0, a1, a2, a3, a4, a5, a6, a7;
        fe_addsub(x[0], x[4], a0, a4); fe_addsub(x[1], x[5], a1, a5); fe_addsub(x[2], x[6], a2, a6); fe_addsub(x[3], x[7], a3, a7);
        a5 = fe_mul(a5, r1); a6 = fe_mul(a6, r2); a7 = fe_mul(a7, r3);
        fe b0, b1, b2, b3, b4, b5, b6, b7;
        fe_addsub(a0, a2, b0, b2); fe_addsub(a1, a3, b1, b3); fe_addsub(a4, a6, b4, b6); fe_addsub(a5, a7, b5, b7);
        b3 = fe_mul(b3, r2); b7 = fe_mul(b7, r2);
        fe X[8];
        fe_addsub(b0, b1, X[0], X[4]); fe_addsub(b2, b3, X[2], X[6]); fe_addsub(b4, b5, X[1], X[5]); fe_addsub(b6, b7, X[3], X[7]);
        fe t = t_js;
#pragma unroll
        for (uint32_t j1 = 0; j1 < 8; j1++) {
            out[((size_t)j1 * S + js) * n + m0] = fe_mul(X[j1], t);
            if (j1 < 7) t = fe_mul(t, step_s);
        }
        t_js = fe_mul(t_js, step);
    }
}

void k_lde_fold8(dst_ctx* c, const fe* poly8n, fe* out) {
    // stage the folded inputs in `out` itself, then transform each coset in place (pass A reads out, pass B writes out)
    dim3 g((unsigned)((c->n + 255) / 256));
    const char* e = c->sw("DISTAFF_FOLD8_DFT");
    const bool all_cosets = c->Bc == c->B && c->j0 == 0 && !(e && e[0] == '0');
    const double bytes = 16.0 * c->n * (8 + c->Bc);
#define FOLD8_DFT(S_) { KScope ks_(c, "fold8_dft_kernel", bytes); hipLaunchKernelGGL(fold8_dft_kernel<S_>, g, dim3(256), 0, c->stream, poly8n, out, c->tw_lo, c->tw_hi, c->tw_lo_bits, c->log_n, c->log_N); }
    if (all_cosets && c->B == 16) FOLD8_DFT(2)
    else if (all_cosets && c->B == 32) FOLD8_DFT(4)
    else if (all_cosets && c->B == 64) FOLD8_DFT(8)
    else if (all_cosets && c->B == 128) FOLD8_DFT(16)
    else if (all_cosets && c->B == 256) FOLD8_DFT(32)
    else { KScope ks_(c, "fold8_kernel", bytes); hipLaunchKernelGGL(fold8_kernel, g, dim3(256), c->Bc * 8 * sizeof(fe), c->stream, poly8n, out, c->tw_lo, c->tw_hi, c->tw_lo_bits, c->log_n, c->log_N, (uint32_t)c->j0, (uint32_t)c->Bc); }
#undef FOLD8_DFT
    ntt_transform(c, {out, 0, c->n, out, 0, c->n}, c->Bc, 1, false, false);
}

// ---- inverse transform of size 8n from coset-major input ------------------------------------------------------------------
// v[q][k] = V(w_8n^(8k+q)); c[m0 + n*m1] = (1/8n) sum_q w_8^(-q*m1) * w_8n^(-q*m0) * (sum_k v[q][k] w_n^(-k*m0)).
// X[m1] = (1/8) sum_q w_8^(-q*m1) * w_8n^(-q*m0) * work[q][m0], m1 < 8: the 8n coefficients out[m0 + n*m1] of residue class m0
__device__ __forceinline__ void cross8_point(const fe* __restrict__ work, size_t m0, size_t n, const fe* itw_lo, const fe* itw_hi, uint32_t lo_bits,
                                             uint32_t log_N, uint32_t log_b, const fe& eight_inv, fe (&X)[8]) {
    const uint64_t nmask = ((uint64_t)1 << log_N) - 1;
    fe x[8];
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
        fe v = work[(size_t)q * n + m0];
        uint64_t e = (((uint64_t)q * m0) << (log_b - 3)) & nmask;          // w_8n = w_N^(B/8)
        x[q] = e ? fe_mul(v, dom_pow(itw_lo, itw_hi, lo_bits, e)) : v;
    }
    // 8-point DFT with root r = w_8^-1 = w_N^-(N/8): X[m1] = sum_q x[q] r^(q*m1)
    fe r1 = dom_pow(itw_lo, itw_hi, lo_bits, (uint64_t)1 << (log_N - 3));
    fe r2 = fe_sqr(r1), r3 = fe_mul(r2, r1);
    // DIF radix-2, three stages
    fe a0 = fe_add(x[0], x[4]), a4 = fe_sub(x[0], x[4]);
    fe a1 = fe_add(x[1], x[5]), a5 = fe_mul(fe_sub(x[1], x[5]), r1);
    fe a2 = fe_add(x[2], x[6]), a6 = fe_mul(fe_sub(x[2], x[6]), r2);
    fe a3 = fe_add(x[3], x[7]), a7 = fe_mul(fe_sub(x[3], x[7]), r3);
    fe b0 = fe_add(a0, a2), b2 = fe_sub(a0, a2);
    fe b1 = fe_add(a1, a3), b3 = fe_mul(fe_sub(a1, a3), r2);
    fe b4 = fe_add(a4, a6), b6 = fe_sub(a4, a6);
    fe b5 = fe_add(a5, a7), b7 = fe_mul(fe_sub(a5, a7), r2);
    X[0] = fe_mul(fe_add(b0, b1), eight_inv); X[4] = fe_mul(fe_sub(b0, b1), eight_inv);
    X[2] = fe_mul(fe_add(b2, b3), eight_inv); X[6] = fe_mul(fe_sub(b2, b3), eight_inv);
    X[1] = fe_mul(fe_add(b4, b5), eight_inv); X[5] = fe_mul(fe_sub(b4, b5), eight_inv);
    X[3] = fe_mul(fe_add(b6, b7), eight_inv); X[7] = fe_mul(fe_sub(b6, b7), eight_inv);
}
__global__ void cross8_kernel(const fe* __restrict__ work, fe* __restrict__ out, const fe* itw_lo, const fe* itw_hi, uint32_t lo_bits,
                              uint32_t log_n, uint32_t log_N, uint32_t log_b, fe eight_inv) {
    const size_t n = (size_t)1 << log_n;
    size_t m0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m0 >= n) return;
    fe X[8];
    cross8_point(work, m0, n, itw_lo, itw_hi, lo_bits, log_N, log_b, eight_inv, X);
#pragma unroll
    for (int m1 = 0; m1 < 8; m1++) out[m0 + (size_t)m1 * n] = X[m1];
}

// ---- combine_polys in one pass (constraint_table.rs:54-88) -----------------------------------------------------------------------------
// The constraint polynomial is  I(x) / (x - 1)  +  F(x) / (x - x_last)  +  T(x) * (x - x_last) / (x^n - 1)  (8n coefficients).
//  * T comes from the inverse-transformed evaluation cosets `work[8][n]`: the 8-point step across cosets gives, per residue class m0,
//    the eight coefficients t[m0 + n m1]; the division by (x^n - 1) / (x - x_last) (polynom.rs:202-236) needs the stride-n suffix sums
//    S_r[k] = sum_{s >= k} t[r + n s] of the classes m0 and m0 - 1:  out[m0 + n m1] = S_{m0-1}[m1 + 1] - x_last * S_{m0}[m1 + 1]
//    (class n - 1 one level down for m0 = 0; nothing above 7n) -- a lane's left neighbour hands its sums over through LDS.
//  * I = A + x^p A', F = C + x^p C' with p = 6n + 2 and A, A', C, C' of n coefficients each (linear combinations of the trace polynomials,
//    dst_internal_boundary_quotients): the quotients of the sparse 8n-coefficient polynomials follow from the n-coefficient quotients.
//    With sA[1 + i] = sum_{t > i} A_t, sA'[0] = sum A' (exclusive suffix sums of the arrays extended by a leading zero) and
//    eC[1 + i] = sum_{t > i} C_t b^(t - i - 1), eC'[0] = C'(b) for b = x_last:
//        i < n:            sA[1 + i] + sA'[0]  +  eC[1 + i] + b^(p - 1 - i) eC'[0]
//        n <= i < p:       sA'[0]              +  b^(p - 1 - i) eC'[0]
//        p <= i < p + n:   sA'[1 + i - p]      +  eC'[1 + i - p]
//    and b^(p - 1 - i) = w_n^(m0 - 1) for every i of class m0 (b has order n).
// The reference's sequence -- two more 8n-point inverse transforms, three divisions and two additions over 8n coefficients each -- is
// DISTAFF_COMBINE=steps (api.hip; the tests compare both).
struct CombineArgs {
    const fe* work; fe* cpoly;
    const fe *sA, *sAp, *eC, *eCp;                 // n + 1 entries each, or all null: transition part only
    const fe *itw_lo, *itw_hi, *tw_lo, *tw_hi;
    uint32_t lo_bits, log_n, log_N, log_b;
    fe eight_inv, x_last;
};
#define COMBINE_THREADS 256
__global__ void __launch_bounds__(COMBINE_THREADS) combine_fused_kernel(CombineArgs a) {
    __shared__ fe S[COMBINE_THREADS][8];
    const size_t n = (size_t)1 << a.log_n;
    const uint32_t t = threadIdx.x;
    // lane t of block b: class m0 = 255 b + t - 1; lane 0 only serves lane 1 as its left neighbour (class n - 1 for the first block)
    const size_t m_plus = (size_t)blockIdx.x * (COMBINE_THREADS - 1) + t;
    const bool inside = m_plus <= n;                             // m0 = m_plus - 1 in [-1, n - 1]
    const size_t m0 = inside ? (m_plus + n - 1) & (n - 1) : 0;
    fe X[8], Sx[9];
    cross8_point(a.work, m0, n, a.itw_lo, a.itw_hi, a.lo_bits, a.log_N, a.log_b, a.eight_inv, X);
    Sx[8] = fe_zero();
#pragma unroll
    for (int k = 7; k >= 0; k--) Sx[k] = k == 7 ? X[7] : fe_add(X[k], Sx[k + 1]);
#pragma unroll
    for (int k = 0; k < 8; k++) S[t][k] = Sx[k];
    __syncthreads();
    if (t == 0 || m_plus > n) return;
    const bool first = m0 == 0;
    fe term = fe_zero();                                         // what every i < p of this class receives from the boundary quotients
    if (a.sA) {
        const fe P = dom_pow(a.tw_lo, a.tw_hi, a.lo_bits, (uint64_t)((m0 + n - 1) & (n - 1)) << a.log_b);      // w_n^(m0 - 1)
        term = fe_add(a.sAp[0], fe_mul(P, a.eCp[0]));
    }
#pragma unroll
    for (int m1 = 0; m1 < 8; m1++) {
        fe v;
        if (m1 < 7) v = fe_sub(first ? S[t - 1][m1] : S[t - 1][m1 + 1], fe_mul(a.x_last, Sx[m1 + 1]));
        else v = first ? S[t - 1][7] : fe_zero();                // i = 7n is the last coefficient of the quotient
        if (a.sA) {
            if (m1 == 0) v = fe_add(v, fe_add(fe_add(a.sA[1 + m0], a.eC[1 + m0]), term));
            else if (m1 < 6 || (m1 == 6 && m0 < 2)) v = fe_add(v, term);
            else if (m1 == 6) v = fe_add(v, fe_add(a.sAp[m0 - 1], a.eCp[m0 - 1]));                  // i - p = m0 - 2
            else if (m0 < 2) v = fe_add(v, fe_add(a.sAp[m0 + n - 1], a.eCp[m0 + n - 1]));          // i - p = m0 + n - 2
        }
        a.cpoly[m0 + (size_t)m1 * n] = v;
    }
}
void k_combine_fused(dst_ctx* c, const fe* work, const fe* q4, size_t q_stride, fe* cpoly) {
    CombineArgs a{};
    a.work = work; a.cpoly = cpoly;
    if (q4) { a.sA = q4; a.sAp = q4 + q_stride; a.eC = q4 + 2 * q_stride; a.eCp = q4 + 3 * q_stride; }
    a.itw_lo = c->itw_lo; a.itw_hi = c->itw_hi; a.tw_lo = c->tw_lo; a.tw_hi = c->tw_hi;
    a.lo_bits = c->tw_lo_bits; a.log_n = c->log_n; a.log_N = c->log_N; a.log_b = c->log_b;
    a.eight_inv = c->eight_inv; a.x_last = c->x_last;
    const size_t blocks = (c->n + 1 + (COMBINE_THREADS - 2)) / (COMBINE_THREADS - 1);
    KScope ks_(c, "combine_fused_kernel", 16.0 * c->n * 16);
    hipLaunchKernelGGL(combine_fused_kernel, dim3((unsigned)blocks), dim3(COMBINE_THREADS), 0, c->stream, a);
}

// the two halves of k_intt8_cosets for the sharded prover: a rank inverts the size-n transforms of the evaluation cosets it owns BEFORE the
// exchange (1/world of them instead of all eight on every rank), the 8-point step across cosets follows on the gathered arrays
void k_intt_cosets_local(dst_ctx* c, fe* vals, fe* out, size_t cosets) { ntt_transform(c, {vals, 0, c->n, out, 0, c->n}, cosets, 1, true, false); }
void k_cross8(dst_ctx* c, const fe* work, fe* out8n) {
    KScope ks_(c, "cross8_kernel", 256.0 * c->n);
    hipLaunchKernelGGL(cross8_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, work, out8n, c->itw_lo, c->itw_hi, c->tw_lo_bits, c->log_n, c->log_N, c->log_b, c->eight_inv);
}
void k_intt8_cosets(dst_ctx* c, fe* vals, fe* out8n, fe* work) { k_intt_cosets_local(c, vals, work, 8); k_cross8(c, work, out8n); }

// ---- layout conversion (inspection; replicated FRI tail of the sharded path) ------------------------------------------------------------------------------------
__global__ void coset_to_natural_kernel(const fe* __restrict__ src, fe* __restrict__ dst, size_t n, size_t cosets) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * cosets) return;
    size_t k = i / cosets, j = i % cosets;
    dst[i] = src[j * n + k];
}
void k_coset_to_natural_len(dst_ctx* c, const fe* src, size_t cosets, size_t len, fe* dst) {      // [cosets][len] -> natural [len * cosets]
    size_t total = len * cosets;
    { KScope ks_(c, "coset_to_natural_kernel", 32.0 * total); hipLaunchKernelGGL(coset_to_natural_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, src, dst, len, cosets); }
}
