// The prover steps that every driver queues the same way -- dst_prove and the phase calls (api.hip), dst_prove_sharded and the
// host-orchestrated dst_shard_* phase calls (shard.hip) -- each stated once (host/steps_impl.h), and the plumbing they share.  Host code
// only: what differs between the drivers (the trace commit, the tree exchanges, where the host waits, how phase times are split) stays
// with the drivers.  Ordinary C++ linkage; nothing here leaves the library (-fvisibility=hidden).  host/steps_impl.h is compiled as part of
// api.hip (like verify/): the lists of units in the Makefiles stay as they are.
#pragma once
#include <chrono>
#include <vector>
#include "../ctx.h"

namespace step {

// ---- plumbing -------------------------------------------------------------------------------------------------------------------------
inline double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// milliseconds between two events recorded on a stream, < 0 when the runtime cannot tell (the error is consumed).  What a driver does
// with the time no event covers is its own policy.
inline double event_ms(hipEvent_t from, hipEvent_t to) {
    float ms = 0;
    if (from && to && hipEventElapsedTime(&ms, from, to) == hipSuccess) return (double)ms;
    (void)hipGetLastError();
    return -1.0;
}

// The last ELEMS elements of dst_ctx::scratch: the small device vectors of the phase in flight.  Steps 3-5 and step 6 never overlap on
// the stream, so they share the region.
struct ScratchTail {
    enum : size_t { ELEMS = 1024, MAX_W = 128, DRAWS = 344, MAX_TC = HS_DRAWS_BYTES / sizeof(fe) - DRAWS, COMPOSE = 516, TZ1 = 520, TZ2 = TZ1 + MAX_W, CZ = TZ2 + MAX_W };
    fe* base;
    explicit ScratchTail(const dst_ctx* c) : base(c->scratch + c->scratch_elems - ELEMS) {}
    // steps 3-5 (step::eval_constraints)
    fe* coef() const { return base; }                // [344] constraint coefficients
    fe* tc() const { return base + DRAWS; }          // [<= MAX_TC] transition coefficients in constraint order
    // step 6 (compose_impl, api.hip)
    fe* draws() const { return base; }               // [516] composition draws
    fe* tz1() const { return base + TZ1; }           // [W] T(z)
    fe* tz2() const { return base + TZ2; }           // [W] T(z g)
    fe* cz() const { return base + CZ; }             // [1] C(z)
};
static_assert(ScratchTail::DRAWS + ScratchTail::MAX_TC <= ScratchTail::ELEMS && ScratchTail::COMPOSE <= ScratchTail::TZ1 && ScratchTail::CZ + 1 <= ScratchTail::ELEMS,
              "the scratch tail holds every phase's vectors for W <= 128 registers");

// ---- steps 3-5 ------------------------------------------------------------------------------------------------------------------------
// Step 3: remembers the 344 constraint coefficients (dst_ctx::air_draws), uploads them with the transition coefficients and queues the
// AIR evaluation.  defer_check: the host does not wait for the verdict (k_constraint_check / the device word c->d_u64 later).
// check_here = false: the evaluation alone; the caller queues the check of the trace rows, the source of the verdict, itself (dst_prove).
int eval_constraints(dst_ctx* c, const dst_public* pub, const uint8_t* coeffs, int64_t* bad_step, bool defer_check, bool check_here = true);
// the two boundary combinations in coefficient form (ip / fp: 8n coefficients each; or the four n-coefficient pieces o0 .. o3), and the
// n-coefficient quotients of them that the fused combination reads
int boundary_polys(dst_ctx* c, const fe* draws344, fe* ip, fe* fp, fe* o0 = nullptr, fe* o1 = nullptr, fe* o2 = nullptr, fe* o3 = nullptr);
int boundary_quotients(dst_ctx* c, const fe* draws344, fe* q4, size_t stride);
// Step 4, combine_polys (constraint_table.rs:54-88) -> c->cpoly, from c->ceval and c->air_draws.  parts: 1 = the two boundary combinations
// and their divisions (need nothing from other ranks), 2 = transition part and sum; 3 = both.  The transition evaluations may already be
// inverse-transformed per coset (c->ceval_inverted, dst_prove_sharded).  What follows cpoly depends on the layout and is the caller's.
int combine(dst_ctx* c, int parts);

// ---- step 7 ---------------------------------------------------------------------------------------------------------------------------
void fri_file_root(dst_ctx* c, int d, const uint8_t root[32]);      // c->fri_roots[d]
inline size_t fri_nd(const dst_ctx* c, int d) { return c->fri_size[d] / c->B; }     // elements per coset in layer d
// evaluations of a natural-order layer (a replicated layer 0 is fri_nat0: fri_e[0] is the rank's coset-major piece)
inline fe* fri_layer_natural(const dst_ctx* c, int d) { return (d == 0 && c->fri_rep_from == 0) ? c->fri_nat0 : c->fri_e[d]; }
// fri::reduce (fri/prover.rs:11-53) over the natural-order layers d0 .. L-1 without a host round trip per layer: leaves, tree, x = prng(root)
// drawn on the device and the fold, until fri_tail_starts_at (ctx.h); then the single-launch tail; ONE wait; all roots filed.  d0 = 0 on a
// single-GPU layout reads the coset-major composition.  Leaves fri_committed = L, fri_folded = L - 1.
int fri_commit_natural(dst_ctx* c, int d0);
// a coset-major layer of the sharded layout: leaves + rank-local tree levels; the fold with x from the host or, alpha_dev != nullptr, from device memory
void fri_shard_layer(dst_ctx* c, int d);
void fri_shard_fold(dst_ctx* c, int d, fe x, const fe* alpha_dev = nullptr);

// ---- step 8 ---------------------------------------------------------------------------------------------------------------------------
// seed = hash of the FRI roots, grinding, query positions (prover.rs:120-133)
int query_seed(dst_ctx* c, uint64_t* nonce, std::vector<uint64_t>& positions);

}  // namespace step

// ---- defined by the drivers, used across them ---------------------------------------------------------------------------------------------
int build_proof_local(dst_ctx* c, const uint64_t* positions, uint32_t num_positions, uint64_t pow_nonce, std::vector<uint8_t>& proof);   // shard.hip: single-GPU openings, every item local
int ensure_shard_buffers(dst_ctx* c);                // shard.hip: exchange buffers of a sharded context
