/* libdistaff_hip.so -- C-ABI of the MI355X-native STARK prover backend for Distaff.
 *
 * The reference (GuildOfWeavers/distaff v0.5.1, pure Rust) has no FFI layer; the drop-in seam is the body of
 * `stark::prove` (/root/reference/src/stark/prover.rs:17), which is called from exactly one place
 * (/root/reference/src/lib.rs:62).  A Rust maintainer replaces that body with calls to the entry points below
 * (INTEGRATION.md shows the `extern "C"` block); Fiat-Shamir dependencies between the nine prover steps force the
 * boundary to be phase-wise, and `dst_prove` chains the phases with the library's own restatement of the
 * reference's challenge derivation.
 *
 * Conventions
 *   - a field element is 16 bytes, little-endian, canonical (< p = 2^128 - 45*2^40 + 1); this is the memory image of
 *     the reference's `u128` (/root/reference/src/utils/mod.rs:35-41).  Pointers need only byte alignment.
 *   - a digest is 32 bytes (BLAKE3, the only serialisable `HashFunction`: src/stark/options.rs:97-120).
 *   - every function returns DST_OK (0) or a negative error code and never aborts the process (the reference
 *     panics instead: src/lib.rs:32,49,56, src/stark/constraints/evaluator.rs:155); `dst_last_error` gives the text.
 *   - a context owns all device memory and one HIP stream; it is not thread-safe; calls are synchronous (they
 *     return after the stream has drained) unless stated otherwise.  Host buffers are caller-owned and are only
 *     read or written during the call.
 */
#ifndef DISTAFF_HIP_H
#define DISTAFF_HIP_H
#include <stddef.h>
#include <stdint.h>

/* exported entry points (the shared library is built with hidden visibility: nothing else leaves it) */
#if defined(__GNUC__)
#define DST_API __attribute__((visibility("default")))
#else
#define DST_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define DST_OK 0
#define DST_ERR_ARG (-1)      /* invalid argument / call order */
#define DST_ERR_HIP (-2)      /* HIP runtime error (no device, out of memory, launch failure) */
#define DST_ERR_AIR (-3)      /* transition constraints not satisfied by the trace (reference panic: evaluator.rs:155) */
#define DST_ERR_STATE (-4)    /* phase called out of order */
#define DST_ERR_COMM (-5)     /* a collective of dst_prove_sharded failed or did not complete within the communicator's limit (a peer that died or
                                 never arrived); the communicator has been aborted and refuses further collectives -- destroy it, create a new one */

typedef struct dst_ctx dst_ctx;

/* Shape of one proving job; mirrors TraceTable::new (src/stark/trace/trace_table.rs:23-58) + ProofOptions (options.rs:16-27). */
typedef struct dst_params {
    uint32_t log_trace_length;   /* n = 2^log_trace_length rows, >= 4 (TraceTable asserts a power of two; MIN_TRACE_LENGTH = 16) */
    uint32_t log_blowup;         /* extension_factor = 2^log_blowup, 16 <= factor <= 256 (options.rs:39-41) */
    uint32_t width;              /* number of registers W < 128 (lib.rs:83) */
    uint32_t ctx_depth;          /* context stack registers (<= 16) */
    uint32_t loop_depth;         /* loop stack registers (<= 8) */
    uint32_t num_queries;        /* 1..128 (options.rs:43-44) */
    uint32_t grinding_factor;    /* <= 32 (options.rs:46) */
    int32_t  device;             /* HIP device ordinal */
    /* multi-GPU sharding of the LDE domain by cosets (DESIGN.md "Multi-GPU"): this context owns cosets
       [rank * B / world, (rank + 1) * B / world); world = 1 means the whole job; world is a power of two <= min(8, B / 2). */
    uint32_t rank, world;
} dst_params;

/* Public inputs / outputs of the boundary constraints (src/stark/constraints/evaluator.rs:35-79). */
typedef struct dst_public {
    uint32_t num_inputs, num_outputs;       /* <= 8 each (lib.rs:136-137) */
    uint8_t inputs[8][16];
    uint8_t outputs[8][16];
} dst_public;

/* ---- lifetime ---------------------------------------------------------------------------------------------------- */
DST_API int dst_ctx_create(const dst_params* params, dst_ctx** out);
DST_API void dst_ctx_destroy(dst_ctx* ctx);
DST_API const char* dst_last_error(const dst_ctx* ctx);      /* ctx may be NULL: returns the creation-time error */
/* milliseconds spent in each of the reference's nine prover steps during the last proof (prover.rs:28,36,66,74,87,103,112,134,167) */
DST_API int dst_phase_ms(const dst_ctx* ctx, double out_ms[9]);

/* ---- step 0: trace upload (host -> HBM).  cols[c] points to n*16 bytes of register c, i.e. the reference's
 *      column-major `Vec<Vec<u128>>` (trace_table.rs:10).  Not part of the timed prover region. ------------------------ */
DST_API int dst_trace_upload(dst_ctx* ctx, const uint8_t* const* cols);
/* same, from one contiguous [W][n] buffer */
DST_API int dst_trace_upload_contiguous(dst_ctx* ctx, const uint8_t* cols);
/* Sharded contexts (world > 1): uploads only the registers this rank interpolates, r = rank (mod world); cols[r] of the other registers is
 * not read.  dst_prove_sharded all-gathers the coefficient vectors ("trace columns shard across the GPUs"), so every GPU
 * receives 1/world of the trace from its host.  Only dst_prove_sharded accepts a context in this state. */
DST_API int dst_trace_upload_owned(dst_ctx* ctx, const uint8_t* const* cols);
/* Asynchronous form for a host-resident trace (what stark::prove receives: prover.rs:17, trace_table.rs:10).  Starts the copies of
 * the W columns on a copy stream and returns at once; the next dst_commit_trace / dst_prove interpolates and extends the registers
 * group by group as their copies land, so that all but the first group's transfer overlaps with the extension.  The host buffers
 * must stay valid until that call returns; for real overlap they must be page-locked (dst_pinned_alloc or the host's own pinning). */
DST_API int dst_trace_upload_async(dst_ctx* ctx, const uint8_t* const* cols);
DST_API int dst_pinned_alloc(size_t bytes, void** out);
DST_API int dst_pinned_free(void* p);

/* ---- steps 1-2: TraceTable::extend + build_merkle_tree (prover.rs:22-35; trace_table.rs:143,174) ---------------------- */
DST_API int dst_commit_trace(dst_ctx* ctx, uint8_t trace_root[32]);

/* ---- steps 3-5: constraint evaluation, combination, constraint LDE + Merkle tree (prover.rs:43-86) ----------------------
 * coeffs = the 344 draws of ConstraintCoefficients::new(trace_root) in draw order (utils/coefficients.rs:66).
 * On DST_ERR_AIR *bad_step receives the first trace step whose transition constraints do not vanish.  The verdict of that check
 * (the reference panics at evaluator.rs:155) travels back with the constraint root: a failing trace is reported AFTER the combination,
 * the constraint LDE and its tree were queued behind the evaluation, so the context's constraint buffers (dst_read_buffer CPOLY, CEVALS,
 * CNODES) hold values computed from a non-vanishing evaluation then; the context stays in the "trace committed" state. */
DST_API int dst_eval_constraints(dst_ctx* ctx, const dst_public* pub, const uint8_t* coeffs /* 344*16 */, uint8_t constraint_root[32], int64_t* bad_step);

/* ---- step 6: DEEP composition (prover.rs:94-101, 189-201).  draws = the 516 draws of prng_vector(constraint_root):
 * draws[0] = z, then CompositionCoefficients (coefficients.rs:80-104).  Outputs the DeepValues (proof.rs:24-28). --------- */
DST_API int dst_compose(dst_ctx* ctx, const uint8_t* draws /* 516*16 */, uint8_t* trace_at_z1 /* W*16 */, uint8_t* trace_at_z2 /* W*16 */);

/* ---- step 7: FRI commit phase (fri/prover.rs:11-53).  Call dst_fri_commit_layer (root of the current layer), then
 * dst_fri_fold with special_x = prng(root); repeat while dst_fri_commit_layer reports more = 1.  The last committed
 * layer (<= 256 evaluations) is the remainder. -------------------------------------------------------------------------- */
DST_API int dst_fri_commit_layer(dst_ctx* ctx, uint8_t layer_root[32], int* more);
DST_API int dst_fri_fold(dst_ctx* ctx, const uint8_t special_x[16]);

/* ---- step 8: proof of work (utils/proof_of_work.rs:4-32): smallest nonce >= 1 whose digest has >= grinding_factor
 * trailing zero bits in its first little-endian u64. ------------------------------------------------------------------- */
DST_API int dst_pow_grind(dst_ctx* ctx, const uint8_t seed[32], uint32_t grinding_factor, uint8_t out_seed[32], uint64_t* nonce);

/* ---- step 9: openings (prover.rs:143-165).  Serialises the whole StarkProof in the reference's wire format
 * (bincode, src/main.rs:44) for the given query positions.  Two-call protocol: pass out = NULL to get the size. --------- */
DST_API int dst_build_proof(dst_ctx* ctx, const uint64_t* positions, uint32_t num_positions, uint64_t pow_nonce,
                    uint8_t* out, size_t cap, size_t* out_len);

/* ---- the whole of stark::prove (prover.rs:17-168) on a trace already uploaded with dst_trace_upload ------------------- */
DST_API int dst_prove(dst_ctx* ctx, const dst_public* pub, uint8_t* proof_out, size_t cap, size_t* proof_len);
/* After DST_ERR_AIR from dst_prove (which has no bad_step argument) or dst_eval_constraints: the first trace step whose transition
 * constraints do not vanish, as the last check of the trace rows on this context found it; -1 when that check found none.  dst_prove
 * checks the rows beside the later phases of the proof and reports when the proof is otherwise complete. */
DST_API int64_t dst_last_bad_step(const dst_ctx* ctx);

/* ---- the other half of the reference's public pair: stark::verify (src/lib.rs:72, src/stark/verifier.rs:11) ------------
 * Host only: no context, no device, no HIP call -- it works on a machine without a GPU.  Returns DST_OK and *accepted = 1 for a valid
 * proof; DST_OK and *accepted = 0 with the reference's error string in `err` for a well-formed proof that does not verify; DST_ERR_ARG
 * (and a reason in `err`) for bytes that are not a StarkProof: truncated input, a length prefix that runs past the end, trailing bytes,
 * options outside ProofOptions::new (options.rs:35-46), a hash tag other than 0, depths outside lib.rs:80-83,138, a field element (in the
 * proof or in `pub`) that is not below p, a remainder longer than 256 values or not the last layer of the proof's own FRI layers.  `err` may be NULL;
 * the text is cut to err_cap - 1 characters.  Re-entrant: no globals.  Milliseconds on one core at any trace length. */
DST_API int dst_verify(const uint8_t program_hash[32], const dst_public* pub, const uint8_t* proof, size_t len,
                       int* accepted, char* err, size_t err_cap);
/* what a proof says about itself without verifying it (proof.rs:11-37, options.rs:16-27, 68-79) */
typedef struct dst_proof_info_t {
    uint32_t log_trace_length;          /* domain depth - log2(extension factor) */
    uint32_t extension_factor, num_queries, grinding_factor;
    uint32_t register_count;            /* 15 + ctx_depth + loop_depth + stack_depth */
    uint32_t ctx_depth, loop_depth, stack_depth;
    uint32_t op_count;
    uint32_t fri_layers, remainder_length;
    uint32_t security_level;            /* ProofOptions::security_level(optimistic = true), options.rs:68-79 */
    uint32_t security_level_proven;     /* ... (optimistic = false) */
    uint64_t pow_nonce;
} dst_proof_info_t;
DST_API int dst_proof_info(const uint8_t* proof, size_t len, dst_proof_info_t* out);

/* ---- Rescue digests and Rescue Merkle trees: what the VM's smpath.n / pmpath.n authenticate ----------------------------------------------
 * A node is two field elements (32 bytes); parent = utils::hasher::digest([l0, l1, r0, r1]): ten Rescue rounds on a six-element state
 * (src/utils/hasher.rs:12-40).  The reference only ever walks a pseudo-random path through an imaginary tree (src/examples/merkle.rs:96-108);
 * these build the tree, hand out authentication paths and lay them out as the secret tapes of the example's program.  No dst_ctx.
 * device >= 0: on that GPU (inputs are checked there); device < 0: on the host, one thread, no HIP call -- works on a machine without a GPU,
 * like dst_verify.  DST_ERR_ARG: null pointer, index past the end, log_leaves out of range, an element not below p. */
/* utils::hasher::digest (hasher.rs:12) on `count` inputs of 4 elements each -> 2 elements each */
DST_API int dst_rescue_digest_many(int device, const uint8_t* in /* count*64 */, size_t count, uint8_t* out /* count*32 */);
typedef struct dst_rtree dst_rtree;
/* tree over 2^log_leaves nodes of 2 elements (32 bytes), 1 <= log_leaves <= 26; parent = digest(l0, l1, r0, r1) (merkle.rs:112-145) */
DST_API int dst_rtree_build(int device, const uint8_t* leaves, uint32_t log_leaves, dst_rtree** out);
DST_API int dst_rtree_root(const dst_rtree* t, uint8_t root[32]);
/* authentication path of leaf `index`: [leaf, sibling, uncle, ...], log_leaves + 1 nodes = a path of "depth n = log_leaves + 1" in the
 * sense of merkle.rs:98-145 (compute_merkle_root of that path and index gives the root) */
DST_API int dst_rtree_path(const dst_rtree* t, uint64_t index, uint8_t* path /* (log_leaves+1)*32 */);
/* the secret tapes A and B that the program `read.ab dup.2 smpath.n swap.2 push.<index> roll.4 swap swap.2 pmpath.n` consumes
 * (generate_program_inputs, merkle.rs:63-94), n = log_leaves + 1: 3n - 2 elements per tape.  what = 1: the leaf and the smpath inputs only
 * (2n - 1 elements), 2: the pmpath inputs only (n - 1), 3: both.  *elems receives the count; tape_a = tape_b = NULL: size query. */
DST_API int dst_rtree_tapes(const dst_rtree* t, uint64_t index, uint32_t what, uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems, size_t* elems);
/* `count` nodes of the node array from `first`: index 1 = root, [2^k, 2^(k+1)) = the level of 2^k nodes, [2^log_leaves, 2^(log_leaves+1)) = the leaves */
DST_API int dst_rtree_read_nodes(const dst_rtree* t, uint64_t first, uint64_t count, uint8_t* out);
/* milliseconds the level kernels of dst_rtree_build took on the device (0 for a host tree).  The library owns the stream of the build, so events
 * around the launches -- without the allocation and the upload of the leaves, which a caller's clock around dst_rtree_build includes -- can only be
 * recorded here; tools/rescue_tree_time.py reports this figure, as dst_phase_ms does for the prover's steps. */
DST_API int dst_rtree_build_ms(const dst_rtree* t, double* device_ms);
/* A tree is not frozen.  dst_rtree_update replaces the leaves at `indices` (count distinct leaf indices, any order) by `leaves` (count * 32 bytes)
 * and recomputes exactly the ancestors of those leaves -- the nodes compute_merkle_root (merkle.rs:112-145) visits from any of them -- level by
 * level, at most count nodes per level; afterwards every node equals that of a tree built from the modified leaf array.  DST_ERR_ARG: a null
 * pointer with count > 0, an index past the end, a repeated index, a leaf element not below p; all of it is checked on the host before anything
 * is queued, so the tree is unchanged after DST_ERR_ARG.  count = 0: DST_OK, nothing happens.  A HIP error during the update leaves the tree
 * unusable: dst_rtree_last_error says so, and every later call on it except dst_rtree_destroy and dst_rtree_last_error returns DST_ERR_STATE. */
DST_API int dst_rtree_update(dst_rtree* t, const uint64_t* indices, const uint8_t* leaves, size_t count);
/* device milliseconds of the level launches of the last dst_rtree_update or dst_rtree_apply (events on the library's stream, as dst_rtree_build_ms; 0 for a host tree) */
DST_API int dst_rtree_update_ms(const dst_rtree* t, double* device_ms);
/* authentication paths of `count` leaves, (log_leaves + 1) * 32 bytes each, in the order of `indices` (repeats allowed); the layout of each is
 * dst_rtree_path's (merkle.rs:98-145).  On a device tree: one upload of the node positions, one gather launch, one copy back, whatever count is. */
DST_API int dst_rtree_paths(const dst_rtree* t, const uint64_t* indices, size_t count, uint8_t* paths);
/* dst_rtree_tapes (generate_program_inputs, merkle.rs:63-94) for `count` leaves: tape_a / tape_b receive count blocks of *elems_each elements,
 * block i for indices[i]; cap_elems_each >= *elems_each; tape_a = tape_b = NULL: size query */
DST_API int dst_rtree_tapes_many(const dst_rtree* t, const uint64_t* indices, size_t count, uint32_t what,
                                 uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each);
/* An ORDERED batch of leaf writes, what a host that keeps state performs: operation i replaces leaf indices[i] by leaves[i] in the tree as
 * operations 0 .. i-1 left it; indices may repeat and come in any order.  paths[i] (may be NULL) is the authentication path of indices[i] in the
 * tree BEFORE operation i, in dst_rtree_path's layout: its first node is the old leaf, and its siblings are those of the path after the write
 * too, so the one path serves "old leaf under the previous root" and "new leaf under roots[i]".  roots[i] (may be NULL) is the root after
 * operation i; the root before operation 0 is dst_rtree_root before the call.  Afterwards every node equals that of a tree built from the final
 * leaves.  On a device tree all operations are hashed together, one launch per level: log_leaves level launches and as many scatters, one
 * upload, one synchronisation, whatever count is (dst_rtree_update_ms then reports these launches).  A host tree applies them one after the
 * other.  DST_ERR_ARG -- a null pointer with count > 0, an index past the end, a leaf element not below p, count >= 2^31 -- is found on the host
 * before anything is queued and leaves the tree unchanged; count = 0: DST_OK, nothing happens; a HIP error leaves the tree unusable as in
 * dst_rtree_update. */
DST_API int dst_rtree_apply(dst_rtree* t, const uint64_t* indices, const uint8_t* leaves /* count*32 */, size_t count,
                            uint8_t* paths /* count*(log_leaves+1)*32, or NULL */, uint8_t* roots /* count*32, or NULL */);
/* host only, no tree: dst_rtree_tapes_many (generate_program_inputs, merkle.rs:63-94) over `count` paths of n nodes each that the caller holds
 * -- the witnesses of dst_rtree_apply / dst_stree_apply, or paths from anywhere; 2 <= n <= 64, indices[i] below 2^(n-1).  The same `what`, the
 * same size query.  Errors are reported by dst_rtree_last_error(NULL). */
DST_API int dst_rescue_path_tapes(const uint8_t* paths /* count*n*32 */, uint32_t n, const uint64_t* indices, size_t count, uint32_t what,
                                  uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each);
/* ---- checking paths and witnesses: the tree-side counterpart of dst_verify.  No tree, no dst_ctx: what a host that holds only a root needs.
 * DST_ERR_ARG: a null pointer with count > 0, n outside 2 .. 64, an index not below 2^(n-1), count >= 2^31, an element of the paths, leaves or
 * roots not below p (found on the host for what the host compares, on the device for what the kernel reads).  A path that does not verify is NOT
 * an error: the call returns DST_OK, first_bad / why say so.  count = 0: DST_OK, *first_bad = -1.  Errors are reported by dst_rtree_last_error(NULL). */
/* compute_merkle_root (src/examples/merkle.rs:112-145) of `count` paths of n nodes each, 2 <= n <= 64, indices[i] < 2^(n-1).
 * leaves == NULL: roots[i] is what path i resolves to.  leaves != NULL: what it resolves to with its first node replaced by leaves[i]
 * (the root after a write that keeps the siblings).  device >= 0: one upload, ONE launch, one copy back whatever count and n are;
 * device < 0: on the host.  *device_ms (may be NULL): events around the launch, 0 on the host. */
DST_API int dst_rescue_path_roots(int device, const uint8_t* paths /* count*n*32 */, uint32_t n, const uint64_t* indices, size_t count,
                                  const uint8_t* leaves /* count*32, or NULL */, uint8_t* roots /* count*32 */, double* device_ms);

enum { DST_PATH_OK = 0, DST_PATH_BAD_LEAF = 1, DST_PATH_BAD_ROOT = 2, DST_PATH_BAD_NEXT_ROOT = 3 };

/* membership / absence: every path resolves to `root`; with leaves != NULL also path i's first node equals leaves[i] (the empty leaf of a
 * sparse tree: the key is absent).  *first_bad = -1 and *why = DST_PATH_OK when all hold, else the lowest failing i and what failed there
 * (within one i the leaf is looked at before the root). */
DST_API int dst_rescue_verify_paths(int device, const uint8_t root[32], const uint8_t* paths, uint32_t n, const uint64_t* indices,
                                    const uint8_t* leaves /* or NULL */, size_t count, int64_t* first_bad, uint32_t* why, double* device_ms);

/* the checker of dst_rtree_apply / dst_stree_apply: write i is accepted when paths[i] resolves to the root before it (root_before for i = 0,
 * else the root after write i-1 AS COMPUTED HERE: BAD_ROOT) and, where roots != NULL, the same path with leaves[i] as its first node resolves
 * to roots[i] (BAD_NEXT_ROOT).  root_after (may be NULL) receives the computed root after the last write, root_before when count = 0: a
 * client that holds only a root follows the state with it.  All 2*count chains run in one launch.
 * With roots == NULL nothing states what leaves[i] must resolve to, so a wrong new leaf shows one write LATER, as that write's BAD_ROOT;
 * in the last write it shows only in root_after, which the caller then holds against the root it expects. */
DST_API int dst_rescue_verify_writes(int device, const uint8_t root_before[32], const uint8_t* paths, uint32_t n, const uint64_t* indices,
                                     const uint8_t* leaves /* count*32 */, const uint8_t* roots /* count*32, or NULL */, size_t count,
                                     int64_t* first_bad, uint32_t* why, uint8_t root_after[32], double* device_ms);

/* following ordered writes with HELD PATHS, without the tree: a client that holds a root and the paths of `held` keys of its own receives the
 * witnesses of a dst_rtree_apply / dst_stree_apply batch and leaves with root_after and its paths under root_after.  The writes are verified
 * first, exactly as dst_rescue_verify_writes verifies them with the same arguments -- first_bad, why and root_after are that call's.  Nothing is
 * written from witnesses that do not hold: when *first_bad >= 0 the call returns DST_OK and out_paths is untouched to the byte.  Otherwise
 * out_paths[j] is the path of held_indices[j] after the last write: with c_i[0] = leaves[i], c_i[t] = digest(c_i[t-1], paths[i][t]) ordered by
 * bit t-1 of indices[i] (the nodes above write i's leaf right after it), node 0 is leaves[i] of the LAST write i with indices[i] ==
 * held_indices[j], node k >= 1 is c_i[k-1] of the LAST write i with indices[i] >> (k-1) == (held_indices[j] >> (k-1)) ^ 1, and a node no write
 * supplies is held_paths[j]'s.  THE HELD PATHS ARE NOT CHECKED: one that resolved to root_before resolves to root_after; one that did not is the
 * caller's problem, found with dst_rescue_verify_paths(root_after, out_paths, ...).  Held indices may repeat; out_paths may be held_paths
 * itself.  held = 0: the call is dst_rescue_verify_writes.  count = 0: out_paths is a copy of held_paths, root_after = root_before.
 * DST_ERR_ARG as above, before anything is written, also for a held index not below 2^(n-1), held >= 2^31 and an element of held_paths not
 * below p.  device >= 0: one upload, ONE launch for all 2*count chains, one launch that gathers the paths, one synchronisation, one copy back,
 * whatever count, held and n are; *device_ms: events around the two launches.  device < 0: on the host, one thread, no HIP call. */
DST_API int dst_rescue_refresh_paths(int device, const uint8_t root_before[32], const uint8_t* paths /* count*n*32 */, uint32_t n, const uint64_t* indices,
                                     const uint8_t* leaves /* count*32 */, const uint8_t* roots /* count*32, or NULL */, size_t count,
                                     const uint64_t* held_indices, const uint8_t* held_paths /* held*n*32 */, size_t held,
                                     uint8_t* out_paths /* held*n*32; may be held_paths itself */,
                                     int64_t* first_bad, uint32_t* why, uint8_t root_after[32] /* may be NULL */, double* device_ms);
/* of *device_ms of the calling thread's last dst_rescue_refresh_paths / dst_rescue_refresh_paths_w, the part of the launch that gathers the paths
 * (an event between the two launches); 0 when that call ran on the host, gathered nothing or failed before its launches */
DST_API double dst_rescue_refresh_last_gather_ms(void);

/* ---- compressed batch openings (multiproofs): the paths of many leaves without the nodes they share.  `count` independent paths are
 * count*n*32 bytes and count*(n-1) digests to check, however much of the tree they share; a multiproof ships every needed node once and its
 * check computes every shared ancestor once.  It is the node set of the reference's BatchMerkleProof (prove_batch / verify_batch,
 * src/crypto/merkle.rs:64-263), laid out level by level.  Conventions of dst_rescue_path_roots: n = the nodes of a path, 2 <= n <= 64,
 * D = n - 1 the depth (log_leaves of a dense tree, depth of a sparse one); node (l, p) is the node of level l at position p < 2^l, level D holds
 * the leaves, level 0 is the root (heap position 2^l + p of a dense tree's node array).
 * For a set S of `count` DISTINCT leaf indices below 2^D let K_D = S and K_{l-1} = { p >> 1 : p in K_l }.  The supplied siblings of level l are
 * the nodes (l, p ^ 1) with p in K_l and p ^ 1 not in K_l.  A multiproof of S is
 *   leaves: count nodes, leaves[i] = the leaf at indices[i], in the caller's order (any order);
 *   nodes:  the supplied siblings of level D, then of level D - 1, ... down to level 1, ascending by position within a level.
 * Their number M = sum over l = 1 .. D of #{ p in K_l : p ^ 1 not in K_l } and their order depend only on S and D, never on the order of
 * `indices`; checking computes digests = sum over l = 0 .. D - 1 of |K_l| parents.
 * DST_ERR_ARG: a null pointer with count > 0, n outside 2 .. 64, an index not below 2^(n-1), a repeated index, num_nodes != M, count >= 2^31,
 * count + M + digests >= 2^32, count = 0 in the three hashing calls (a proof of nothing proves nothing) -- all found on the host before anything
 * is queued -- and an element of leaves or nodes not below p, found before any result is written (on the host, or by the kernel as in the path
 * checks).  The tree-less calls report errors by dst_rtree_last_error(NULL); device < 0 runs on the host, one thread, no HIP call. */
/* M and the digest count of a set, no hashing (host only); count = 0 gives 0 and 0 */
DST_API int dst_rescue_multiproof_size(uint32_t n, const uint64_t* indices, size_t count, size_t* num_nodes, uint64_t* digests);
/* the multiproof of `count` distinct leaves of a tree (n = log_leaves + 1): leaves receives count*32 bytes, nodes *num_nodes * 32 <= cap_nodes * 32.
 * nodes == NULL: size query, only *num_nodes is written.  On a device tree: one upload of positions, one gather launch, one copy back, whatever
 * count is.  count = 0: DST_OK with 0 nodes.  The tree is never changed. */
DST_API int dst_rtree_multiproof(const dst_rtree* t, const uint64_t* indices, size_t count, uint8_t* leaves /* count*32 */,
                                 uint8_t* nodes /* cap_nodes*32, or NULL */, size_t cap_nodes, size_t* num_nodes);
/* the root a multiproof resolves to; *digests (may be NULL) = how many parents were computed.  device >= 0: one upload (leaves, nodes and the job
 * lists of every level), at most n - 1 level launches, one synchronisation, one copy back; *device_ms (may be NULL): events around the launches.
 * Called with OTHER leaves over the same nodes it gives the root after those unordered writes -- the supplied siblings are exactly the nodes
 * such writes do not change -- which is how a client that holds only a root follows dst_rtree_update / dst_stree_set of stored keys. */
DST_API int dst_rescue_multiproof_root(int device, uint32_t n, const uint64_t* indices, const uint8_t* leaves /* count*32 */, size_t count,
                                       const uint8_t* nodes /* num_nodes*32 */, size_t num_nodes, uint8_t root[32], uint64_t* digests, double* device_ms);
/* *ok = 1 when the multiproof resolves to `root`, else 0: a multiproof that does not is NOT an error, the call returns DST_OK */
DST_API int dst_rescue_verify_multiproof(int device, const uint8_t root[32], uint32_t n, const uint64_t* indices, const uint8_t* leaves /* count*32 */,
                                         size_t count, const uint8_t* nodes /* num_nodes*32 */, size_t num_nodes, int* ok, double* device_ms);
/* the expansion: the `count` full authentication paths in dst_rtree_path's layout, in the order of `indices` -- what dst_rescue_path_tapes and
 * the path checks take -- and the root they resolve to (to be held against the root the caller trusts).  device >= 0: the level launches of
 * dst_rescue_multiproof_root, one gather launch, one copy back. */
DST_API int dst_rescue_multiproof_paths(int device, uint32_t n, const uint64_t* indices, const uint8_t* leaves /* count*32 */, size_t count,
                                        const uint8_t* nodes /* num_nodes*32 */, size_t num_nodes, uint8_t* paths /* count*n*32 */, uint8_t root[32],
                                        double* device_ms);
DST_API void dst_rtree_destroy(dst_rtree* t);
DST_API const char* dst_rtree_last_error(const dst_rtree* t);     /* t may be NULL: the error of the calling thread's last failed dst_rtree_build / dst_rtree_load / dst_rescue_digest_many / dst_rescue_path_tapes / dst_rescue_path_roots / dst_rescue_verify_* / dst_rescue_multiproof_* */

/* ---- sparse Rescue Merkle trees: a set addressed by keys of up to 63 bits (accounts, notes, nullifiers) ------------------------------------
 * A sparse tree of depth D, 1 <= D <= 63, IS the dense tree above over 2^D leaves in which every leaf that was never set holds the tree's empty
 * leaf (two canonical elements given at creation, (0, 0) by default): same parents, same roots, same paths, so smpath.n / pmpath.n with
 * n = D + 1 <= 64 authenticate them.  Level D is the leaf level, level 0 the root; E_D = the empty leaf and E_l = digest(E_{l+1}, E_{l+1}) is
 * every empty subtree of level l.  Only nodes with a set leaf below them are stored: per level l a list sorted by prefix, the distinct
 * key >> (D - l) and their node values.  A key set to the empty value stays stored (its nodes then equal the defaults, so roots do not depend
 * on it) until dst_stree_compact drops it; dst_stree_remove deletes keys outright.  Either way the nodes left without a key below them go too,
 * and what remains is, level by level, the tree that create + one set of the remaining keys makes.  A tree without keys has root E_0.  The reference has no such structure (it walks "a pseudo-random path
 * through an imaginary tree", src/examples/merkle.rs:96-108).
 * The conventions are dst_rtree's: no dst_ctx; device >= 0 on that GPU with a stream the tree owns, device < 0 on the host with one thread and
 * no HIP call; DST_ERR_ARG is found on the host before anything is queued and leaves the tree unchanged; a HIP error inside a call that changes
 * the tree (set, apply, remove, compact) leaves it unusable (DST_ERR_STATE from everything but destroy and last_error). */
typedef struct dst_stree dst_stree;
DST_API int dst_stree_create(int device, uint32_t depth, const uint8_t empty_leaf[32] /* NULL: (0, 0) */, dst_stree** out);
/* inserts the keys that are not stored and replaces those that are: `count` distinct indices below 2^depth in any order, count * 32 bytes of
 * leaves.  Afterwards every stored node equals that of a tree created fresh and set once with the union (the later value of a key wins).  One
 * digest per distinct ancestor of the touched keys -- the sum over the levels l < depth of the number of distinct index >> (depth - l) -- and no
 * more; untouched nodes are carried over, never hashed again (moving them costs O(stored nodes)).  Building a tree is create + one set.
 * DST_ERR_ARG: a repeated index, an index past the end, an element not below p, a null pointer with count > 0, more than 2^32 - 2 stored nodes.
 * count = 0: DST_OK. */
DST_API int dst_stree_set(dst_stree* t, const uint64_t* indices, const uint8_t* leaves /* count*32 */, size_t count);
/* deletes the stored keys among `count` distinct indices below 2^depth (any order) and ignores the others; *removed (may be NULL) = how many
 * were stored.  A node with no stored key below it is no longer stored; an ancestor of a removed key that still has one is hashed again, a side
 * without keys being its level's E_l; no other node is hashed.  last_digests = the number of those surviving ancestors.  The root is that of the
 * dense tree with the empty leaf at the removed positions; removing every key gives the tree without keys (root E_0, 0 nodes), usable again.
 * On a device tree: one carry-over launch, one level launch per level that keeps a touched parent, one synchronisation; node values never
 * travel to the host.  DST_ERR_ARG: a repeated index, an index past the end, a null pointer with count > 0.  count = 0, or no index stored:
 * DST_OK, the tree is unchanged, last_digests = 0. */
DST_API int dst_stree_remove(dst_stree* t, const uint64_t* indices, size_t count, uint64_t* removed /* may be NULL */);
/* deletes every stored key whose leaf equals the empty leaf -- what dst_stree_set / dst_stree_apply with the empty value leave behind -- and every
 * node left without a key below it; *removed (may be NULL) = how many keys.  The root and every remaining node are unchanged (a stored empty
 * side and an absent side hash alike), so no digest is computed: last_digests = 0.  On a device tree: one launch that flags those leaves, a
 * copy back of one byte per stored key, one carry-over launch.
 * WITNESSED REMOVAL is dst_stree_apply with empty leaves -- per write the path and the root after it, which dst_rescue_verify_writes checks --
 * followed by dst_stree_compact, which frees the nodes. */
DST_API int dst_stree_compact(dst_stree* t, uint64_t* removed /* may be NULL */);
/* the leaf at each of `count` indices below 2^depth (repeats allowed): 32 bytes per index where dst_stree_paths returns 32 * (depth + 1).  An
 * index that is not stored gives the empty leaf and stored[i] = 0.  On a device tree: one upload, one launch, one copy back, whatever count is. */
DST_API int dst_stree_get(const dst_stree* t, const uint64_t* indices, size_t count,
                          uint8_t* leaves /* count*32 */, uint8_t* stored /* count bytes of 0 / 1, may be NULL */);
DST_API int dst_stree_root(const dst_stree* t, uint8_t root[32]);
/* authentication paths [leaf, sibling, uncle, ...] of `count` indices below 2^depth, stored or not (repeats allowed), (depth + 1) * 32 bytes
 * each in dst_rtree_path's layout: compute_merkle_root (merkle.rs:112-145) of the path and the index gives the root.  A leaf or sibling that is
 * not stored is the E_l of its level; a path whose leaf is E_depth proves that the key is empty.  On a device tree: one upload, one launch, one
 * copy back, whatever count is. */
DST_API int dst_stree_paths(const dst_stree* t, const uint64_t* indices, size_t count, uint8_t* paths /* count*(depth+1)*32 */);
/* dst_rtree_multiproof with n = depth + 1 for `count` distinct keys below 2^depth, stored or not: an unstored leaf or sibling is the E_l of its
 * level, as in dst_stree_paths, so absent keys are proven by the same call.  On a device tree: one upload, one lookup launch, one copy back. */
DST_API int dst_stree_multiproof(const dst_stree* t, const uint64_t* indices, size_t count, uint8_t* leaves /* count*32 */,
                                 uint8_t* nodes /* cap_nodes*32, or NULL */, size_t cap_nodes, size_t* num_nodes);
/* dst_rtree_apply on a sparse tree: ordered writes to keys below 2^depth, stored or not, repeats allowed; paths of depth + 1 nodes.  The old leaf
 * of a key that is not stored before operation i is E_depth, a sibling subtree without keys the E_l of its level.  Afterwards the tree is what
 * dst_stree_set makes of the distinct keys with the later value of each (a key written with the empty value stays stored).  On a device tree: depth
 * level launches compute every witness against the stored generation, then that one set runs; last_digests = count * depth + the set's digests,
 * last_device_ms the sum of both.  DST_ERR_ARG as dst_rtree_apply, and a device tree that would pass 2^31 - 2 stored nodes. */
DST_API int dst_stree_apply(dst_stree* t, const uint64_t* indices, const uint8_t* leaves /* count*32 */, size_t count,
                            uint8_t* paths /* count*(depth+1)*32, or NULL */, uint8_t* roots /* count*32, or NULL */);
/* dst_rtree_tapes_many with n = depth + 1: the same `what`, the same size query */
DST_API int dst_stree_tapes_many(const dst_stree* t, const uint64_t* indices, size_t count, uint32_t what,
                                 uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each);
/* `count` entries from `first` of level `level`'s sorted list: the prefixes and / or the nodes (either may be NULL); *level_count (may be NULL)
 * always receives the level's length.  How a host sees every node, and how it persists a tree. */
DST_API int dst_stree_read_level(const dst_stree* t, uint32_t level, uint64_t first, uint64_t count,
                                 uint64_t* prefixes, uint8_t* nodes /* count*32 */, uint64_t* level_count);
typedef struct dst_stree_info_t {
    uint32_t depth;
    int32_t device;                     /* -1: a host tree */
    uint64_t keys, nodes;               /* stored keys; stored nodes of all levels, the leaves included */
    uint64_t last_digests;              /* digests computed by the last dst_stree_set / dst_stree_apply / dst_stree_remove / dst_stree_compact */
    double last_device_ms;              /* events around that call's level launches, as dst_rtree_update_ms; 0 on a host tree */
} dst_stree_info_t;
DST_API int dst_stree_info(const dst_stree* t, dst_stree_info_t* out);

/* ---- save, restore and audit: a tree survives a restart without being hashed again ------------------------------------------------------------
 * THE BLOB is little-endian and self-describing, and byte-identical whether a host tree or a device tree wrote it:
 *   header, 64 bytes:  8 bytes of magic "DSTTREE1" (the last byte is the version digit) | u32 kind: 1 = dense, 2 = sparse | u32 depth: log_leaves
 *                      of a dense tree, the depth of a sparse one | 32 bytes of empty leaf, all zero in a dense blob | u64 number of keys (2^log_leaves
 *                      in a dense blob) | u64 number of stored nodes;
 *   dense body:        the 2^(log_leaves+1) - 1 nodes of heap positions 1 and up, 32 bytes each: the bytes of dst_rtree_read_nodes(t, 1, ...);
 *   sparse body:       depth + 1 level lengths as u64, then every level's sorted prefixes as u64, then every level's nodes, 32 bytes each.  All
 *                      three run in the order the tree keeps its levels -- the leaf level (depth) first, the root level (0) last -- so saving
 *                      is a copy.  A key stored with the empty value stays stored.  The E_l are not in the blob: load derives them from the empty
 *                      leaf as dst_stree_create does.
 * The length must be exactly what the header implies: 64 + 32 * nodes (dense), 64 + 8 * (depth + 1) + 40 * nodes (sparse).
 * SAVE: out == NULL is the size query; *len always receives the length; DST_ERR_ARG when cap is smaller.  The tree is unchanged.
 * LOAD takes untrusted bytes and refuses with DST_ERR_ARG, before anything is allocated: a short blob or trailing bytes, a wrong magic, version
 * or kind, a depth outside 1..26 (dense) / 1..63 (sparse), counts that disagree with the depth or with each other, an element -- the empty leaf
 * included -- that is not below p, and any sparse shape that create + set could not have made: prefixes of a level not strictly ascending or not
 * below 2^level, level l not exactly the distinct prefix >> 1 of level l + 1, more than one root, a leaf level whose length is not the key count,
 * 2^32 - 1 stored nodes or more.  *out is NULL after any refusal and nothing stays allocated; the reason is dst_rtree_last_error(NULL) /
 * dst_stree_last_error(NULL).  A sparse blob without keys is valid: the tree with root E_0.
 * With audit == 0 load hashes NOTHING (a sparse load computes the depth digests E_l on the host, as create does): one allocation, the upload
 * of the nodes straight from the caller's blob (a sparse tree's two small tables and its prefixes beside them), no digest launch, no second copy
 * of the blob in host memory; dst_rtree_build_ms and last_digests then read 0.  A TREE LOADED WITHOUT AUDIT IS ONLY AS GOOD AS ITS BLOB: the shape is
 * checked, the node values are believed.  With audit != 0 the audit below runs before the tree is handed out; a bad node is DST_ERR_ARG, *out is
 * NULL and the error text names the node ("audit: node 5 ...", "audit: the node of level 3 with prefix 5 ...").  A caller that wants the
 * location in numbers loads without audit and calls the audit itself.  A loaded tree is a full tree: update, apply, set, remove, compact,
 * paths, tapes and multiproofs work on it as on a built one.
 * AUDIT checks that every stored parent is the digest of its two children, on built and on loaded trees, and leaves the tree unchanged.  The
 * work of a build, but no level waits for the one below: on a device tree it is ONE launch over all parents of all levels, whatever the depth.
 * Dense: *first_bad = the lowest heap position p in [1, 2^log_leaves) whose node differs from digest(node[2p], node[2p+1]), -1 when there is
 * none.  Sparse: every stored node of a level l < depth must equal the digest of its children at level l + 1, a child that is not stored being
 * E_{l+1}; the bad parent nearest the root is reported, within its level the one of the lowest prefix; *bad_level = -1 (and *bad_prefix = 0)
 * when there is none.  A bad node is NOT an error: the call returns DST_OK.  *device_ms (may be NULL): events around the launch, 0 on the host. */
DST_API int dst_rtree_save(const dst_rtree* t, uint8_t* out /* cap bytes, or NULL */, size_t cap, size_t* len);
DST_API int dst_rtree_load(int device, const uint8_t* blob, size_t len, uint32_t audit, dst_rtree** out);
DST_API int dst_rtree_audit(const dst_rtree* t, int64_t* first_bad, double* device_ms /* may be NULL */);
DST_API int dst_stree_save(const dst_stree* t, uint8_t* out /* cap bytes, or NULL */, size_t cap, size_t* len);
DST_API int dst_stree_load(int device, const uint8_t* blob, size_t len, uint32_t audit, dst_stree** out);
DST_API int dst_stree_audit(const dst_stree* t, int32_t* bad_level, uint64_t* bad_prefix, double* device_ms /* may be NULL */);
DST_API void dst_stree_destroy(dst_stree* t);
DST_API const char* dst_stree_last_error(const dst_stree* t);     /* t may be NULL: the error of the calling thread's last failed dst_stree_create / dst_stree_load */

/* ---- wide-key sparse Rescue Merkle trees: keys of up to 127 bits, depth up to 127 --------------------------------------------------------------
 * The keys of accounts, notes and nullifiers are hashes.  Cut down to the 63 bits of a dst_stree key, two of them collide after about 2^31.5
 * insertions; at 127 bits the birthday bound is 2^63.  A dst_wtree is the sparse tree above with 16-byte keys and 1 <= depth <= 127: the same
 * definition (the dense tree over 2^depth leaves with the empty leaf wherever nothing was set), the same parents, the same E_l, the same path
 * layout [leaf, sibling, uncle, ...], the same tapes, so smpath.n / pmpath.n with n = depth + 1 <= 128 authenticate it.
 * WHY 127 AND NOT 255: pmpath rebuilds the index with binacc into ONE field element, so every index must stay below p, and 2^127 < p =
 * 2^128 - 45 * 2^40 + 1 holds where 2^128 does not; up to depth 127 both smpath and pmpath authenticate the tree, and index + 2^(n-1), the tape
 * rule (merkle.rs:68), still fits in 128 bits.
 * A KEY, an index or a prefix is 16 bytes, a little-endian integer: the memory image of a u128 and the layout of a field element, at any
 * alignment.  A key must be below 2^depth as a whole -- one that violates this only in its high 8 bytes is refused -- and "repeated" compares
 * all 128 bits: two keys with equal low halves and different high halves are two keys.
 * THE LIMIT ON STORED NODES stays 2^32 - 2 (2^31 - 2 for dst_wtree_apply on a device tree), because flat positions are 32 bits; a random
 * 127-bit key stores about 110 nodes of its own, so a tree holds some 3.9e7 such keys.
 * Each call has the semantics, the argument checks (DST_ERR_ARG, found on the host before anything is queued, the tree unchanged), the host
 * path for device < 0, the launch count per call, the last_digests and last_device_ms, and the rule that a HIP error inside a call that changes
 * the tree leaves it unusable, of the dst_stree_* call of the same name; dst_wtree_info fills a dst_stree_info_t.  Beyond those, DST_ERR_ARG:
 * more than 2^40 keys in one call.  Multiproofs, plain and compact, and save / load follow below the path tools. */
typedef struct dst_wtree dst_wtree;
DST_API int dst_wtree_create(int device, uint32_t depth /* 1 .. 127 */, const uint8_t empty_leaf[32] /* NULL: (0, 0) */, dst_wtree** out);   /* dst_stree_create */
DST_API int dst_wtree_set(dst_wtree* t, const uint8_t* keys /* count*16 */, const uint8_t* leaves /* count*32 */, size_t count);              /* dst_stree_set */
DST_API int dst_wtree_remove(dst_wtree* t, const uint8_t* keys /* count*16 */, size_t count, uint64_t* removed /* may be NULL */);            /* dst_stree_remove */
DST_API int dst_wtree_compact(dst_wtree* t, uint64_t* removed /* may be NULL */);                                                            /* dst_stree_compact */
DST_API int dst_wtree_get(const dst_wtree* t, const uint8_t* keys /* count*16 */, size_t count,
                          uint8_t* leaves /* count*32 */, uint8_t* stored /* count bytes of 0 / 1, may be NULL */);                           /* dst_stree_get */
DST_API int dst_wtree_root(const dst_wtree* t, uint8_t root[32]);                                                                            /* dst_stree_root */
DST_API int dst_wtree_paths(const dst_wtree* t, const uint8_t* keys /* count*16 */, size_t count, uint8_t* paths /* count*(depth+1)*32 */);   /* dst_stree_paths */
DST_API int dst_wtree_apply(dst_wtree* t, const uint8_t* keys /* count*16 */, const uint8_t* leaves /* count*32 */, size_t count,
                            uint8_t* paths /* count*(depth+1)*32, or NULL */, uint8_t* roots /* count*32, or NULL */);                        /* dst_stree_apply */
DST_API int dst_wtree_tapes_many(const dst_wtree* t, const uint8_t* keys /* count*16 */, size_t count, uint32_t what,
                                 uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each);                               /* dst_stree_tapes_many */
DST_API int dst_wtree_read_level(const dst_wtree* t, uint32_t level, uint64_t first, uint64_t count,
                                 uint8_t* prefixes /* count*16 */, uint8_t* nodes /* count*32 */, uint64_t* level_count);                    /* dst_stree_read_level */
DST_API int dst_wtree_info(const dst_wtree* t, dst_stree_info_t* out);                                                                       /* dst_stree_info */
/* dst_stree_audit; bad_prefix receives 16 bytes, all zero when no parent is bad */
DST_API int dst_wtree_audit(const dst_wtree* t, int32_t* bad_level, uint8_t bad_prefix[16], double* device_ms /* may be NULL */);
/* test build only (the product library answers DST_ERR_STATE): overwrites entry `index` of level `level`'s node list and hashes nothing, so that an
 * audit has something to find */
DST_API int dst_wtree_test_set_node(dst_wtree* t, uint32_t level, uint64_t index, const uint8_t node[32]);
DST_API void dst_wtree_destroy(dst_wtree* t);
DST_API const char* dst_wtree_last_error(const dst_wtree* t);     /* t may be NULL: the error of the calling thread's last failed dst_wtree_create / dst_wtree_load */
/* the path tools without a tree over 16-byte indices: 2 <= n <= 128, indices[i] below 2^(n-1) as a whole; everything else -- arguments, verdicts,
 * `why`, first_bad, the one launch of a device >= 0 call, device_ms, errors filed with dst_rtree_last_error(NULL) -- as dst_rescue_path_roots,
 * dst_rescue_verify_paths, dst_rescue_verify_writes and dst_rescue_path_tapes.  The direction bit of level k is bit k of the whole index. */
DST_API int dst_rescue_path_roots_w(int device, const uint8_t* paths /* count*n*32 */, uint32_t n, const uint8_t* indices /* count*16 */, size_t count,
                                    const uint8_t* leaves /* count*32, or NULL */, uint8_t* roots /* count*32 */, double* device_ms);
DST_API int dst_rescue_verify_paths_w(int device, const uint8_t root[32], const uint8_t* paths /* count*n*32 */, uint32_t n, const uint8_t* indices /* count*16 */,
                                      const uint8_t* leaves /* count*32, or NULL */, size_t count, int64_t* first_bad, uint32_t* why, double* device_ms);
DST_API int dst_rescue_verify_writes_w(int device, const uint8_t root_before[32], const uint8_t* paths /* count*n*32 */, uint32_t n, const uint8_t* indices /* count*16 */,
                                       const uint8_t* leaves /* count*32 */, const uint8_t* roots /* count*32, or NULL */, size_t count, int64_t* first_bad,
                                       uint32_t* why, uint8_t root_after[32] /* may be NULL */, double* device_ms);
DST_API int dst_rescue_path_tapes_w(const uint8_t* paths /* count*n*32 */, uint32_t n, const uint8_t* indices /* count*16 */, size_t count, uint32_t what,
                                    uint8_t* tape_a, uint8_t* tape_b, size_t cap_elems_each, size_t* elems_each);
/* dst_rescue_refresh_paths over 16-byte little-endian indices and held indices, 2 <= n <= 128: the witnesses of dst_wtree_apply */
DST_API int dst_rescue_refresh_paths_w(int device, const uint8_t root_before[32], const uint8_t* paths /* count*n*32 */, uint32_t n, const uint8_t* indices /* count*16 */,
                                       const uint8_t* leaves /* count*32 */, const uint8_t* roots /* count*32, or NULL */, size_t count,
                                       const uint8_t* held_indices /* held*16 */, const uint8_t* held_paths /* held*n*32 */, size_t held,
                                       uint8_t* out_paths /* held*n*32; may be held_paths itself */,
                                       int64_t* first_bad, uint32_t* why, uint8_t root_after[32] /* may be NULL */, double* device_ms);

/* ---- multiproofs of wide trees, plain and COMPACT ------------------------------------------------------------------------------------------------
 * The multiproof above over 16-byte indices and 2 <= n <= 128: the same node set, the same order (level n - 1 first, ascending by position within
 * a level), M and `digests` as dst_rescue_multiproof_size counts them.  A path of a deep sparse tree is mostly empty subtrees -- of the 118 nodes per key that a
 * plain proof of 256 keys of a 2^20-key tree of depth 127 supplies, 11.5 are stored (profiles/rescue_tree.md, "Wide batch proofs and restore") --
 * so the wide calls also have a COMPACT form that neither ships such a sibling nor hashes a parent of two empty subtrees:
 *   absent_bits, ceil(M / 8) bytes: bit m (bit m & 7 of byte m >> 3; padding bits 0) is set when supplied node m is NOT STORED in the tree; `nodes`
 *   then holds only the S = M - popcount stored ones, in the same order.  "Not stored" is by absence, not by value, so a host tree and a device
 *   tree give the same bits: a key stored with the empty value has stored ancestors until dst_wtree_compact.
 *   empties, n*32 bytes: E_0 .. E_{n-1}, the value of an empty subtree of every level (dst_rescue_empty_nodes), which the checking side computes
 *   once per (empty leaf, depth).  THE TABLE IS BELIEVED: a check with a wrong table checks against another tree; compute it, do not receive it.
 * A leaf is known-empty when its 32 bytes equal E_{n-1}, a supplied node when its bit is set, a parent exactly when both children are; such a
 * parent is E_l of its level and is never hashed.  *digests = the parents actually computed; a proof in which everything is known-empty resolves
 * to E_0 with 0 digests and no launch.  With absent_bits == NULL a call is the plain form: `nodes` holds all M, empties must be NULL.
 * dst_rescue_empty_nodes (host only): out[32 l ..) = E_l for l = 0 .. n - 1 with E_{n-1} = the empty leaf, the chain dst_wtree_create computes.
 * dst_wtree_multiproof: the leaves of `count` distinct keys below 2^depth, stored or not (an absent key has the leaf E_depth: absence is proven
 * by the same call), and the supplied nodes.  absent_bits == NULL: plain, *num_nodes = M, byte-equal to dst_stree_multiproof wherever both
 * trees exist.  Otherwise compact: absent_bits receives the bits, nodes the S stored nodes, *num_nodes = S.  *total (may be NULL) = M.  nodes ==
 * NULL is the size query (a compact one looks the nodes up; absent_bits is then not written).  DST_ERR_ARG as dst_stree_multiproof.  On a device
 * tree at most two launches whatever count is: one locates the count + M nodes in the level lists and leaves their flat positions on the device
 * -- the host receives 4 bytes per node -- and one packs the stored leaves and nodes, which alone come back; no E_l crosses the bus, and a tree
 * without nodes launches nothing.
 * dst_rescue_multiproof_root_w / dst_rescue_verify_multiproof_w / dst_rescue_multiproof_paths_w: the narrow calls with absent_bits and empties
 * behind num_nodes.  DST_ERR_ARG, found on the host before anything is queued, beyond the narrow calls': num_nodes != M - popcount(absent_bits)
 * (plain: != M), a nonzero padding bit, absent_bits without empties or empties without absent_bits, an element of empties not below p.  device
 * >= 0: one upload (the table with it), one launch per level THAT HAS A JOB, one gather launch for the expansion, one synchronisation, one copy
 * back; device < 0: the same plan on the host.  dst_rescue_multiproof_last_levels: how many levels had a job in the calling thread's last
 * successful dst_rescue_multiproof_root* / verify_multiproof* / multiproof_paths* call.  Errors: dst_rtree_last_error(NULL). */
DST_API int dst_rescue_empty_nodes(const uint8_t empty_leaf[32] /* NULL: (0, 0) */, uint32_t n /* 2 .. 128 */, uint8_t* out /* n*32 */);
DST_API int dst_rescue_multiproof_size_w(uint32_t n, const uint8_t* indices /* count*16 */, size_t count, size_t* num_nodes, uint64_t* digests);
DST_API int dst_wtree_multiproof(const dst_wtree* t, const uint8_t* keys /* count*16 */, size_t count, uint8_t* leaves /* count*32 */,
                                 uint8_t* nodes /* cap_nodes*32, or NULL */, size_t cap_nodes, size_t* num_nodes,
                                 uint8_t* absent_bits /* ceil(M/8) bytes, or NULL */, size_t* total /* may be NULL */);
DST_API int dst_rescue_multiproof_root_w(int device, uint32_t n, const uint8_t* indices /* count*16 */, const uint8_t* leaves /* count*32 */, size_t count,
                                         const uint8_t* nodes /* num_nodes*32 */, size_t num_nodes, const uint8_t* absent_bits /* or NULL */,
                                         const uint8_t* empties /* n*32, or NULL */, uint8_t root[32], uint64_t* digests /* may be NULL */, double* device_ms /* may be NULL */);
DST_API int dst_rescue_verify_multiproof_w(int device, const uint8_t root[32], uint32_t n, const uint8_t* indices /* count*16 */, const uint8_t* leaves /* count*32 */,
                                           size_t count, const uint8_t* nodes /* num_nodes*32 */, size_t num_nodes, const uint8_t* absent_bits /* or NULL */,
                                           const uint8_t* empties /* n*32, or NULL */, int* ok, double* device_ms /* may be NULL */);
DST_API int dst_rescue_multiproof_paths_w(int device, uint32_t n, const uint8_t* indices /* count*16 */, const uint8_t* leaves /* count*32 */, size_t count,
                                          const uint8_t* nodes /* num_nodes*32 */, size_t num_nodes, const uint8_t* absent_bits /* or NULL */,
                                          const uint8_t* empties /* n*32, or NULL */, uint8_t* paths /* count*n*32 */, uint8_t root[32], double* device_ms /* may be NULL */);
DST_API uint32_t dst_rescue_multiproof_last_levels(void);
/* save / load of a wide tree: dst_stree_save / dst_stree_load with BLOB KIND 3 -- the header of kind 2 with depth 1 .. 127, then depth + 1 level
 * lengths as u64, every level's prefixes as 16-byte little-endian integers, every level's nodes, the leaf level first; exactly 64 + 8 * (depth +
 * 1) + 48 * nodes bytes, the same from a host tree and a device tree.  Load refuses what dst_stree_load refuses, comparing all 128 bits of a
 * prefix, and the kinds 1 and 2 (dst_stree_load refuses kind 3); audit == 0 hashes nothing, audit != 0 runs dst_wtree_audit and names a bad node
 * in the text.  Failures of load: dst_wtree_last_error(NULL). */
DST_API int dst_wtree_save(const dst_wtree* t, uint8_t* out /* cap bytes, or NULL */, size_t cap, size_t* len);
DST_API int dst_wtree_load(int device, const uint8_t* blob, size_t len, uint32_t audit, dst_wtree** out);

/* ---- host-side helpers that the Rust host would otherwise take from `rand` (they run on the CPU) -------------------- */
DST_API void dst_prng_vector(const uint8_t seed[32], uint32_t count, uint8_t* out /* count*16 */);          /* field.rs:271 */
DST_API int dst_query_positions(const uint8_t seed[32], uint64_t domain_size, uint32_t blowup, uint32_t num_queries, uint64_t* out); /* utils/mod.rs:25 */
DST_API void dst_blake3(const uint8_t* in, size_t len, uint8_t out[32]);                                     /* crypto/hash.rs:205 (host) */

/* ---- benchmark inputs: the Fibonacci example trace (src/examples/fibonacci.rs:32-47) filling exactly 2^log_n rows
 * (W = 20, ctx_depth 1, loop_depth 0).  cols = [20][n] elements; outputs the program hash and the result. -------------- */
DST_API int dst_fibonacci_trace(uint32_t log_n, uint8_t* cols, uint8_t program_hash[32], uint8_t result[16]);

/* ---- coset-sharded proving on several GPUs (one context per GPU, params.rank / params.world) ----------
 * The phases mirror the single-GPU ones; collectives are issued by the host between them.  `what`: 0 trace-tree boundary
 * nodes, 1 constraint-tree boundary nodes, 2 FRI-tree boundary nodes of (sharded) layer `arg`, 3 combined constraint evaluations,
 * 4 last FRI layer (remainder: all of it, natural order, after the commit phase), 5 size query only: the largest item
 * dst_shard_fri_begin hands out.  dst_shard_import takes the all-gathered items of all ranks (rank-major); for trees it
 * finishes the replicated upper levels and returns the root.  *_is_device: the pointer is device memory (possibly owned
 * by another HIP runtime instance in the process, e.g. a torch tensor) instead of host memory. */
DST_API int dst_shard_commit_trace(dst_ctx* ctx);
DST_API int dst_shard_eval_constraints(dst_ctx* ctx, const dst_public* pub, const uint8_t* coeffs /* 344*16 */, int64_t* bad_step);
DST_API int dst_shard_combine(dst_ctx* ctx);
DST_API int dst_shard_fri_layer(dst_ctx* ctx, int* more);
DST_API int dst_shard_fri_fold(dst_ctx* ctx, const uint8_t special_x[16]);
DST_API int dst_shard_export_size(dst_ctx* ctx, uint32_t what, uint32_t arg, size_t* bytes);
DST_API int dst_shard_export(dst_ctx* ctx, uint32_t what, uint32_t arg, void* dst, int dst_is_device);
DST_API int dst_shard_import(dst_ctx* ctx, uint32_t what, uint32_t arg, const void* src, int src_is_device, uint8_t root_out[32]);
/* openings: `count` items by LOCAL index from buffer 0 trace leaves, 1 trace local nodes, 2 trace upper nodes, 3 constraint
 * evaluations (elements), 4 constraint local nodes, 5 constraint upper nodes, 6 FRI layer `arg` evaluations (elements), 7 FRI leaves,
 * 8 FRI local nodes, 9 FRI upper nodes, 10 LDE rows (idx = natural positions owned by this rank, W elements each), 11 transition
 * evaluations of the last dst_eval_constraints / dst_shard_eval_constraints (elements; this rank's cosets of the 8n-point domain,
 * coset-major: index q * n + k is the point 8k + q on one GPU).  The element buffers 3, 6 (sharded layers) and 11 are coset-major. */
DST_API int dst_shard_read(dst_ctx* ctx, uint32_t buffer, uint32_t arg, const uint64_t* idx, uint32_t count, uint8_t* out);
/* The FRI commit phase (fri/prover.rs:11-53): call dst_shard_fri_begin, all-gather the *bytes it wrote into `send` (same size
 * on every rank), call dst_shard_fri_end with the gathered bytes (rank-major); repeat while *more.  Large layers stay sharded:
 * begin = leaves + rank-local tree levels + export of the boundary nodes, end = upper tree, root, fold at field::prng(root).
 * From the first layer of at most 2^17 elements (or with fewer than one 4-element row per coset) begin hands out the rank's
 * cosets of the layer's EVALUATIONS instead (*more = 0) and end commits that layer and all following ones on every rank by
 * itself (replicated tail: no further exchanges).  dst_shard_fri_roots then returns the roots of all layers. */
DST_API int dst_shard_fri_begin(dst_ctx* ctx, void* send, int send_is_device, size_t cap, size_t* bytes, int* more);
DST_API int dst_shard_fri_end(dst_ctx* ctx, const void* gathered, int src_is_device, uint8_t root_out[32]);
DST_API int dst_shard_fri_roots(dst_ctx* ctx, uint8_t* roots /* 32 per layer, or NULL */, size_t cap, uint32_t* num_layers, uint32_t* replicated_from);

/* Step 9 across ranks (prover.rs:143-165; merkle.rs:64-124 prove_batch; fri/prover.rs:55-96 build_proof).  Every rank derives the
 * same ordered list of openings from the query positions.  dst_shard_open returns the items THIS rank owns, concatenated in that
 * order (blob == NULL: only the sizes; all_lens, if not NULL, receives every rank's blob length, `world` entries);
 * dst_shard_assemble takes the blobs of all ranks back to back (blob_lens[g] bytes each) and writes the serialised StarkProof
 * (proof.rs:11-77, bincode as src/main.rs:44) -- identical bytes on every rank. */
DST_API int dst_shard_open(dst_ctx* ctx, const uint64_t* positions, uint32_t num_positions, uint8_t* blob, size_t cap, size_t* blob_len, uint64_t* all_lens);
DST_API int dst_shard_assemble(dst_ctx* ctx, const uint64_t* positions, uint32_t num_positions, uint64_t pow_nonce, const uint8_t* blobs,
                       const uint64_t* blob_lens, uint8_t* out, size_t cap, size_t* out_len);
DST_API int dst_shard_info(dst_ctx* ctx, uint64_t* op_count, uint32_t* num_fri_layers, uint32_t* stack_depth);

/* ---- inspection (tests and profiling): copies an internal device buffer to the host.  `what` ids are listed in
 * distaff_amd/csrc/ctx.h (DST_BUF_*).  Two-call protocol: out = NULL returns the size through *len. ------------------- */
DST_API int dst_read_buffer(dst_ctx* ctx, uint32_t what, uint32_t arg, uint8_t* out, size_t cap, size_t* len);
/* 1: this is the test / bench build (libdistaff_hip_hooks.so: calibration kernels, the alternative formulations behind the test-only
 * DISTAFF_* switches of INTEGRATION.md section 6); 0: the product library, which has neither */
DST_API int dst_test_hooks(void);
/* micro-benchmark hook used by bench.py's roofline section: runs `iters` dependent modular multiplications per lane
 * on `lanes` lanes and returns the elapsed milliseconds.  (Test / bench build only: the product library returns DST_ERR_STATE.) */
DST_API int dst_bench_mulmod(dst_ctx* ctx, uint64_t lanes, uint32_t iters, double* ms);
/* peak of the 32x32+64 multiply-add (v_mad_u64_u32) on this device: `iters` iterations of 32 independent-enough mads per lane on
 * `lanes` lanes; returns the elapsed milliseconds (rate = lanes * iters * 32 / time).  The integer-multiplier roofline of the path.
 * (Test / bench build only: the product library returns DST_ERR_STATE.) */
DST_API int dst_bench_mad(dst_ctx* ctx, uint64_t lanes, uint32_t iters, double* ms);
/* the shader clock (MHz) the device sustains under this path's arithmetic: `iters` iterations of four dependent modular multiplications per lane
 * on `lanes` lanes, every wavefront timing itself with s_memtime against the constant 100 MHz s_memrealtime; the median.  The power management
 * does not hold the nominal clock under this load (profiles/r6_power_clock.md).  (Test / bench build only: the product library returns DST_ERR_STATE.) */
DST_API int dst_bench_clock(dst_ctx* ctx, uint64_t lanes, uint32_t iters, double* mhz);
/* box fingerprint: milliseconds for 2^23 lanes to run `code_kib` (16 or 176) KiB of straight-line multiply-adds once each.  The ratio
 * of the two times per instruction is 0.9 on a healthy device; a device on which code beyond the instruction cache is slow shows it here.
 * code_kib = 177: the 176 KiB kernel in its convoy form (256 lanes per workgroup, a workgroup barrier every 16 KiB: the wavefronts share
 * their instruction-cache lines) -- whether that form would help on the device at hand.
 * (Test / bench build only: the product library returns DST_ERR_STATE.) */
DST_API int dst_bench_code(dst_ctx* ctx, uint32_t code_kib, double* ms);
/* element-wise device field arithmetic on caller data (tests): op 0 add, 1 sub, 2 mul, 3 mul (portable formulation), 4 inv(a), 5 a^b,
 * 6 sum_{j<40} a[(i+j) % count] * b[(i+7j) % count] + a[i] with one reduction, 7 a * b as a multiplication by the table entry
 * (b, b * 2^64) (a: any 128-bit value, b canonical), 8 a * 2^64, 9 / 10 the sum / the difference of one sum-and-difference pair,
 * 11 a * (low 32 bits of b), 12 a^2, 13 a^3, 256 + T (T = 1 .. 64): the sum of op 6 over T terms instead of 40.  Every operation is one
 * call of the device function on the operands as given (no check that they are canonical); any other op is DST_ERR_ARG. */
DST_API int dst_field_op(dst_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t count);
/* per-kernel timing with HIP events on the context's stream.  level 0: off; 1: every kernel launch is bracketed (costs ~5 % of a
 * proof: ~300 launches lose their back-to-back issue); 2: only the heavy kernels (NTT passes, constraint kernel, leaf hashing:
 * ~35 launches, ~90 % of the device time, no measurable cost).  dst_kernel_stats drains the events and writes a JSON object
 * {"kernel": {"launches": k, "ms": total, "bytes": algorithmic}, ...}. */
DST_API int dst_set_profiling(dst_ctx* ctx, int level);
DST_API int dst_kernel_stats(dst_ctx* ctx, char* json_out, size_t cap, int reset);

/* ---- one proof over several GPUs, collectives behind the C-ABI -------------------------------------------------------------------
 * The reference has no multi-device path (src/math/polynom.rs:36-37); the partitioning follows SURVEY.md 8(e): rank g of `world` owns
 * the cosets [g*B/world, (g+1)*B/world) of every extension, Merkle trees are finished from an all-to-all of boundary nodes (rank g
 * builds the subtree over the trace indices k in [g*n/world, (g+1)*n/world)), an all-gather of the `world` subtree roots and the top
 * log2(world) levels; constraint evaluations and the first small FRI layer are all-gathered.  No all-reduce anywhere.
 *
 * One communicator handle per rank.  RCCL transport (one process per GPU, xGMI): the rank-0 host calls dst_comm_unique_id and hands
 * the 128 bytes to the other ranks through its own channel; every rank then calls dst_comm_init with the device it created its
 * context on.  librccl.so is bound at run time, a single-GPU host never needs it.  In-process transport (dst_comm_init_local fills
 * `world` handles): the ranks are threads of one process, e.g. a host that drives all GPUs of a node itself, or tests; stream-ordered like
 * RCCL -- a collective is enqueued on the ranks' streams (events between them, device-to-device copies over peer access), the host threads
 * only hand over pointers and never wait for a stream (DISTAFF_LOCAL_TRANSPORT=blocking: the older form that drains the streams around
 * every collective).
 * dst_prove_sharded is stark::prove on context `ctx` (created with rank / world in dst_params, trace uploaded on EVERY rank): all ranks
 * call it, all ranks receive the same proof bytes; when any rank fails every rank returns an error.  dst_prove_sharded_local is the
 * one-call form for a single-process host: `world` contexts, one thread each. */
typedef struct dst_comm dst_comm;
DST_API int dst_comm_unique_id(uint8_t id[128]);
DST_API int dst_comm_init(const uint8_t id[128], uint32_t rank, uint32_t world, int device, dst_comm** out);
DST_API int dst_comm_init_local(uint32_t world, dst_comm** out /* [world] */);
/* the host's own transport (MPI, its process launcher's channel, ...): `fn` is called for every collective with kind 0 = all-gather of
 * `bytes` per rank, 1 = all-to-all with chunks of `bytes` (both on DEVICE buffers, complete when fn returns), 2 = all-gather of host values;
 * it returns 0 on success */
typedef int (*dst_comm_fn)(void* user, int kind, const void* send, void* recv, size_t bytes);
DST_API int dst_comm_init_callbacks(uint32_t rank, uint32_t world, dst_comm_fn fn, void* user, dst_comm** out);
DST_API void dst_comm_destroy(dst_comm* comm);
/* Containment.  The reference panics (src/lib.rs:32,49,56); dst_prove_sharded returns an error on every rank instead, also when a peer
 * never arrives: every host wait behind a collective is a bounded poll of the stream (plus ncclCommGetAsyncError on the RCCL transport).
 * After `seconds` without completion (default 60, DISTAFF_COMM_TIMEOUT_S at creation; <= 0: no limit) the rank aborts its communicator --
 * ncclCommAbort on RCCL, which also ends the kernels stuck on the stream; the in-process transport wakes every peer out of its barrier --
 * and returns DST_ERR_COMM; dst_comm_last_error then names the wait and the index, kind and size of the last collective this rank issued
 * (with dst_comm_trace the whole issue order).  dst_comm_abort does the same from the host's side (a watchdog that learnt of a dead
 * peer).  A callback transport's channel is the host's to bound: a callback that returns non-zero ends the rank the same way. */
DST_API int dst_comm_set_timeout(dst_comm* comm, double seconds);
DST_API int dst_comm_abort(dst_comm* comm);
/* What a communicator is and what its transport says about itself.  For the RCCL transport rccl_ranks / rccl_rank / device come from
 * ncclCommCount / ncclCommUserRank / ncclCommCuDevice on the live communicator (the proof that RCCL connected `world` ranks);
 * for the in-process transport peers_other_device = ranks whose buffers live on another device than this rank's and peers_enabled = how many
 * of those this rank reaches with peer access (hipDeviceEnablePeerAccess; the others are staged through the host), both known after the
 * first device collective. */
enum { DST_COMM_RCCL = 0, DST_COMM_LOCAL = 1, DST_COMM_CALLBACKS = 2 };
typedef struct dst_comm_info {
    uint32_t transport, rank, world;
    int32_t device;                     /* -1 when the transport does not know it */
    uint32_t rccl_ranks, rccl_rank, rccl_version;
    uint32_t peers_other_device, peers_enabled;
} dst_comm_info;
DST_API int dst_comm_describe(const dst_comm* comm, dst_comm_info* out);
/* Issue-order record of the collectives of this rank (see comm.h): enable = 1 start / 0 stop / -1 unchanged; `out` receives the record so
 * far as text ("<G|A|H> <bytes per rank> <stream index|->" per line), *len its full length.  DISTAFF_SHARD_DEBUG=1 starts it at creation. */
DST_API int dst_comm_trace(dst_comm* comm, int enable, char* out, size_t cap, size_t* len);
/* helper for callback transports that stage through their own buffers: one synchronous copy of `bytes` between host memory and memory of
 * the calling thread's current device, in either direction or device to device (the direction follows from the pointers) */
DST_API int dst_comm_copy(void* dst, const void* src, size_t bytes);
DST_API const char* dst_comm_last_error(const dst_comm* comm);   /* comm may be NULL: the creation-time error */
DST_API int dst_prove_sharded(dst_ctx* ctx, dst_comm* comm, const dst_public* pub, uint8_t* proof, size_t cap, size_t* len);
/* host-side view of the last dst_prove_sharded on this rank: out[0] = milliseconds inside the transport's calls (enqueue time on RCCL, the
 * whole exchange on a blocking transport), out[1] = milliseconds waiting for tree roots (the only host waits of the protocol), out[2] =
 * number of tree exchanges */
DST_API int dst_shard_stage_ms(const dst_ctx* ctx, double out[3]);
/* device-side view of the collectives of the last dst_prove_sharded on this rank: milliseconds from enqueue to completion (events around
 * every collective on the stream it was queued on; on RCCL that includes the wait for the slowest peer), summed per kind --
 * out[0] coefficient all-gathers, [1] tree all-to-alls (boundary nodes), [2] tree all-gathers (subtree roots + status records, or boundary
 * nodes in the all-gather-only form), [3] the all-gather of the constraint evaluations, [4] the all-gather of the first replicated FRI
 * layer, [5] all-gathers of host values (openings; host wall time), [6] number of collectives, [7] of which timed by events */
DST_API int dst_shard_exchange_ms(const dst_ctx* ctx, double out[8]);
DST_API int dst_prove_sharded_local(dst_ctx** ctxs, uint32_t world, const dst_public* pub, uint8_t* proof, size_t cap, size_t* len);

#ifdef __cplusplus
}
#endif
#endif
