// BLAKE3 leaf hashing and Merkle tree construction for gfx950.
//
// Replaces TraceTable::build_merkle_tree (/root/reference/src/stark/trace/trace_table.rs:174-185), MerkleTree::new /
// build_merkle_nodes (src/crypto/merkle.rs:25,269-294), evaluations_to_leaves (src/stark/prover.rs:180-187) and
// fri::utils::hash_values (src/stark/fri/utils.rs:16-22).  One lane hashes one leaf / one node; kernels that consume
// coset-major evaluations emit natural-order digests through an LDS tile transpose, so that global reads are
// KT*16-byte runs along k and global writes are JT*32-byte runs along the leaf index.
#include "ctx.h"
#include "blake3_dev.h"
#include "rescue_dev.h"
#include "host/stree_levels.h"
#include "host/tree_sequence.h"
#include "host/merkle_plan.h"

#define HASH_THREADS 256
static_assert(HASH_THREADS == MERKLE_THREADS, "host/merkle_plan.h sizes the grids of the tree kernels");

__device__ __forceinline__ void store_digest(digest* p, const uint32_t* cv) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
    q[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
}
// h = BLAKE3(two[0] || two[1]): a parent from its two children, in global memory or in LDS
__device__ __forceinline__ void hash_pair(const digest* two, uint32_t* h) {
    const uint4* p = reinterpret_cast<const uint4*>(two);
    uint4 a = p[0], b = p[1], c = p[2], d = p[3];
    uint32_t m[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    b3_hash64(m, h);
}
// h = BLAKE3(base[0] || base[stride] || base[2 stride] || base[3 stride]): a row of four field elements
__device__ __forceinline__ void hash_four(const fe* base, size_t stride, uint32_t* h) {
    uint32_t m[16];
#pragma unroll
    for (uint32_t e = 0; e < 4; e++) {
        fe v = base[(size_t)e * stride];
        m[4 * e] = v.v[0]; m[4 * e + 1] = v.v[1]; m[4 * e + 2] = v.v[2]; m[4 * e + 3] = v.v[3];
    }
    b3_hash64(m, h);
}

// BLAKE3 of `count` field elements read through `get(i)`; count * 16 <= 2032 bytes (one or two chunks)
template <class Get>
__device__ __forceinline__ void hash_elements(Get get, uint32_t count, uint32_t* out8) {
    uint32_t cv[8], cv1[8];
    const uint32_t first = count < 64u ? count : 64u;       // elements in chunk 0 (1024 bytes = 64 elements)
    const bool two_chunks = count > 64u;
    for (int pass = 0; pass < 2; pass++) {
        const uint32_t base = pass == 0 ? 0u : 64u;
        const uint32_t cnt = pass == 0 ? first : count - 64u;
        uint32_t* c = pass == 0 ? cv : cv1;
        b3_iv(c);
        const uint32_t blocks = (cnt + 3u) / 4u;
        for (uint32_t b = 0; b < blocks; b++) {
            uint32_t m[16];
#pragma unroll
            for (uint32_t e = 0; e < 4; e++) {
                uint32_t i = b * 4u + e;
                fe v = i < cnt ? get(base + i) : fe_zero();
                m[4 * e] = v.v[0]; m[4 * e + 1] = v.v[1]; m[4 * e + 2] = v.v[2]; m[4 * e + 3] = v.v[3];
            }
            uint32_t rem = cnt - b * 4u;
            uint32_t block_len = rem >= 4u ? 64u : rem * 16u;
            uint32_t flags = (b == 0 ? B3_CHUNK_START : 0u) | (b == blocks - 1 ? (B3_CHUNK_END | (two_chunks ? 0u : B3_ROOT)) : 0u);
            b3_compress(c, m, (uint32_t)pass, 0, block_len, flags);
        }
        if (!two_chunks) break;
    }
    if (two_chunks) {
        uint32_t m[16];
#pragma unroll
        for (int i = 0; i < 8; i++) { m[i] = cv[i]; m[8 + i] = cv1[i]; }
        b3_iv(cv);
        b3_compress(cv, m, 0, 0, 64, B3_PARENT | B3_ROOT);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) out8[i] = cv[i];
}

// ---- tile transpose: the kernels that read coset-major evaluations run blocks of KT x T lanes (kk fastest on the read side, tt fastest on
//      the write side) over grid = (extent / KT, cols / T), and hand the digest of (k, t) to the lane that writes it through an LDS tile ------
// the tail of such a kernel: lane (kk, tt) holds the digest of element k = blockIdx.x * KT + kk, column blockIdx.y * T + tt; out rows are `width` wide
__device__ __forceinline__ void tile_transpose_store(digest* tile, const uint32_t* h, uint32_t kk, uint32_t tt, uint32_t KT, uint32_t log_t, digest* __restrict__ out, uint32_t width) {
    const uint32_t T = 1u << log_t;
    store_digest(&tile[kk * T + tt], h);
    __syncthreads();
    const uint32_t kk2 = threadIdx.x >> log_t, tt2 = threadIdx.x & (T - 1);
    const size_t o = ((size_t)blockIdx.x * KT + kk2) * width + blockIdx.y * T + tt2;
    out[o] = tile[kk2 * T + tt2];
}
// the launch shape for `extent` elements along k and `cols` columns: T = min(cols, 32) columns per block, HASH_THREADS lanes =
// (HASH_THREADS >> log_t) indices k x 2^log_t columns, fewer lanes when the array has fewer than that many k (tiny traces, or many ranks at a
// small blowup): the grid never comes out empty
struct TileShape { uint32_t log_t, threads; dim3 grid; };
static TileShape tile_shape(size_t extent, uint32_t cols) {
    TileShape s;
    const uint32_t t = cols < 32 ? cols : 32u;
    s.log_t = 0;
    while ((1u << s.log_t) < t) s.log_t++;
    const size_t want = extent << s.log_t;
    s.threads = (uint32_t)(want < HASH_THREADS ? want : HASH_THREADS);
    const uint32_t KT = s.threads >> s.log_t;
    s.grid = dim3((unsigned)(extent / KT), (unsigned)(cols >> s.log_t));
    return s;
}

// ---- trace leaves: leaf(B*k + j) = BLAKE3(reg_0 || ... || reg_{W-1}) at that row --------------------------------------------
__global__ void __launch_bounds__(HASH_THREADS) trace_leaves_kernel(const fe* __restrict__ lde, digest* __restrict__ leaves,
                                                                   uint32_t W, size_t n, uint32_t Bc, uint32_t log_jt) {
    __shared__ digest tile[HASH_THREADS];
    const uint32_t JT = 1u << log_jt, KT = blockDim.x >> log_jt;          // the launcher shrinks the block for tiny traces
    const uint32_t kk = threadIdx.x % KT, jj = threadIdx.x / KT;
    const size_t k = (size_t)blockIdx.x * KT + kk;
    const uint32_t j = blockIdx.y * JT + jj;
    const fe* base = lde + (size_t)j * n + k;
    const size_t col_stride = (size_t)Bc * n;
    uint32_t h[8];
    hash_elements([&](uint32_t c) { return base[(size_t)c * col_stride]; }, W, h);
    tile_transpose_store(tile, h, kk, jj, KT, log_jt, leaves, Bc);
}

void k_trace_leaves(dst_ctx* c) {
    const TileShape s = tile_shape(c->n, (uint32_t)c->Bc);
    { KScope ks_(c, "trace_leaves_kernel", (16.0 * c->W + 32.0) * c->Bc * c->n, true); hipLaunchKernelGGL(trace_leaves_kernel, s.grid, dim3(s.threads), 0, c->stream, (const fe*)c->lde, c->trace_leaves, (uint32_t)c->W, c->n, (uint32_t)c->Bc, s.log_t); }
}

// ---- generic Merkle levels: out[i] = H(children[2i] || children[2i+1]) -------------------------------------------------------
__global__ void __launch_bounds__(HASH_THREADS) merkle_level_kernel(const digest* __restrict__ children, digest* __restrict__ out, size_t count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t h[8];
    hash_pair(children + 2 * i, h);
    store_digest(out + i, h);
}

// two levels per launch for the wide levels: a lane turns four consecutive children into their two parents and the grandparent (three
// compressions, every lane busy), so the level in between is written but not read back and a tree needs half as many wide launches
// children[0 .. 4 * count) -> parents = nodes[2 * count .. 4 * count) and grand = nodes[count .. 2 * count)   (heap positions of the two levels above)
__global__ void __launch_bounds__(HASH_THREADS) merkle_level2_kernel(const digest* __restrict__ children, digest* __restrict__ parents, digest* __restrict__ grand, size_t count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;          // grandparent index, count of them
    if (i >= count) return;
    uint32_t h0[8], h1[8], g[8];
    hash_pair(children + 4 * i, h0);
    hash_pair(children + 4 * i + 2, h1);
    store_digest(parents + 2 * i, h0);
    store_digest(parents + 2 * i + 1, h1);
    uint32_t m[16];
#pragma unroll
    for (int w = 0; w < 8; w++) { m[w] = h0[w]; m[8 + w] = h1[w]; }
    b3_hash64(m, g);
    store_digest(grand + i, g);
}

// the top of the tree in one workgroup: nodes[count .. 2*count) are already valid, fills nodes[1 .. count)
__global__ void __launch_bounds__(HASH_THREADS) merkle_top_kernel(digest* nodes, uint32_t count) {
    for (uint32_t cnt = count >> 1; cnt >= 1; cnt >>= 1) {
        for (uint32_t i = threadIdx.x; i < cnt; i += HASH_THREADS) {
            uint32_t h[8];
            hash_pair(nodes + 2 * (cnt + i), h);
            store_digest(nodes + cnt + i, h);
        }
        __threadfence_block();
        __syncthreads();
    }
    if (threadIdx.x < 8) nodes[0].w[threadIdx.x] = 0;          // merkle.rs:275
}

// nine levels in one launch: workgroup b hashes the 512 nodes nodes[count + 512 b ..) down to ONE node, keeping the intermediate levels
// in LDS and writing every level to its place in the heap.  Replaces nine launch-bound level kernels in the middle of a tree (between
// the wide levels, which are work-bound and keep one launch each, and the single-workgroup top).
__global__ void __launch_bounds__(HASH_THREADS) merkle_subtree_kernel(digest* nodes, size_t count) {
    __shared__ digest lvl[HASH_THREADS];
    const size_t b = blockIdx.x;
    uint32_t h[8];
    hash_pair(nodes + count + 512 * b + 2 * threadIdx.x, h);
    store_digest(nodes + (count >> 1) + 256 * b + threadIdx.x, h);
    store_digest(&lvl[threadIdx.x], h);
    __syncthreads();
    size_t level = count >> 1;
    for (uint32_t width = 128; width >= 1; width >>= 1) {          // nodes of this workgroup on the level being built
        level >>= 1;
        const bool active = threadIdx.x < width;
        if (active) {
            hash_pair(&lvl[2 * threadIdx.x], h);
            store_digest(nodes + level + (size_t)width * b + threadIdx.x, h);
        }
        __syncthreads();                                            // everyone has read its pair
        if (active) store_digest(&lvl[threadIdx.x], h);
        __syncthreads();
    }
}
static_assert(MERKLE_SUBTREE_NODES == 2 * HASH_THREADS && MERKLE_TOP_MAX <= 0xFFFFFFFFu, "merkle_subtree_kernel: a lane per pair of the 512 nodes; merkle_top_kernel: 32-bit count");

// Builds the tree levels above a filled level of `count` children, down to the level of `stop_count` nodes (0: down to the root nodes[1], and
// nodes[0] cleared).  leaves: the children as an array of their own, or nullptr: they are the level nodes[count .. 2 count) of the heap.
// host/merkle_plan.h chooses the kernels; this is the only place that launches them.
void k_merkle(dst_ctx* c, const digest* leaves, digest* nodes, size_t count, size_t stop_count) {
    const digest* children = leaves ? leaves : nodes + count;
    size_t level2_min = MERKLE_LEVEL2_MIN;
    if (const char* e = c->sw("DISTAFF_MERKLE_LEVEL2_LOG")) { const int k = atoi(e); level2_min = (size_t)1 << (k < 0 ? 0 : k > 40 ? 40 : k); }      // tests: the fused form on small trees
    for (const merkle_launch& l : merkle_plan(count, !leaves, stop_count, level2_min, c->sw("DISTAFF_MERKLE_LEVELS") != nullptr)) {
        KScope ks_(c, merkle_launch_name(l), merkle_launch_bytes(l));
        const dim3 g((unsigned)merkle_launch_blocks(l)), b(HASH_THREADS);
        switch (l.kind) {
            case MERKLE_LEVEL: hipLaunchKernelGGL(merkle_level_kernel, g, b, 0, c->stream, children, nodes + l.count, l.count); break;
            case MERKLE_LEVEL2: hipLaunchKernelGGL(merkle_level2_kernel, g, b, 0, c->stream, children, nodes + 2 * l.count, nodes + l.count, l.count); break;
            case MERKLE_SUBTREE: hipLaunchKernelGGL(merkle_subtree_kernel, g, b, 0, c->stream, nodes, l.count); break;
            case MERKLE_TOP: hipLaunchKernelGGL(merkle_top_kernel, g, b, 0, c->stream, nodes, (uint32_t)l.count); break;
        }
        children = nodes + merkle_launch_filled(l);
    }
}

// ---- constraint tree: leaves are raw evaluation pairs (prover.rs:180-187); the first node level hashes four consecutive
//      natural-order evaluations B*k + 4q .. 4q+3, i.e. cosets 4q..4q+3 at index k ---------------------------------------------
__global__ void __launch_bounds__(HASH_THREADS) constraint_level1_kernel(const fe* __restrict__ cevals, digest* __restrict__ out,
                                                                        size_t n, uint32_t Bc, uint32_t log_qt) {
    __shared__ digest tile[HASH_THREADS];
    const uint32_t QT = 1u << log_qt, KT = blockDim.x >> log_qt;
    const uint32_t kk = threadIdx.x % KT, qq = threadIdx.x / KT;
    const size_t k = (size_t)blockIdx.x * KT + kk;
    const uint32_t q = blockIdx.y * QT + qq;
    uint32_t h[8];
    hash_four(cevals + (size_t)(4 * q) * n + k, n, h);
    tile_transpose_store(tile, h, kk, qq, KT, log_qt, out, Bc / 4);
}

// the first node level of the constraint tree: leaves = the Bc n / 2 evaluation pairs of this context, Bc n / 4 nodes at cnodes[Bc n / 4 ..)
void k_constraint_level1(dst_ctx* c) {
    const TileShape s = tile_shape(c->n, (uint32_t)(c->Bc / 4));
    const size_t level1 = c->Bc * c->n / 4;
    { KScope ks_(c, "constraint_level1_kernel", 96.0 * level1); hipLaunchKernelGGL(constraint_level1_kernel, s.grid, dim3(s.threads), 0, c->stream, (const fe*)c->cevals, c->cnodes + level1, c->n, (uint32_t)c->Bc, s.log_t); }
}
void k_constraint_tree(dst_ctx* c) {
    k_constraint_level1(c);
    k_merkle(c, nullptr, c->cnodes, c->Bc * c->n / 4, 0);
}

// ---- FRI leaves: leaf(r) = BLAKE3(e[r] || e[r+R] || e[r+2R] || e[r+3R]), R = N_d / 4 (quartic.rs:137, fri/utils.rs:16) ----------
// layer 0 reads the coset-major composition evaluations: r = B*k + j with k < n/4, and r + s*R = B*(k + s*n/4) + j
__global__ void __launch_bounds__(HASH_THREADS) fri_leaves0_kernel(const fe* __restrict__ comp, digest* __restrict__ leaves,
                                                                  size_t n, uint32_t Bc, uint32_t log_jt) {
    __shared__ digest tile[HASH_THREADS];
    const uint32_t JT = 1u << log_jt, KT = blockDim.x >> log_jt;          // the launcher shrinks the block for tiny traces
    const uint32_t kk = threadIdx.x % KT, jj = threadIdx.x / KT;
    const size_t k = (size_t)blockIdx.x * KT + kk;
    const uint32_t j = blockIdx.y * JT + jj;
    uint32_t h[8];
    hash_four(comp + (size_t)j * n + k, n / 4, h);
    tile_transpose_store(tile, h, kk, jj, KT, log_jt, leaves, Bc);
}

void k_fri_leaves_layer0(dst_ctx* c) {
    const size_t kq = c->n / 4;
    const TileShape s = tile_shape(kq, (uint32_t)c->Bc);
    { KScope ks_(c, "fri_leaves0_kernel", 96.0 * kq * c->Bc); hipLaunchKernelGGL(fri_leaves0_kernel, s.grid, dim3(s.threads), 0, c->stream, (const fe*)c->comp, c->fri_leaves[0], c->n, (uint32_t)c->Bc, s.log_t); }
}

__global__ void __launch_bounds__(HASH_THREADS) fri_leaves_kernel(const fe* __restrict__ e, digest* __restrict__ leaves, size_t R) {
    size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    uint32_t h[8];
    hash_four(e + r, R, h);
    store_digest(leaves + r, h);
}

void k_fri_leaves_at(dst_ctx* c, const fe* e, digest* leaves, size_t R) {        // natural-order layer of 4R evaluations
    { KScope ks_(c, "fri_leaves_kernel", 96.0 * R); hipLaunchKernelGGL(fri_leaves_kernel, dim3((unsigned)((R + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, c->stream,
                       e, leaves, R); }
}
void k_fri_leaves(dst_ctx* c, int layer) { k_fri_leaves_at(c, c->fri_e[layer], c->fri_leaves[layer], c->fri_size[layer] / 4); }

// ---- coset-sharded trees (world > 1): a rank owns leaves B*k + j for its cosets j and keeps them as local index k*Bc + jl, so the
//      lowest log2(Bc) levels of every tree are rank-local.  `k_merkle` with a stop count builds the local heap down to `stop_count`
//      nodes (one per k); after the all-gather `k_upper_tree` interleaves the ranks' boundary nodes (node G*k + g = gathered[g][k])
//      and finishes the replicated upper part of the tree. ---------------------------------------------------------------------
__global__ void interleave_boundary_kernel(const digest* __restrict__ gathered, digest* __restrict__ out, size_t nb, uint32_t G) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nb * G) return;
    size_t k = t / G, g = t % G;
    out[t] = gathered[g * nb + k];
}
void k_upper_tree(dst_ctx* c, const digest* gathered, digest* upper, size_t nb, uint32_t G) {
    size_t count = nb * G;
    { KScope ks_(c, "interleave_boundary_kernel", 64.0 * count); hipLaunchKernelGGL(interleave_boundary_kernel, dim3((unsigned)((count + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, c->stream, gathered, upper + count, nb, G); }
    k_merkle(c, nullptr, upper, count, 0);
}
// dst[i] = the digest at the head of record i (records `stride` bytes apart): the ranks' subtree roots out of the exchanged root + status records
__global__ void digests_from_records_kernel(const uint8_t* __restrict__ recs, size_t stride, digest* __restrict__ dst, uint32_t count) {
    const uint32_t i = threadIdx.x >> 3, w = threadIdx.x & 7;
    if (i < count) dst[i].w[w] = reinterpret_cast<const uint32_t*>(recs + (size_t)i * stride)[w];
}
void k_digests_from_records(dst_ctx* c, const void* recs, size_t stride, digest* dst, size_t count) {      // count <= 8
    KScope ks_(c, "digests_from_records_kernel", 0.0);
    hipLaunchKernelGGL(digests_from_records_kernel, dim3(1), dim3(64), 0, c->stream, (const uint8_t*)recs, stride, dst, (uint32_t)count);
}
// FRI leaves of a coset-major layer e[Bc][nd]: leaf (k, jl), k < nd/4, local index k*Bc + jl
__global__ void __launch_bounds__(HASH_THREADS) fri_leaves_cm_kernel(const fe* __restrict__ e, digest* __restrict__ leaves, size_t nd, uint32_t Bc) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t q = nd / 4;
    if (t >= q * Bc) return;
    size_t jl = t / q, k = t % q;
    uint32_t h[8];
    hash_four(e + jl * nd + k, q, h);
    store_digest(leaves + k * Bc + jl, h);
}
void k_fri_leaves_cm(dst_ctx* c, const fe* e, digest* leaves, size_t nd) {
    size_t total = nd / 4 * c->Bc;
    { KScope ks_(c, "fri_leaves_cm_kernel", 96.0 * total); hipLaunchKernelGGL(fri_leaves_cm_kernel, dim3((unsigned)((total + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, c->stream, e, leaves, nd, (uint32_t)c->Bc); }
}

// ---- Rescue digests and Rescue Merkle trees (rescue_dev.h): utils::hasher::digest (src/utils/hasher.rs:12) and the trees that the VM's
//      smpath / pmpath authenticate (parent = digest(l0, l1, r0, r1), src/examples/merkle.rs:112-145).  They need no prover context: the
//      launchers take a stream.  A node is two field elements; node arrays have the layout of k_merkle_levels (nodes[1] = root,
//      nodes[count .. 2 count) = the level of `count` nodes).  `bad` receives 1 when an input element is not below p. ------------------
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_digest_kernel(const fe* __restrict__ in, fe* __restrict__ out, size_t count, uint32_t* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * RESCUE_THREADS + threadIdx.x;
    if (i >= count) return;
    const fe v0 = in[4 * i], v1 = in[4 * i + 1], v2 = in[4 * i + 2], v3 = in[4 * i + 3];
    if (!(rescue_canonical(v0) && rescue_canonical(v1) && rescue_canonical(v2) && rescue_canonical(v3))) *bad = 1u;
    fe d0, d1;
    rescue_digest4(v0, v1, v2, v3, d0, d1);
    out[2 * i] = d0; out[2 * i + 1] = d1;
}
// the parent at node-array position p on one lane: nodes[p] = digest(nodes[2 p], nodes[2 p + 1]); check: the children are leaves
__device__ __forceinline__ void rescue_parent(fe* nodes, size_t p, uint32_t check, uint32_t* bad) {
    const fe v0 = nodes[4 * p], v1 = nodes[4 * p + 1], v2 = nodes[4 * p + 2], v3 = nodes[4 * p + 3];
    if (check && !(rescue_canonical(v0) && rescue_canonical(v1) && rescue_canonical(v2) && rescue_canonical(v3))) *bad = 1u;
    fe d0, d1;
    rescue_digest4(v0, v1, v2, v3, d0, d1);
    nodes[2 * p] = d0; nodes[2 * p + 1] = d1;
}
// the same parent on a group of eight lanes (six of them working, one state element each): the narrow levels, where a launch lasts one
// wavefront's dependent chain whatever its width -- the chain per lane is a sixth as long.  A group past the end (!live) is given a
// valid p, keeps the barriers and stores nothing.
__device__ __forceinline__ void rescue_parent_spread(fe* nodes, size_t p, bool live, uint32_t check, uint32_t* bad, fe* xch) {
    const uint32_t e = threadIdx.x & 7u;
    fe v = fe_zero();                                                  // state after hasher.rs:18: (0, 0, r1, r0, l1, l0)
    if (e >= 2u && e < 6u) {
        v = nodes[4 * p + (5u - e)];
        if (check && live && !rescue_canonical(v)) *bad = 1u;
    }
    rescue_permute_lane(v, e, xch + (threadIdx.x & ~7u));
    if (live && (e == 5u || e == 4u)) nodes[2 * p + (5u - e)] = v;
}
// one whole level of `count` parents, p = count + i, in either form
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_tree_level_kernel(fe* nodes, size_t count, uint32_t check, uint32_t* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * RESCUE_THREADS + threadIdx.x;
    if (i >= count) return;
    rescue_parent(nodes, count + i, check, bad);
}
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_tree_level_spread_kernel(fe* nodes, size_t count, uint32_t check, uint32_t* __restrict__ bad) {
    __shared__ fe xch[RESCUE_THREADS];
    const size_t i = (size_t)blockIdx.x * (RESCUE_THREADS / 8u) + (threadIdx.x >> 3);
    rescue_parent_spread(nodes, count + (i < count ? i : 0), i < count, check, bad, xch);
}
// updates in place (dst_rtree_update): the dirty parents of a level, p = list[g] a node-array position.  The host has validated the new
// leaves and every inner node is a digest, so nothing is checked here.
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_tree_update_kernel(fe* nodes, const uint32_t* __restrict__ list, size_t count) {
    const size_t g = (size_t)blockIdx.x * RESCUE_THREADS + threadIdx.x;
    if (g >= count) return;
    rescue_parent(nodes, list[g], 0u, nullptr);
}
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_tree_update_spread_kernel(fe* nodes, const uint32_t* __restrict__ list, size_t count) {
    __shared__ fe xch[RESCUE_THREADS];
    const size_t g = (size_t)blockIdx.x * (RESCUE_THREADS / 8u) + (threadIdx.x >> 3);
    rescue_parent_spread(nodes, list[g < count ? g : 0], g < count, 0u, nullptr, xch);
}
// compile-time knob (profiles/rescue_tree.md): levels of at most this many parents use the spread form
#ifndef RESCUE_SPREAD_MAX
#define RESCUE_SPREAD_MAX ((size_t)1 << 15)
#endif
// nodes[pos[i]] = vals[i] (the new leaves of an update) and out[i] = nodes[pos[i]] (batched openings): one lane per element, two per node
__global__ void rescue_tree_scatter_kernel(fe* __restrict__ nodes, const uint32_t* __restrict__ pos, const fe* __restrict__ vals, size_t count) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * count) return;
    nodes[2 * (size_t)pos[t >> 1] + (t & 1)] = vals[t];
}
__global__ void rescue_tree_gather_kernel(const fe* __restrict__ nodes, const uint32_t* __restrict__ pos, fe* __restrict__ out, size_t count) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * count) return;
    out[t] = nodes[2 * (size_t)pos[t >> 1] + (t & 1)];
}

int k_rescue_digests(hipStream_t stream, const fe* in, fe* out, size_t count, uint32_t* bad) {
    hipLaunchKernelGGL(rescue_digest_kernel, dim3((unsigned)((count + RESCUE_THREADS - 1) / RESCUE_THREADS)), dim3(RESCUE_THREADS), 0, stream, in, out, count, bad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// one level of `count` parents: the whole level of that width (list == nullptr), or the parents at the positions list[0 .. count) (device)
static int rescue_level(hipStream_t stream, fe* nodes, size_t count, const uint32_t* list, uint32_t check, uint32_t* bad) {
    const bool spread = count <= RESCUE_SPREAD_MAX;
    const size_t per_block = spread ? RESCUE_THREADS / 8 : RESCUE_THREADS;
    const dim3 grid((unsigned)((count + per_block - 1) / per_block)), block(RESCUE_THREADS);
    if (list && spread) hipLaunchKernelGGL(rescue_tree_update_spread_kernel, grid, block, 0, stream, nodes, list, count);
    else if (list) hipLaunchKernelGGL(rescue_tree_update_kernel, grid, block, 0, stream, nodes, list, count);
    else if (spread) hipLaunchKernelGGL(rescue_tree_level_spread_kernel, grid, block, 0, stream, nodes, count, check, bad);
    else hipLaunchKernelGGL(rescue_tree_level_kernel, grid, block, 0, stream, nodes, count, check, bad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// fills nodes[1 .. leaves) of a node array whose leaf level nodes[leaves .. 2 leaves) is in place
int k_rescue_tree(hipStream_t stream, fe* nodes, size_t leaves, uint32_t* bad) {
    for (size_t count = leaves >> 1; count >= 1; count >>= 1)
        if (rescue_level(stream, nodes, count, nullptr, count == (leaves >> 1) ? 1u : 0u, bad)) return -1;
    return 0;
}
// recomputes the dirty parents level by level, from the level of leaves / 2 parents (level log_leaves - 1) to the root (level 0): level l has
// cnt[l] dirty parents, their positions sorted at lists[off[l] ..); a level that is dirty as a whole (cnt[l] == 2^l) has no list
int k_rescue_tree_update(hipStream_t stream, fe* nodes, uint32_t log_leaves, const uint32_t* lists, const size_t* off, const size_t* cnt) {
    for (uint32_t l = log_leaves; l-- > 0;)
        if (rescue_level(stream, nodes, cnt[l], cnt[l] == ((size_t)1 << l) ? nullptr : lists + off[l], 0u, nullptr)) return -1;
    return 0;
}
int k_rescue_tree_scatter(hipStream_t stream, fe* nodes, const uint32_t* pos, const fe* vals, size_t count) {
    hipLaunchKernelGGL(rescue_tree_scatter_kernel, dim3((unsigned)((2 * count + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, stream, nodes, pos, vals, count);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int k_rescue_tree_gather(hipStream_t stream, const fe* nodes, const uint32_t* pos, fe* out, size_t count) {
    hipLaunchKernelGGL(rescue_tree_gather_kernel, dim3((unsigned)((2 * count + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, stream, nodes, pos, out, count);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- sparse Rescue Merkle trees (dst_stree_*, host/stree_levels.h): a level is a sorted list of prefixes and a node list beside it, all levels in
//      one node array and one prefix array; a "flat position" indexes both.  A parent with prefix q looks its children up by a lower-bound search
//      for 2q among the child level's prefixes [cstart, cstart + ccnt) and takes a side that is not stored from (e0, e1), the value of an empty
//      subtree of the child level.  The search comes first: only the flat positions found live across the digest.  The parents of a launch are
//      the flat positions list[0 .. count) (a dirty list) or pstart + [0 .. count) (the whole level, list == nullptr).  The host has validated the
//      leaves, every inner node is a digest: nothing is checked here.  The kernels that read prefixes or indices are stated once over the key
//      type K: uint64_t (dst_stree_*) and stree_wide, 16 bytes (dst_wtree_*, depth <= 127).  The wider search state -- two prefixes of two words
//      each and the search bounds -- is dead before the digest starts, as the narrow search's is. ----------------------------------------------
template <class K>
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_stree_level_kernel(fe* nodes, const K* __restrict__ pref, const uint32_t* __restrict__ list, size_t count,
                                                                           size_t pstart, size_t cstart, size_t ccnt, fe e0, fe e1) {
    const size_t g = (size_t)blockIdx.x * RESCUE_THREADS + threadIdx.x;
    if (g >= count) return;
    const size_t p = list ? (size_t)list[g] : pstart + g;
    size_t left, right;
    stree_children(pref + cstart, ccnt, pref[p], left, right);
    fe v0 = e0, v1 = e1, v2 = e0, v3 = e1;
    if (left != STREE_ABSENT) { v0 = nodes[2 * (cstart + left)]; v1 = nodes[2 * (cstart + left) + 1]; }
    if (right != STREE_ABSENT) { v2 = nodes[2 * (cstart + right)]; v3 = nodes[2 * (cstart + right) + 1]; }
    fe d0, d1;
    rescue_digest4(v0, v1, v2, v3, d0, d1);
    nodes[2 * p] = d0; nodes[2 * p + 1] = d1;
}
// the six-lanes-of-eight form (rescue_parent_spread): lanes 5, 4 hold l0, l1 and lanes 3, 2 hold r0, r1; a group past the end is given the first
// parent, keeps the barriers and stores nothing
template <class K>
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_stree_level_spread_kernel(fe* nodes, const K* __restrict__ pref, const uint32_t* __restrict__ list, size_t count,
                                                                                  size_t pstart, size_t cstart, size_t ccnt, fe e0, fe e1) {
    __shared__ fe xch[RESCUE_THREADS];
    const size_t i = (size_t)blockIdx.x * (RESCUE_THREADS / 8u) + (threadIdx.x >> 3);
    const bool live = i < count;
    const size_t g = live ? i : 0;
    const size_t p = list ? (size_t)list[g] : pstart + g;
    const uint32_t e = threadIdx.x & 7u;
    fe v = fe_zero();                                                  // state after hasher.rs:18: (0, 0, r1, r0, l1, l0)
    if (e >= 2u && e < 6u) {
        size_t left, right;
        stree_children(pref + cstart, ccnt, pref[p], left, right);
        const size_t child = e >= 4u ? left : right;
        v = (e & 1u) ? e0 : e1;
        if (child != STREE_ABSENT) v = nodes[2 * (cstart + child) + (1u - (e & 1u))];
    }
    rescue_permute_lane(v, e, xch + (threadIdx.x & ~7u));
    if (live && (e == 5u || e == 4u)) nodes[2 * p + (5u - e)] = v;
}
// the nodes a set does not touch: dst[j] = src[from[j]] for from[j] != STREE_NEW, two lanes per node
__global__ void rescue_stree_carry_kernel(fe* __restrict__ dst, const fe* __restrict__ src, const uint32_t* __restrict__ from, size_t count) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * count) return;
    const uint32_t f = from[t >> 1];
    if (f != STREE_NEW) dst[t] = src[2 * (size_t)f + (t & 1)];
}
// openings: one lane per (index, path node, element).  levels[2 l], levels[2 l + 1] = start and length of level l; empties[2 l ..) = the value of
// an empty subtree of level l.  A node that is not stored, the leaf included, is that value.
template <class K>
__global__ void rescue_stree_open_kernel(const fe* __restrict__ nodes, const K* __restrict__ pref, const uint64_t* __restrict__ levels, const fe* __restrict__ empties,
                                         const K* __restrict__ indices, fe* __restrict__ out, size_t count, uint32_t depth) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = depth + 1;
    if (t >= 2 * count * n) return;
    const size_t s = t >> 1;
    uint32_t level;
    K prefix;
    stree_path_slot(depth, indices[s / n], (uint32_t)(s % n), level, prefix);
    const size_t start = levels[2 * level], pos = stree_find(pref + start, levels[2 * level + 1], prefix);
    out[t] = pos != STREE_ABSENT ? nodes[2 * (start + pos) + (t & 1)] : empties[2 * level + (t & 1)];
}
// the nodes of a multiproof (dst_stree_multiproof): one lane per (node, element); node s is (level[s], prefix[s]), found in its level's list like a
// path node above, its level's empty subtree when it is not stored
template <class K>
__global__ void rescue_stree_lookup_kernel(const fe* __restrict__ nodes, const K* __restrict__ pref, const uint64_t* __restrict__ levels, const fe* __restrict__ empties,
                                           const K* __restrict__ prefix, const uint32_t* __restrict__ level, fe* __restrict__ out, size_t count) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * count) return;
    const size_t s = t >> 1;
    const uint32_t l = level[s];
    const size_t start = levels[2 * l], pos = stree_find(pref + start, levels[2 * l + 1], prefix[s]);
    out[t] = pos != STREE_ABSENT ? nodes[2 * (start + pos) + (t & 1)] : empties[2 * l + (t & 1)];
}
// the compact multiproof of a wide tree (dst_wtree_multiproof), two launches of LOCATE_THREADS lanes a block, one lane per asked node.  The first
// finds node s = (level[s], prefix[s]) in its level's list and leaves flat[s] = its flat position, or STREE_NEW when it is not stored, and rank[s]
// = how many stored nodes the block has before s (an inclusive scan over the block's flags in LDS), with the block's count in totals[block].  The
// second packs the stored nodes: block b starts at the sum of totals[0 .. b) -- every lane adds a stride of them, a tree in LDS adds the lanes --
// and lane s copies nodes[flat[s]] to out[base + rank[s]].  Barriers and LDS only, no cross-lane instructions: the host emulation runs them too.
#define LOCATE_THREADS RESCUE_LOCATE_BLOCK
template <class K>
__global__ void __launch_bounds__(LOCATE_THREADS) rescue_stree_locate_kernel(const K* __restrict__ pref, const uint64_t* __restrict__ levels, const K* __restrict__ prefix,
                                                                            const uint32_t* __restrict__ level, uint32_t* __restrict__ flat, uint32_t* __restrict__ rank,
                                                                            uint32_t* __restrict__ totals, size_t count) {
    __shared__ uint32_t scan[LOCATE_THREADS];
    const size_t s = (size_t)blockIdx.x * LOCATE_THREADS + threadIdx.x;
    uint32_t at = STREE_NEW;
    if (s < count) {
        const uint32_t l = level[s];
        const size_t start = levels[2 * l], pos = stree_find(pref + start, levels[2 * l + 1], prefix[s]);
        if (pos != STREE_ABSENT) at = (uint32_t)(start + pos);
    }
    const uint32_t stored = at != STREE_NEW ? 1u : 0u;
    scan[threadIdx.x] = stored;
    __syncthreads();
    for (uint32_t d = 1; d < LOCATE_THREADS; d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? scan[threadIdx.x - d] : 0u;
        __syncthreads();
        scan[threadIdx.x] += add;
        __syncthreads();
    }
    if (s < count) { flat[s] = at; rank[s] = scan[threadIdx.x] - stored; }
    if (threadIdx.x == LOCATE_THREADS - 1u) totals[blockIdx.x] = scan[threadIdx.x];
}
__global__ void __launch_bounds__(LOCATE_THREADS) rescue_stree_pack_kernel(const fe* __restrict__ nodes, const uint32_t* __restrict__ flat, const uint32_t* __restrict__ rank,
                                                                          const uint32_t* __restrict__ totals, fe* __restrict__ out, size_t count) {
    __shared__ uint32_t sum[LOCATE_THREADS];
    uint32_t mine = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += LOCATE_THREADS) mine += totals[b];
    sum[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t d = LOCATE_THREADS / 2u; d >= 1u; d >>= 1) {
        if (threadIdx.x < d) sum[threadIdx.x] += sum[threadIdx.x + d];
        __syncthreads();
    }
    const size_t s = (size_t)blockIdx.x * LOCATE_THREADS + threadIdx.x;
    if (s >= count) return;                                            // after the last barrier
    const uint32_t at = flat[s];
    if (at == STREE_NEW) return;
    const size_t to = (size_t)sum[0] + rank[s];
    out[2 * to] = nodes[2 * (size_t)at]; out[2 * to + 1] = nodes[2 * (size_t)at + 1];
}
// the leaves alone (dst_stree_get): one lane per index, one search of the leaf level [lstart, lstart + lcnt); a key that is not stored gives the
// empty leaf (e0, e1) and stored[i] = 0
template <class K>
__global__ void rescue_stree_get_kernel(const fe* __restrict__ nodes, const K* __restrict__ pref, size_t lstart, size_t lcnt, fe e0, fe e1,
                                        const K* __restrict__ indices, fe* __restrict__ out, uint8_t* __restrict__ stored, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const size_t pos = stree_find(pref + lstart, lcnt, indices[i]);
    const bool has = pos != STREE_ABSENT;
    out[2 * i] = has ? nodes[2 * (lstart + pos)] : e0;
    out[2 * i + 1] = has ? nodes[2 * (lstart + pos) + 1] : e1;
    stored[i] = has ? 1 : 0;
}
// which stored keys hold the empty leaf (dst_stree_compact): flags[i] = 1 when both elements of leaves[i] equal (e0, e1), one lane per key
__global__ void rescue_stree_empty_leaves_kernel(const fe* __restrict__ leaves, fe e0, fe e1, uint8_t* __restrict__ flags, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    flags[i] = fe_eq(leaves[2 * i], e0) && fe_eq(leaves[2 * i + 1], e1) ? 1 : 0;
}

template <class K>
static int rescue_stree_level(hipStream_t stream, fe* nodes, const K* pref, const uint32_t* list, size_t count, size_t pstart, size_t cstart, size_t ccnt, const fe* empty) {
    const bool spread = count <= RESCUE_SPREAD_MAX;
    const size_t per_block = spread ? RESCUE_THREADS / 8 : RESCUE_THREADS;
    const dim3 grid((unsigned)((count + per_block - 1) / per_block)), block(RESCUE_THREADS);
    if (spread) hipLaunchKernelGGL(rescue_stree_level_spread_kernel<K>, grid, block, 0, stream, nodes, pref, list, count, pstart, cstart, ccnt, empty[0], empty[1]);
    else hipLaunchKernelGGL(rescue_stree_level_kernel<K>, grid, block, 0, stream, nodes, pref, list, count, pstart, cstart, ccnt, empty[0], empty[1]);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int k_rescue_stree_level(hipStream_t stream, fe* nodes, const uint64_t* pref, const uint32_t* list, size_t count, size_t pstart, size_t cstart, size_t ccnt, const fe* empty) {
    return rescue_stree_level(stream, nodes, pref, list, count, pstart, cstart, ccnt, empty);
}
int k_rescue_stree_level(hipStream_t stream, fe* nodes, const stree_wide* pref, const uint32_t* list, size_t count, size_t pstart, size_t cstart, size_t ccnt, const fe* empty) {
    return rescue_stree_level(stream, nodes, pref, list, count, pstart, cstart, ccnt, empty);
}
int k_rescue_stree_carry(hipStream_t stream, fe* dst, const fe* src, const uint32_t* from, size_t count) {
    hipLaunchKernelGGL(rescue_stree_carry_kernel, dim3((unsigned)((2 * count + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, stream, dst, src, from, count);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
template <class K>
static int rescue_stree_open(hipStream_t stream, const fe* nodes, const K* pref, const uint64_t* levels, const fe* empties, const K* indices, fe* out, size_t count, uint32_t depth) {
    const size_t lanes = 2 * count * (depth + 1);
    hipLaunchKernelGGL(rescue_stree_open_kernel<K>, dim3((unsigned)((lanes + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, stream, nodes, pref, levels, empties, indices, out, count, depth);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int k_rescue_stree_open(hipStream_t stream, const fe* nodes, const uint64_t* pref, const uint64_t* levels, const fe* empties, const uint64_t* indices, fe* out, size_t count, uint32_t depth) {
    return rescue_stree_open(stream, nodes, pref, levels, empties, indices, out, count, depth);
}
int k_rescue_stree_open(hipStream_t stream, const fe* nodes, const stree_wide* pref, const uint64_t* levels, const fe* empties, const stree_wide* indices, fe* out, size_t count, uint32_t depth) {
    return rescue_stree_open(stream, nodes, pref, levels, empties, indices, out, count, depth);
}
template <class K>
static int rescue_stree_lookup(hipStream_t stream, const fe* nodes, const K* pref, const uint64_t* levels, const fe* empties, const K* prefix, const uint32_t* level, fe* out, size_t count) {
    hipLaunchKernelGGL(rescue_stree_lookup_kernel<K>, dim3((unsigned)((2 * count + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, stream, nodes, pref, levels, empties, prefix, level, out, count);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int k_rescue_stree_lookup(hipStream_t stream, const fe* nodes, const uint64_t* pref, const uint64_t* levels, const fe* empties, const uint64_t* prefix, const uint32_t* level, fe* out, size_t count) {
    return rescue_stree_lookup(stream, nodes, pref, levels, empties, prefix, level, out, count);
}
int k_rescue_stree_lookup(hipStream_t stream, const fe* nodes, const stree_wide* pref, const uint64_t* levels, const fe* empties, const stree_wide* prefix, const uint32_t* level, fe* out, size_t count) {
    return rescue_stree_lookup(stream, nodes, pref, levels, empties, prefix, level, out, count);
}
template <class K>
static int rescue_stree_get(hipStream_t stream, const fe* nodes, const K* pref, size_t lstart, size_t lcnt, const fe* empty, const K* indices, fe* out, uint8_t* stored, size_t count) {
    hipLaunchKernelGGL(rescue_stree_get_kernel<K>, dim3((unsigned)((count + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, stream, nodes, pref, lstart, lcnt, empty[0], empty[1], indices, out, stored, count);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int k_rescue_stree_get(hipStream_t stream, const fe* nodes, const uint64_t* pref, size_t lstart, size_t lcnt, const fe* empty, const uint64_t* indices, fe* out, uint8_t* stored, size_t count) {
    return rescue_stree_get(stream, nodes, pref, lstart, lcnt, empty, indices, out, stored, count);
}
int k_rescue_stree_get(hipStream_t stream, const fe* nodes, const stree_wide* pref, size_t lstart, size_t lcnt, const fe* empty, const stree_wide* indices, fe* out, uint8_t* stored, size_t count) {
    return rescue_stree_get(stream, nodes, pref, lstart, lcnt, empty, indices, out, stored, count);
}
int k_rescue_stree_locate(hipStream_t stream, const stree_wide* pref, const uint64_t* levels, const stree_wide* prefix, const uint32_t* level, uint32_t* flat, uint32_t* rank, uint32_t* totals,
                          size_t count) {
    hipLaunchKernelGGL(rescue_stree_locate_kernel<stree_wide>, dim3((unsigned)((count + LOCATE_THREADS - 1) / LOCATE_THREADS)), dim3(LOCATE_THREADS), 0, stream, pref, levels, prefix, level, flat,
                       rank, totals, count);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int k_rescue_stree_pack(hipStream_t stream, const fe* nodes, const uint32_t* flat, const uint32_t* rank, const uint32_t* totals, fe* out, size_t count) {
    hipLaunchKernelGGL(rescue_stree_pack_kernel, dim3((unsigned)((count + LOCATE_THREADS - 1) / LOCATE_THREADS)), dim3(LOCATE_THREADS), 0, stream, nodes, flat, rank, totals, out, count);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int k_rescue_stree_empty_leaves(hipStream_t stream, const fe* leaves, const fe* empty, uint8_t* flags, size_t count) {
    hipLaunchKernelGGL(rescue_stree_empty_leaves_kernel, dim3((unsigned)((count + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, stream, leaves, empty[0], empty[1], flags, count);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- ordered leaf writes (dst_rtree_apply, dst_stree_apply; host/tree_sequence.h): operation i of `count` has, per level, a version -- the value of
//      its leaf's ancestor there once operations 0 .. i are applied.  One launch turns the versions of a level (vin, 2 elements each) into those
//      of the level above (vout): version i = digest of vin[i] and its sibling, which the source word src[i] places -- the version of an earlier
//      operation in vin, a node of the tree as it was before the call (nodes; read only, a dense node array or a sparse tree's flat array), or
//      (e0, e1), an empty subtree of the child level.  Bit k - 1 of idx[i] says which child vin[i] is.  The sibling is node k of operation i's
//      authentication path of n nodes (paths, when asked for); the launch of the leaf level (own != nullptr) also stores node 0, the leaf's value
//      before operation i, found by own[i] in the same way.  The host has validated the leaves and made every source word. ----------------------
__device__ __forceinline__ fe rescue_seq_read(const fe* __restrict__ nodes, const fe* __restrict__ vin, uint32_t w, uint32_t elem, fe v /* of an empty subtree */) {
    if (w != TSEQ_EMPTY) v = *((w & TSEQ_VERSION) ? vin + 2 * (size_t)(w & ~TSEQ_VERSION) + elem : nodes + 2 * (size_t)w + elem);
    return v;
}
// one lane per digest: the lookups and the loads first, only the four inputs live across the digest
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_seq_level_kernel(const fe* __restrict__ nodes, const fe* __restrict__ vin, fe* __restrict__ vout, const uint32_t* __restrict__ src,
                                                                         const uint32_t* __restrict__ own, const uint64_t* __restrict__ idx, fe* __restrict__ paths, size_t count,
                                                                         uint32_t k, uint32_t n, fe e0, fe e1) {
    const size_t i = (size_t)blockIdx.x * RESCUE_THREADS + threadIdx.x;
    if (i >= count) return;
    if (own && paths) {
        const uint32_t w = own[i];
        paths[2 * i * n] = rescue_seq_read(nodes, vin, w, 0u, e0);
        paths[2 * i * n + 1] = rescue_seq_read(nodes, vin, w, 1u, e1);
    }
    const uint32_t w = src[i];
    const bool right = (idx[i] >> (k - 1u)) & 1u;                      // this operation's node is the right child: the sibling goes first
    const fe s0 = rescue_seq_read(nodes, vin, w, 0u, e0), s1 = rescue_seq_read(nodes, vin, w, 1u, e1);
    const fe c0 = vin[2 * i], c1 = vin[2 * i + 1];
    if (paths) { paths[2 * (i * n + k)] = s0; paths[2 * (i * n + k) + 1] = s1; }
    fe d0, d1;
    rescue_digest4(rescue_pick(right, s0, c0), rescue_pick(right, s1, c1), rescue_pick(right, c0, s0), rescue_pick(right, c1, s1), d0, d1);
    vout[2 * i] = d0; vout[2 * i + 1] = d1;
}
// the six-lanes-of-eight form (rescue_parent_spread): lanes 5, 4 hold l0, l1 and lanes 3, 2 hold r0, r1, each from the sibling or from vin[i]; lanes
// 7, 6 of the leaf level's launch copy the old leaf.  A group past the end is given operation 0, keeps the barriers and stores nothing.
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_seq_level_spread_kernel(const fe* __restrict__ nodes, const fe* __restrict__ vin, fe* __restrict__ vout, const uint32_t* __restrict__ src,
                                                                                const uint32_t* __restrict__ own, const uint64_t* __restrict__ idx, fe* __restrict__ paths, size_t count,
                                                                                uint32_t k, uint32_t n, fe e0, fe e1) {
    __shared__ fe xch[RESCUE_THREADS];
    const size_t g = (size_t)blockIdx.x * (RESCUE_THREADS / 8u) + (threadIdx.x >> 3);
    const bool live = g < count;
    const size_t i = live ? g : 0;
    const uint32_t e = threadIdx.x & 7u, elem = 1u - (e & 1u);
    fe v = fe_zero();                                                  // state after hasher.rs:18: (0, 0, r1, r0, l1, l0)
    if (e >= 6u) {
        if (live && own && paths) paths[2 * i * n + (e - 6u)] = rescue_seq_read(nodes, vin, own[i], e - 6u, rescue_pick(e == 6u, e0, e1));
    } else if (e >= 2u) {
        const bool right = (idx[i] >> (k - 1u)) & 1u;
        if ((e >= 4u) == right) {                                      // this lane's side is the sibling's
            v = rescue_seq_read(nodes, vin, src[i], elem, rescue_pick(elem != 0u, e1, e0));
            if (live && paths) paths[2 * (i * n + k) + elem] = v;
        } else v = vin[2 * i + elem];
    }
    rescue_permute_lane(v, e, xch + (threadIdx.x & ~7u));
    if (live && (e == 5u || e == 4u)) vout[2 * i + (5u - e)] = v;
}
// nodes[pos[i]] = vals[from[i]]: the last versions of a level into a dense node array, two lanes per node
__global__ void rescue_tree_scatter_from_kernel(fe* __restrict__ nodes, const uint32_t* __restrict__ pos, const fe* __restrict__ vals, const uint32_t* __restrict__ from, size_t count) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * count) return;
    nodes[2 * (size_t)pos[t >> 1] + (t & 1)] = vals[2 * (size_t)from[t >> 1] + (t & 1)];
}

int k_rescue_seq_level(hipStream_t stream, const fe* nodes, const fe* vin, fe* vout, const uint32_t* src, const uint32_t* own, const uint64_t* idx, fe* paths, size_t count, uint32_t k, uint32_t n,
                       const fe* empty) {
    const bool spread = count <= RESCUE_SPREAD_MAX;
    const size_t per_block = spread ? RESCUE_THREADS / 8 : RESCUE_THREADS;
    const dim3 grid((unsigned)((count + per_block - 1) / per_block)), block(RESCUE_THREADS);
    if (spread) hipLaunchKernelGGL(rescue_seq_level_spread_kernel, grid, block, 0, stream, nodes, vin, vout, src, own, idx, paths, count, k, n, empty[0], empty[1]);
    else hipLaunchKernelGGL(rescue_seq_level_kernel, grid, block, 0, stream, nodes, vin, vout, src, own, idx, paths, count, k, n, empty[0], empty[1]);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int k_rescue_tree_scatter_from(hipStream_t stream, fe* nodes, const uint32_t* pos, const fe* vals, const uint32_t* from, size_t count) {
    hipLaunchKernelGGL(rescue_tree_scatter_from_kernel, dim3((unsigned)((2 * count + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, stream, nodes, pos, vals, from, count);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- checking paths (dst_rescue_path_roots, dst_rescue_verify_paths, dst_rescue_verify_writes; host/path_verify.h): a chain is compute_merkle_root
//      (src/examples/merkle.rs:112-145) of one path of n nodes and one index -- n - 1 dependent digests, the first over (leaf, path[1]) ordered by
//      bit 0 of the index, digest k over the running value and path[k] ordered by bit k - 1.  All chains of a call are independent: ONE launch runs
//      every level of every chain.  `mode` says which chains there are: the `count` paths with their own first node as the leaf
//      (RESCUE_PATH_OWN), with alt[i] in its place (RESCUE_PATH_ALT), or both over one copy of the paths (RESCUE_PATH_BOTH: chain c < count is
//      path c with its own leaf, chain count + i path i with alt[i]).  out[c] = what chain c resolves to; `bad` receives 1 when an element a
//      chain reads -- its leaf, every sibling -- is not below p. ---------------------------------------------------------------------------------
// Following writes (dst_rescue_refresh_paths, host/path_refresh.h) needs the chains of the written leaves node by node, not only their ends: with
// STORE (RESCUE_PATH_BOTH only) the substitute-leaf chain of path i (c = count + i) also writes its running digest after level k = 1 .. n - 2 to
// mid[k - 1][i] -- level-major, n - 2 levels of `count` nodes, so that neighbouring chains store side by side -- where mid = out + 2 chains: the
// chain nodes follow the roots in one buffer, so both forms take the same
// arguments.  Each lane form states the chain once, STORE is a compile-time switch, and the instantiations without it are the code they were.
// the six-lanes-of-eight form (rescue_parent_spread): lanes 5, 4 hold l0, l1 and lanes 3, 2 hold r0, r1.  After the permutation the digest sits in
// lanes 5, 4; it reaches the side bit k - 1 of the index names through the group's LDS slots 5, 4, and the other side loads path[k].  A group past
// the end is given chain 0, keeps the barriers and stores nothing.  The lanes that hand the digest over are the lanes that store it: no barrier more.
template <class K, bool STORE = false>
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_path_root_spread_kernel(const fe* __restrict__ paths, uint32_t n, const K* __restrict__ indices, size_t count,
                                                                                const fe* __restrict__ alt, uint32_t mode, size_t chains, fe* __restrict__ out, uint32_t* __restrict__ bad) {
    __shared__ fe xch[RESCUE_THREADS];
    const size_t g = (size_t)blockIdx.x * (RESCUE_THREADS / 8u) + (threadIdx.x >> 3);
    const bool live = g < chains;
    const size_t c = live ? g : 0, i = c < count ? c : c - count;
    const bool sub = mode == RESCUE_PATH_ALT || c >= count;
    const uint32_t e = threadIdx.x & 7u, elem = 1u - (e & 1u);
    const bool works = e >= 2u && e < 6u;
    fe* const xs = xch + (threadIdx.x & ~7u);
    const fe* const path = paths + 2 * i * n;
    const K idx = indices[i];
    fe v = fe_zero();                                                  // state after hasher.rs:18: (0, 0, r1, r0, l1, l0)
    if (works) {
        const bool right = stree_bit(idx, 0u);                         // the leaf is the right child: the sibling goes first
        v = (e >= 4u) == right ? path[2 + elem] : sub ? alt[2 * i + elem] : path[elem];
        if (live && !rescue_canonical(v)) *bad = 1u;
    }
    rescue_permute_lane(v, e, xs);
#pragma unroll 1
    for (uint32_t k = 2; k < n; k++) {
        if (e == 5u || e == 4u) {
            xs[e] = v;
            if (STORE && live && c >= count) out[2 * (chains + (k - 2u) * count + i) + (5u - e)] = v;        // mid[k - 2][i]: the node after level k - 1
        }
        __syncthreads();
        v = fe_zero();
        if (works) {
            const bool right = stree_bit(idx, k - 1u);
            if ((e >= 4u) == right) {
                v = path[2 * k + elem];
                if (live && !rescue_canonical(v)) *bad = 1u;
            } else v = xs[4u + (e & 1u)];
        }
        __syncthreads();                                               // the digest has been read before the permutation writes the slots again
        rescue_permute_lane(v, e, xs);
    }
    if (live && (e == 5u || e == 4u)) out[2 * c + (5u - e)] = v;
}
// one chain per lane, for more chains than RESCUE_SPREAD_MAX: the digest is stated once, in a loop over the levels; only the running digest, the
// index and the chain's base address live across it.  Lanes read their paths n * 32 bytes apart: a level is milliseconds of arithmetic.
template <class K, bool STORE = false>
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_path_root_kernel(const fe* __restrict__ paths, uint32_t n, const K* __restrict__ indices, size_t count,
                                                                         const fe* __restrict__ alt, uint32_t mode, size_t chains, fe* __restrict__ out, uint32_t* __restrict__ bad) {
    const size_t c = (size_t)blockIdx.x * RESCUE_THREADS + threadIdx.x;
    if (c >= chains) return;
    const size_t i = c < count ? c : c - count;
    const fe* const path = paths + 2 * i * n;
    const fe* const leaf = (mode == RESCUE_PATH_ALT || c >= count) ? alt + 2 * i : path;
    const K idx = indices[i];
    fe d0 = leaf[0], d1 = leaf[1];
    if (!(rescue_canonical(d0) && rescue_canonical(d1))) *bad = 1u;
#pragma unroll 1
    for (uint32_t k = 1; k < n; k++) {
        const fe s0 = path[2 * k], s1 = path[2 * k + 1];
        if (!(rescue_canonical(s0) && rescue_canonical(s1))) *bad = 1u;
        const bool right = stree_bit(idx, k - 1u);                     // the running node is the right child: the sibling goes first
        const fe c0 = d0, c1 = d1;
        rescue_digest4(rescue_pick(right, s0, c0), rescue_pick(right, s1, c1), rescue_pick(right, c0, s0), rescue_pick(right, c1, s1), d0, d1);
        if (STORE && c >= count && k + 1u < n) {                       // mid[k - 1][i]: the node after level k
            fe* const m = out + 2 * (chains + (k - 1u) * count + i);
            m[0] = d0; m[1] = d1;
        }
    }
    out[2 * c] = d0; out[2 * c + 1] = d1;
}
// the refreshed paths (host/path_refresh.h): one lane per (held path, position k, element).  sel = the write that supplies the position, below 0
// to keep the held node; position 0 takes the written leaf, position k >= 1 the write's chain node at height k - 1 -- the written leaf again for
// k = 1, mid[k - 2][sel] above (level-major over `count` writes).  Every element of the held paths is read, and `bad` receives 1 when one is not below p.
__global__ void rescue_path_refresh_kernel(const fe* __restrict__ held, const int32_t* __restrict__ sel, const fe* __restrict__ leaves, const fe* __restrict__ mid, size_t count, uint32_t n,
                                           size_t total /* held paths * n * 2 */, fe* __restrict__ out, uint32_t* __restrict__ bad) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint32_t k = (uint32_t)((t >> 1) % n), el = (uint32_t)(t & 1);
    fe v = held[t];
    if (!rescue_canonical(v)) *bad = 1u;
    const int32_t s = sel[t >> 1];
    if (s >= 0) v = k <= 1u ? leaves[2 * (size_t)s + el] : mid[2 * ((size_t)(k - 2u) * count + (size_t)s) + el];
    out[t] = v;
}
// store: RESCUE_PATH_BOTH, and out is 2 count roots followed by n - 2 levels of count chain nodes
template <class K>
static int rescue_path_roots(hipStream_t stream, const fe* paths, uint32_t n, const K* indices, size_t count, const fe* alt_leaves, uint32_t mode, fe* out, bool store, uint32_t* bad) {
    const size_t chains = mode == RESCUE_PATH_BOTH ? 2 * count : count;
    const bool spread = chains <= RESCUE_SPREAD_MAX;
    const size_t per_block = spread ? RESCUE_THREADS / 8 : RESCUE_THREADS;
    const dim3 grid((unsigned)((chains + per_block - 1) / per_block)), block(RESCUE_THREADS);
    if (store && spread) hipLaunchKernelGGL((rescue_path_root_spread_kernel<K, true>), grid, block, 0, stream, paths, n, indices, count, alt_leaves, mode, chains, out, bad);
    else if (store) hipLaunchKernelGGL((rescue_path_root_kernel<K, true>), grid, block, 0, stream, paths, n, indices, count, alt_leaves, mode, chains, out, bad);
    else if (spread) hipLaunchKernelGGL(rescue_path_root_spread_kernel<K>, grid, block, 0, stream, paths, n, indices, count, alt_leaves, mode, chains, out, bad);
    else hipLaunchKernelGGL(rescue_path_root_kernel<K>, grid, block, 0, stream, paths, n, indices, count, alt_leaves, mode, chains, out, bad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int k_rescue_path_roots(hipStream_t stream, const fe* paths, uint32_t n, const uint64_t* indices, size_t count, const fe* alt_leaves, uint32_t mode, fe* out, uint32_t* bad) {
    return rescue_path_roots(stream, paths, n, indices, count, alt_leaves, mode, out, false, bad);
}
int k_rescue_path_roots(hipStream_t stream, const fe* paths, uint32_t n, const stree_wide* indices, size_t count, const fe* alt_leaves, uint32_t mode, fe* out, uint32_t* bad) {
    return rescue_path_roots(stream, paths, n, indices, count, alt_leaves, mode, out, false, bad);
}
int k_rescue_path_chains(hipStream_t stream, const fe* paths, uint32_t n, const uint64_t* indices, size_t count, const fe* leaves, fe* out, uint32_t* bad) {
    return rescue_path_roots(stream, paths, n, indices, count, leaves, RESCUE_PATH_BOTH, out, true, bad);
}
int k_rescue_path_chains(hipStream_t stream, const fe* paths, uint32_t n, const stree_wide* indices, size_t count, const fe* leaves, fe* out, uint32_t* bad) {
    return rescue_path_roots(stream, paths, n, indices, count, leaves, RESCUE_PATH_BOTH, out, true, bad);
}
int k_rescue_path_refresh(hipStream_t stream, const fe* held, const int32_t* sel, const fe* leaves, const fe* mid, size_t count, uint32_t n, size_t held_paths, fe* out, uint32_t* bad) {
    const size_t total = 2 * held_paths * n;
    hipLaunchKernelGGL(rescue_path_refresh_kernel, dim3((unsigned)((total + HASH_THREADS - 1) / HASH_THREADS)), dim3(HASH_THREADS), 0, stream, held, sel, leaves, mid, count, n, total, out, bad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- multiproofs (dst_rescue_multiproof_root, dst_rescue_verify_multiproof, dst_rescue_multiproof_paths; host/multiproof_plan.h): the leaves of a
//      set, the siblings nobody can recompute from them and every digest above them live in one pool of nodes, [leaves | supplied nodes | the
//      results of the leaf level's parents | ... | the root].  One launch hashes the jobs of one level: job j is pool[out_j] = digest(pool[left_j],
//      pool[right_j]), three 32-bit pool indices at jobs[3 j ..); every ancestor the paths share is one job, not one per path.  The jobs of a launch
//      read only what the upload or an earlier launch wrote.  A pool index below `inputs` is a leaf or a supplied node -- each is read by exactly
//      one job of the call -- and `bad` receives 1 when an element of it is not below p. -------------------------------------------------------------
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_multiproof_level_kernel(fe* pool, const uint32_t* __restrict__ jobs, size_t count, uint32_t inputs, uint32_t* __restrict__ bad) {
    const size_t j = (size_t)blockIdx.x * RESCUE_THREADS + threadIdx.x;
    if (j >= count) return;
    const uint32_t left = jobs[3 * j], right = jobs[3 * j + 1], out = jobs[3 * j + 2];
    const fe v0 = pool[2 * (size_t)left], v1 = pool[2 * (size_t)left + 1], v2 = pool[2 * (size_t)right], v3 = pool[2 * (size_t)right + 1];
    if ((left < inputs && !(rescue_canonical(v0) && rescue_canonical(v1))) || (right < inputs && !(rescue_canonical(v2) && rescue_canonical(v3)))) *bad = 1u;
    fe d0, d1;
    rescue_digest4(v0, v1, v2, v3, d0, d1);
    pool[2 * (size_t)out] = d0; pool[2 * (size_t)out + 1] = d1;
}
// the six-lanes-of-eight form (rescue_parent_spread): lanes 5, 4 hold l0, l1 and lanes 3, 2 hold r0, r1.  A group past the end is given job 0,
// keeps the barriers and stores nothing.
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_multiproof_level_spread_kernel(fe* pool, const uint32_t* __restrict__ jobs, size_t count, uint32_t inputs, uint32_t* __restrict__ bad) {
    __shared__ fe xch[RESCUE_THREADS];
    const size_t g = (size_t)blockIdx.x * (RESCUE_THREADS / 8u) + (threadIdx.x >> 3);
    const bool live = g < count;
    const size_t j = live ? g : 0;
    const uint32_t e = threadIdx.x & 7u;
    fe v = fe_zero();                                                  // state after hasher.rs:18: (0, 0, r1, r0, l1, l0)
    if (e >= 2u && e < 6u) {
        const uint32_t from = jobs[3 * j + (e >= 4u ? 0u : 1u)];
        v = pool[2 * (size_t)from + (1u - (e & 1u))];
        if (live && from < inputs && !rescue_canonical(v)) *bad = 1u;
    }
    rescue_permute_lane(v, e, xch + (threadIdx.x & ~7u));
    if (live && (e == 5u || e == 4u)) pool[2 * (size_t)jobs[3 * j + 2] + (5u - e)] = v;
}
int k_rescue_multiproof_level(hipStream_t stream, fe* pool, const uint32_t* jobs, size_t count, uint32_t inputs, uint32_t* bad) {
    const bool spread = count <= RESCUE_SPREAD_MAX;
    const size_t per_block = spread ? RESCUE_THREADS / 8 : RESCUE_THREADS;
    const dim3 grid((unsigned)((count + per_block - 1) / per_block)), block(RESCUE_THREADS);
    if (spread) hipLaunchKernelGGL(rescue_multiproof_level_spread_kernel, grid, block, 0, stream, pool, jobs, count, inputs, bad);
    else hipLaunchKernelGGL(rescue_multiproof_level_kernel, grid, block, 0, stream, pool, jobs, count, inputs, bad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- audits (dst_rtree_audit, dst_stree_audit): is every stored parent still the digest of its two children?  The work of a build without its
//      shape: all parents are there, no level waits for the one below, so ONE launch checks every parent of every level.  A lane hashes the
//      children as the level kernels do, compares the digest with the stored node, which it reads after the digest, and a parent that differs
//      goes into *first_bad by atomicMin -- the only word these kernels write; the host sets it to all ones.  The key orders the parents from
//      the root down: a dense tree's heap position; a sparse tree's level in the high 32 bits and the index within the level's list below. ------
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_tree_audit_kernel(const fe* __restrict__ nodes, size_t leaves, unsigned long long* __restrict__ first_bad) {
    const size_t p = (size_t)blockIdx.x * RESCUE_THREADS + threadIdx.x + 1;
    if (p >= leaves) return;
    fe d0, d1;
    rescue_digest4(nodes[4 * p], nodes[4 * p + 1], nodes[4 * p + 2], nodes[4 * p + 3], d0, d1);
    if (!(fe_eq(d0, nodes[2 * p]) && fe_eq(d1, nodes[2 * p + 1]))) atomicMin(first_bad, (unsigned long long)p);
}
// the six-lanes-of-eight form (rescue_parent_spread): the digest ends in lanes 5, 4, which compare an element each.  A group past the end is
// given the root, keeps the barriers and reports nothing.
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_tree_audit_spread_kernel(const fe* __restrict__ nodes, size_t leaves, unsigned long long* __restrict__ first_bad) {
    __shared__ fe xch[RESCUE_THREADS];
    const size_t i = (size_t)blockIdx.x * (RESCUE_THREADS / 8u) + (threadIdx.x >> 3) + 1;
    const bool live = i < leaves;
    const size_t p = live ? i : 1;
    const uint32_t e = threadIdx.x & 7u;
    fe v = fe_zero();                                                  // state after hasher.rs:18: (0, 0, r1, r0, l1, l0)
    if (e >= 2u && e < 6u) v = nodes[4 * p + (5u - e)];
    rescue_permute_lane(v, e, xch + (threadIdx.x & ~7u));
    if (live && (e == 5u || e == 4u) && !fe_eq(v, nodes[2 * p + (5u - e)])) atomicMin(first_bad, (unsigned long long)p);
}
// sparse: the parents are the flat positions [first, first + count) -- every level above the leaf level, which the layout puts first.  levels[2 l],
// levels[2 l + 1] = start and length of level l and the starts fall as l grows, so the level of p is the number of levels l < depth that start
// past p; empties[2 l ..) = the value of an empty subtree of level l.  The searches come first, as in rescue_stree_level_kernel.
__device__ __forceinline__ uint32_t rescue_stree_level_of(const uint64_t* __restrict__ levels, uint32_t depth, size_t p) {
    uint32_t l = 0;
    for (uint32_t k = 0; k < depth; k++) l += p < levels[2 * k] ? 1u : 0u;
    return l;
}
template <class K>
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_stree_audit_kernel(const fe* __restrict__ nodes, const K* __restrict__ pref, const uint64_t* __restrict__ levels,
                                                                           const fe* __restrict__ empties, uint32_t depth, size_t first, size_t count,
                                                                           unsigned long long* __restrict__ first_bad) {
    const size_t g = (size_t)blockIdx.x * RESCUE_THREADS + threadIdx.x;
    if (g >= count) return;
    const size_t p = first + g;
    const uint32_t l = rescue_stree_level_of(levels, depth, p);
    const size_t cstart = levels[2 * l + 2];
    size_t left, right;
    stree_children(pref + cstart, levels[2 * l + 3], pref[p], left, right);
    fe v0 = empties[2 * l + 2], v1 = empties[2 * l + 3], v2 = v0, v3 = v1;
    if (left != STREE_ABSENT) { v0 = nodes[2 * (cstart + left)]; v1 = nodes[2 * (cstart + left) + 1]; }
    if (right != STREE_ABSENT) { v2 = nodes[2 * (cstart + right)]; v3 = nodes[2 * (cstart + right) + 1]; }
    fe d0, d1;
    rescue_digest4(v0, v1, v2, v3, d0, d1);
    if (!(fe_eq(d0, nodes[2 * p]) && fe_eq(d1, nodes[2 * p + 1]))) atomicMin(first_bad, ((unsigned long long)l << 32) | (unsigned long long)(p - levels[2 * l]));
}
// the six-lanes-of-eight form (rescue_stree_level_spread_kernel): lanes 5, 4 hold l0, l1 and lanes 3, 2 hold r0, r1; a group past the end is
// given the first parent, keeps the barriers and reports nothing
template <class K>
__global__ void __launch_bounds__(RESCUE_THREADS) rescue_stree_audit_spread_kernel(const fe* __restrict__ nodes, const K* __restrict__ pref, const uint64_t* __restrict__ levels,
                                                                                  const fe* __restrict__ empties, uint32_t depth, size_t first, size_t count,
                                                                                  unsigned long long* __restrict__ first_bad) {
    __shared__ fe xch[RESCUE_THREADS];
    const size_t i = (size_t)blockIdx.x * (RESCUE_THREADS / 8u) + (threadIdx.x >> 3);
    const bool live = i < count;
    const size_t p = first + (live ? i : 0);
    const uint32_t e = threadIdx.x & 7u;
    const uint32_t l = rescue_stree_level_of(levels, depth, p);
    fe v = fe_zero();                                                  // state after hasher.rs:18: (0, 0, r1, r0, l1, l0)
    if (e >= 2u && e < 6u) {
        const size_t cstart = levels[2 * l + 2];
        size_t left, right;
        stree_children(pref + cstart, levels[2 * l + 3], pref[p], left, right);
        const size_t child = e >= 4u ? left : right;
        v = empties[2 * l + 2 + (1u - (e & 1u))];
        if (child != STREE_ABSENT) v = nodes[2 * (cstart + child) + (1u - (e & 1u))];
    }
    rescue_permute_lane(v, e, xch + (threadIdx.x & ~7u));
    if (live && (e == 5u || e == 4u) && !fe_eq(v, nodes[2 * p + (5u - e)])) atomicMin(first_bad, ((unsigned long long)l << 32) | (unsigned long long)(p - levels[2 * l]));
}

int k_rescue_tree_audit(hipStream_t stream, const fe* nodes, size_t leaves, unsigned long long* first_bad) {
    const size_t count = leaves - 1;
    const bool spread = count <= RESCUE_SPREAD_MAX;
    const size_t per_block = spread ? RESCUE_THREADS / 8 : RESCUE_THREADS;
    const dim3 grid((unsigned)((count + per_block - 1) / per_block)), block(RESCUE_THREADS);
    if (spread) hipLaunchKernelGGL(rescue_tree_audit_spread_kernel, grid, block, 0, stream, nodes, leaves, first_bad);
    else hipLaunchKernelGGL(rescue_tree_audit_kernel, grid, block, 0, stream, nodes, leaves, first_bad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
template <class K>
static int rescue_stree_audit(hipStream_t stream, const fe* nodes, const K* pref, const uint64_t* levels, const fe* empties, uint32_t depth, size_t first, size_t count,
                              unsigned long long* first_bad) {
    const bool spread = count <= RESCUE_SPREAD_MAX;
    const size_t per_block = spread ? RESCUE_THREADS / 8 : RESCUE_THREADS;
    const dim3 grid((unsigned)((count + per_block - 1) / per_block)), block(RESCUE_THREADS);
    if (spread) hipLaunchKernelGGL(rescue_stree_audit_spread_kernel<K>, grid, block, 0, stream, nodes, pref, levels, empties, depth, first, count, first_bad);
    else hipLaunchKernelGGL(rescue_stree_audit_kernel<K>, grid, block, 0, stream, nodes, pref, levels, empties, depth, first, count, first_bad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int k_rescue_stree_audit(hipStream_t stream, const fe* nodes, const uint64_t* pref, const uint64_t* levels, const fe* empties, uint32_t depth, size_t first, size_t count,
                         unsigned long long* first_bad) {
    return rescue_stree_audit(stream, nodes, pref, levels, empties, depth, first, count, first_bad);
}
int k_rescue_stree_audit(hipStream_t stream, const fe* nodes, const stree_wide* pref, const uint64_t* levels, const fe* empties, uint32_t depth, size_t first, size_t count,
                         unsigned long long* first_bad) {
    return rescue_stree_audit(stream, nodes, pref, levels, empties, depth, first, count, first_bad);
}
