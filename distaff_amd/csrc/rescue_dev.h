// Rescue over the 128-bit field on the device: the permutation behind utils::hasher::digest (the reference's src/utils/hasher.rs:12-40),
// i.e. the hash of the VM's smpath / pmpath Merkle trees.  Ten rounds of apply_round (:28) on a six-element state: add ARK[0..6][r], cube,
// MDS, add ARK[6..12][r], x^INV_ALPHA, MDS.  One digest is 9 180 field multiplications by the reference's count -- per round 12 for the cubes, 834 for
// the inverse S-box, 72 for the two MDS products (here accumulated with one reduction per row, so cheaper than 72 full multiplications) --
// 8 340 of them inside the inverse S-box, which is the
// addition chain of host_vm.h's inv_alpha4 (127 squarings + 12 multiplications per element) -- here data-driven (RESCUE_CHAIN) so that the
// chain is ONE squaring loop and ONE multiplication site instead of 25 inlined copies: the kernel stays far below the instruction cache.
//
// Two formulations of the same rounds:
//   rescue_permute6      one lane holds the whole state in registers; the six elements advance through the chain in lock-step, six
//                        independent multiplications in flight per lane.  For wide launches: every SIMD has work, throughput counts.
//   rescue_permute_lane  one digest spread over six lanes of a group of eight, one state element per lane; the two MDS products of a
//                        round exchange the state through LDS.  A sixth of the dependent chain per lane: for the narrow levels at the top
//                        of a tree, where a launch is one wavefront's latency whatever its width.
// The 120 round constants and 36 MDS entries are wave-uniform in the first form: they are read from constant memory with uniform
// indices (scalar loads), nothing is staged in registers across the chain.
#pragma once
#include "fe.h"
#include "rescue_constants.h"

#define RESCUE_ROUNDS 10u          // HASH_NUM_ROUNDS (src/lib.rs); rounds 0..9 of the 16-column ARK table
#define RESCUE_THREADS 64u         // one wavefront per workgroup: up to 8192 digests reach every SIMD, and the LDS exchange of the spread form is a one-wave barrier

// half round h of round h / 2 adds ARK[(h & 1) * 6 + i][h / 2] (hasher.rs:33,37).  The tables of rescue_constants.h are constants with
// constant initialisers: the device compilation places them in constant memory, and uniform indices become scalar loads.
#define RESCUE_ARK(h, i) rescue_const(HASHER_ARK[((h) & 1u) * 6u + (i)][(h) >> 1])
#define RESCUE_MDS(k) rescue_const(HASHER_MDS[k])

// the addition chain for INV_ALPHA = (10)^40 10001100 (10)^16 10101011b (host_vm.h:54-86), one word per step:
// bits 0..7 squarings, then bits 8..10 the multiplier (0 none, 1 the value the step started from, 2 x, 3 a4, 4 a8, 5 a16), bits 12..13 where
// the result is kept (1 a4, 2 a8, 3 a16); a_k = x^((10)^k).  127 squarings, 12 multiplications.
#define RESCUE_STEP(nsqr, mul, keep) ((uint32_t)(nsqr) | ((uint32_t)(mul) << 8) | ((uint32_t)(keep) << 12))
#define RESCUE_CHAIN_STEPS 13u
__constant__ const uint32_t RESCUE_CHAIN[RESCUE_CHAIN_STEPS] = {
    RESCUE_STEP(1, 0, 0),       // a1 = x^(10b)
    RESCUE_STEP(2, 1, 0),       // a2
    RESCUE_STEP(4, 1, 1),       // a4
    RESCUE_STEP(8, 1, 2),       // a8
    RESCUE_STEP(16, 1, 3),      // a16
    RESCUE_STEP(32, 1, 0),      // (10)^32
    RESCUE_STEP(16, 4, 0),      // (10)^40
    RESCUE_STEP(1, 2, 0),       // 1
    RESCUE_STEP(4, 2, 0),       // 0001
    RESCUE_STEP(1, 2, 0),       // 1
    RESCUE_STEP(34, 5, 0),      // 00 (10)^16
    RESCUE_STEP(8, 3, 0),       // (10)^4 ...
    RESCUE_STEP(0, 2, 0),       // ... + 1 = 10101011
};

__device__ __forceinline__ fe rescue_const(const uint32_t* w) { return fe_make(w[0], w[1], w[2], w[3]); }
__device__ __forceinline__ bool rescue_canonical(const fe& a) {          // a < p = 0xFFFFFFFF_FFFFFFFF_FFFFD300_00000001
    return !(a.v[3] == FE_P3 && a.v[2] == FE_P2 && (a.v[1] > FE_P1 || (a.v[1] == FE_P1 && a.v[0] >= FE_P0)));
}

// c ? a : b limb by limb (a conditional between two structures would select an address and keep both in memory)
__device__ __forceinline__ fe rescue_pick(bool c, const fe& a, const fe& b) { return fe_make(c ? a.v[0] : b.v[0], c ? a.v[1] : b.v[1], c ? a.v[2] : b.v[2], c ? a.v[3] : b.v[3]); }

// s[i] <- s[i]^INV_ALPHA for E elements in lock-step (hasher.rs:54-59)
template <int E>
__device__ __forceinline__ void rescue_inv_sbox(fe (&s)[E]) {
    fe x[E], a4[E], a8[E], a16[E];
#pragma unroll
    for (int i = 0; i < E; i++) x[i] = a4[i] = a8[i] = a16[i] = s[i];
#pragma unroll 1
    for (uint32_t st = 0; st < RESCUE_CHAIN_STEPS; st++) {
        const uint32_t w = RESCUE_CHAIN[st], nsqr = w & 0xFFu, mul = (w >> 8) & 7u, keep = (w >> 12) & 3u;
        fe m[E];
#pragma unroll
        for (int i = 0; i < E; i++) m[i] = rescue_pick(mul == 2u, x[i], rescue_pick(mul == 3u, a4[i], rescue_pick(mul == 4u, a8[i], rescue_pick(mul == 5u, a16[i], s[i]))));
#pragma unroll 1
        for (uint32_t k = 0; k < nsqr; k++) {
#pragma unroll
            for (int i = 0; i < E; i++) s[i] = fe_sqr(s[i]);
        }
        if (mul != 0u) {
#pragma unroll
            for (int i = 0; i < E; i++) s[i] = fe_mul(s[i], m[i]);
        }
#pragma unroll
        for (int i = 0; i < E; i++) {
            a4[i] = rescue_pick(keep == 1u, s[i], a4[i]);
            a8[i] = rescue_pick(keep == 2u, s[i], a8[i]);
            a16[i] = rescue_pick(keep == 3u, s[i], a16[i]);
        }
    }
}

// the whole state in one lane's registers
__device__ __forceinline__ void rescue_permute6(fe (&s)[6]) {
#pragma unroll 1
    for (uint32_t h = 0; h < 2u * RESCUE_ROUNDS; h++) {                 // half rounds: constants, S-box (cube / inverse), MDS
#pragma unroll
        for (int i = 0; i < 6; i++) s[i] = fe_add(s[i], RESCUE_ARK(h, i));
        if (h & 1u) rescue_inv_sbox<6>(s);
        else {
#pragma unroll
            for (int i = 0; i < 6; i++) s[i] = fe_cube(s[i]);
        }
        fe r[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {                                    // apply_mds (hasher.rs:61): one reduction per row
            fe_acc A;
            fe_acc_zero(A);
#pragma unroll
            for (int j = 0; j < 6; j++) fe_acc_mac(A, s[j], RESCUE_MDS(i * 6 + j));
            r[i] = fe_acc_reduce(A);
        }
#pragma unroll
        for (int i = 0; i < 6; i++) s[i] = r[i];
    }
}

// digest of (v0, v1, v2, v3): hasher.rs:16-25 reverses the state on the way in and on the way out
__device__ __forceinline__ void rescue_digest4(const fe& v0, const fe& v1, const fe& v2, const fe& v3, fe& d0, fe& d1) {
    fe s[6] = {fe_zero(), fe_zero(), v3, v2, v1, v0};
    rescue_permute6(s);
    d0 = s[5]; d1 = s[4];
}

// one state element per lane: lane e (0..5) of a group of eight holds state[e]; lanes 6 and 7 of the group only keep the barriers.
// xch = the group's eight LDS slots.  Every lane of the workgroup must call this (workgroup barriers inside).
__device__ __forceinline__ void rescue_permute_lane(fe& v, uint32_t e, fe* xch) {
    const uint32_t ec = e < 6u ? e : 5u;
#pragma unroll 1
    for (uint32_t h = 0; h < 2u * RESCUE_ROUNDS; h++) {
        fe s[1] = {fe_add(v, RESCUE_ARK(h, ec))};
        if (h & 1u) rescue_inv_sbox<1>(s);
        else s[0] = fe_cube(s[0]);
        xch[e] = s[0];
        __syncthreads();
        fe_acc A;
        fe_acc_zero(A);
#pragma unroll
        for (int j = 0; j < 6; j++) fe_acc_mac(A, xch[j], RESCUE_MDS(ec * 6u + j));
        v = fe_acc_reduce(A);
        __syncthreads();                                                 // everyone has read the state before the next half round overwrites it
    }
}
