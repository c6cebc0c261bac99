// TEST INFRASTRUCTURE (host build against the stand-in HIP header of this directory; work-items are fibers): the coset DIT of the first pass
// (ntt_lds.h: lds_dit_round / lds_dit_tail) with the one-sided lazy butterflies switched ON against the same rounds switched OFF, on a
// 64 x 4 tile (three rounds of two stages) and a 32 x 4 tile (two rounds and the single-stage tail), for every coset of blowup 8.
// The kernel below is the first pass's path through a tile as ntt_pass_a walks it: stage twiddles of the coset from the pre-scale table,
// bit-reversed fill with the column rotated by the row, the rounds, and the read-out that multiplies every element by a table value --
// where the lazy values end.  Both outputs must be equal byte for byte, and equal to the coset transform summed term by term.
// Inputs: random, all p - 1, alternating 0 / p - 1, and one made so that sums land in [p, 2^128) -- the only values the two forms
// represent differently (a fraction of 2^-82 of uniform data); how many elements of the lazy tiles are such values is printed.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "hip/hip_runtime.h"
#include "../../distaff_amd/csrc/ntt_lds.h"

#define THREADS 128
alignas(16) static thread_local unsigned char tile_smem[64 * 4 * 16 + 64 * 32];

template <bool LAZY>
__global__ void first_pass_tile(const fe* src, fe* dst, fe* raw, const fe_tw* prescale, const fe* tw4, uint32_t log_n1, uint32_t log_b, uint32_t j) {
    const uint32_t log_t = 2, T = 4, n1 = 1u << log_n1, count = n1 * T;
    fe* L = reinterpret_cast<fe*>(tile_smem);
    fe_tw* TW = reinterpret_cast<fe_tw*>(L + count);
    const uint32_t pmask = (1u << (log_b + log_n1)) - 1u;
    for (uint32_t i = threadIdx.x; i + 1 < n1; i += THREADS) {                 // as ntt_pass_a: entry i = block size 2^(lb+1), index k
        const uint32_t lb = 31u - (uint32_t)__clz(i + 1), k = i + 1 - (1u << lb);
        TW[i] = prescale[((j + (k << log_b)) << (log_n1 - lb - 1)) & pmask];
    }
    for (uint32_t idx = threadIdx.x; idx < count; idx += THREADS) {
        const uint32_t row = idx >> log_t, col = (idx + row) & (T - 1);
        L[lds_slot(__brev(row) >> (32 - log_n1), col, log_t)] = src[row * T + col];
    }
    __syncthreads();
    lds_ntt_dit<THREADS, NttKeepInLds, LAZY>(L, TW, log_n1, log_t, 1u, log_n1 + 1u);
    for (uint32_t idx = threadIdx.x; idx < count; idx += THREADS) { raw[idx] = L[idx]; dst[idx] = fe_mul(L[idx], tw4[idx]); }
}

static uint64_t rs = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
static const fe P_MINUS_1 = fe_make(FE_P0 - 1u, FE_P1, FE_P2, FE_P3);
static bool canonical(const fe& a) { return !(a.v[3] == FE_P3 && a.v[2] == FE_P2 && (a.v[1] > FE_P1 || (a.v[1] == FE_P1 && a.v[0] >= FE_P0))); }

int main() {
    const uint32_t log_b = 3, B = 1u << log_b;
    long bad = 0, tiles = 0, above = 0, elements = 0;
    for (uint32_t log_n1 = 5; log_n1 <= 6; log_n1++) {
        const uint32_t n1 = 1u << log_n1, count = n1 * 4, order = B * n1;
        fe g = fe_make(0x1920F4AAu, 0x86B8723Eu, 0xB364080Au, 0x120532E7u);                 // generator of the 2^40 roots of unity
        for (uint32_t i = log_b + log_n1; i < 40; i++) g = fe_sqr(g);                      // w of order B * n1
        std::vector<fe> pw(order);
        std::vector<fe_tw> prescale(order);
        pw[0] = fe_one();
        for (uint32_t i = 1; i < order; i++) pw[i] = fe_mul(pw[i - 1], g);
        for (uint32_t i = 0; i < order; i++) prescale[i] = fe_tw_make(pw[i]);
        std::vector<fe> tw4(count), src(count), on(count), off(count), raw_on(count), raw_off(count);
        for (uint32_t i = 0; i < count; i++) tw4[i] = pw[(i * 7u + 1u) & (order - 1)];
        for (int input = 0; input < 4; input++) {
            // 3: p - 1 in the lower half of the rows, 1 in the upper: the first stage of coset 0 adds them to u + r = p exactly, which the lazy form
            // keeps as p (the canonical form gives 0) and carries through every later stage
            for (uint32_t i = 0; i < count; i++)
                src[i] = input == 0 ? fe_make((uint32_t)rnd(), (uint32_t)rnd(), (uint32_t)rnd(), (uint32_t)rnd() & 0x7FFFFFFFu)
                       : input == 3 ? ((i >> 2) < n1 / 2 ? P_MINUS_1 : fe_one()) : (input == 1 || ((i >> 2) & 1)) ? P_MINUS_1 : fe_zero();
            for (uint32_t j = 0; j < B; j++) {
                hipLaunchKernelGGL(first_pass_tile<true>, dim3(1), dim3(THREADS), 0, nullptr, src.data(), on.data(), raw_on.data(), prescale.data(), tw4.data(), log_n1, log_b, j);
                hipLaunchKernelGGL(first_pass_tile<false>, dim3(1), dim3(THREADS), 0, nullptr, src.data(), off.data(), raw_off.data(), prescale.data(), tw4.data(), log_n1, log_b, j);
                tiles++;
                for (uint32_t k = 0; k < n1; k++) for (uint32_t t = 0; t < 4; t++) {
                    fe want = fe_zero();                                                   // X[k] = sum_m x[m] g^(j m) w_n1^(m k), g w_n1 = w^(j + B k)
                    for (uint32_t m = 0; m < n1; m++) want = fe_add(want, fe_mul(src[m * 4 + t], pw[((uint64_t)m * (j + B * k)) & (order - 1)]));
                    const uint32_t idx = k * 4 + t;
                    elements++;
                    if (!canonical(raw_on[idx])) above++;
                    const bool ok = fe_eq(on[idx], off[idx]) && canonical(on[idx]) && canonical(raw_off[idx]) && fe_eq(raw_off[idx], want) && fe_eq(off[idx], fe_mul(want, tw4[idx]));
                    if (!ok) { if (bad < 10) printf("MISMATCH log_n1 %u input %d coset %u row %u column %u\n", log_n1, input, j, k, t); bad++; }
                }
            }
        }
    }
    printf("tiles %ld elements %ld mismatches %ld lazy results at or above p %ld\n", tiles, elements, bad, above);
    return bad ? 1 : 0;
}
