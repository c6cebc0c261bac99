// Host helpers of context creation: powers of roots of unity on the host field (ctx.h's dev_upload takes them to the device).  Shared by
// ctx_init (api.hip: domain tables, periodic constants) and k_ntt_init (kernels_ntt.hip: every table of the transform plan).  Host code only.
#pragma once
#include <vector>
#include "../ctx.h"
#include "../host_vm.h"

static fe h_root_of_unity(uint32_t log_order) {               // field.rs:228: G^(2^(40 - log_order))
    const dsth::u128 G = (((dsth::u128)0x120532E7B364080Aull) << 64) | 0x86B8723E1920F4AAull;      // field.rs:14
    dsth::u128 r = G;
    for (uint32_t i = log_order; i < 40; i++) r = dsth::hf_mul(r, r);
    return dsth::fe_from_u128(r);
}
static std::vector<fe> h_powers(fe base, size_t count) {
    std::vector<fe> v(count);
    dsth::u128 b = dsth::fe_to_u128(base), cur = 1;
    for (size_t i = 0; i < count; i++) { v[i] = dsth::fe_from_u128(cur); cur = dsth::hf_mul(cur, b); }
    return v;
}
static std::vector<fe_tw> h_powers_tw(fe base, size_t count) {     // table pairs (w, w * 2^64 mod p) of the powers
    std::vector<fe_tw> v(count);
    dsth::u128 b = dsth::fe_to_u128(base), cur = 1;
    for (size_t i = 0; i < count; i++) { v[i] = fe_tw_make(dsth::fe_from_u128(cur)); cur = dsth::hf_mul(cur, b); }
    return v;
}
static fe h_inv(fe a) { return dsth::fe_from_u128(dsth::hf_pow(dsth::fe_to_u128(a), dsth::FIELD_P - 2)); }
static fe h_pow(fe a, dsth::u128 e) { return dsth::fe_from_u128(dsth::hf_pow(dsth::fe_to_u128(a), e)); }
