// The user-stack constraints operation by operation: flag(op) * term(op, slot) added up with the shift helpers of
// constraints/stack/mod.rs:199-262, as the reference states them.  It exists only in the test build (DISTAFF_AIR=generic, instances
// air_kernel<16,8,0,32,...>) as a statement of the constraints that shares nothing with the nested sums of air_stack_nested.h, which the
// tests compare with it: its own shift helpers, its own RESCR and CMP.  Keep it that way.
//
// Included by air_kernel.h alone, after the definitions it uses (AirConsts, AirFlags, Acc, matmul, the AS_* section bits).
#pragma once

// SECT selects what a launch adds up (AS_STACK_MOVE, AS_STACK_ARITH, AS_STACK_HIGH, AS_STACK_RESCR); every launch emits what it has:
// the constraints are linear in the flags, and so is the combination.  o / nw: the stack slices (SL items) of the current / next row,
// sl <= SL their length, sd the stack depth, sbase the index of the first auxiliary constraint.
template <int SL, int SECT, class ACC>
__device__ __forceinline__ void air_stack_per_operation(ACC& acc, const fe (&o)[SL], const fe (&nw)[SL], int sl, int sd, uint32_t sbase,
                                                        const AirFlags& fl, const fe* per, const AirConsts* consts) {
    fe ev[SL], aux0 = fe_zero(), aux1 = fe_zero();
#pragma unroll
    for (int i = 0; i < SL; i++) ev[i] = fe_zero();
    auto LDF = [&](int idx) { return fl.ldf(idx); };
    auto agg = [&](int i, const fe& f, const fe& v) { if (i < sd) ev[i] = fe_add(ev[i], fe_mul(f, v)); };
    auto copy_from = [&](int from, const fe& f) {
#pragma unroll
        for (int i = 0; i < SL; i++) if (i >= from && i < sl) agg(i, f, fe_sub(o[i], nw[i]));
    };
    auto rshift = [&](int num, const fe& f) {
#pragma unroll
        for (int i = 0; i < SL; i++) if (i >= num && i < sl) agg(i, f, fe_sub(o[i - num < 0 ? 0 : i - num], nw[i]));
    };
    auto lshift = [&](int from, int num, const fe& f) {
#pragma unroll
        for (int i = 0; i < SL; i++) {
            if (i >= from - num && i < sl - num) agg(i, f, fe_sub(o[i + num < SL ? i + num : 0], nw[i]));
            else if (i >= sl - num && i < sl) agg(i, f, nw[i]);
        }
    };
    fe f;
    if constexpr ((SECT & AS_STACK_MOVE) != 0) {      // low-degree ops that only move stack items
        // flags that only shift / copy are merged before the multiplications
        // right shift by 1: READ (0x10), DUP (0x12)  (PUSH is with the high-degree ops)
        f = LDF(0x12); agg(0, f, fe_sub(nw[0], o[0]));
        rshift(1, fe_add(LDF(0x10), f));
        // right shift by 2: READ2 (0x11), DUP2 (0x13), PAD2 (0x15)
        f = LDF(0x13); agg(0, f, fe_sub(nw[0], o[0])); agg(1, f, fe_sub(nw[1], o[1]));
        f = LDF(0x15); agg(0, f, nw[0]); agg(1, f, nw[1]);
        rshift(2, fe_add(fe_add(LDF(0x11), LDF(0x13)), LDF(0x15)));
        // DUP4 (0x14)
        f = LDF(0x14);
#pragma unroll
        for (int i = 0; i < 4; i++) agg(i, f, fe_sub(nw[i], o[i]));
        rshift(4, f);
        // left shift (1,1): ASSERT (0x00), DROP (0x03)
        lshift(1, 1, fe_add(fl.assert_flag, LDF(0x03)));
        aux0 = fe_add(aux0, fe_mul(fl.assert_flag, fe_sub(fe_one(), o[0])));
        // ASSERTEQ (0x01): left shift (2,2)
        lshift(2, 2, LDF(0x01));
        aux0 = fe_add(aux0, fe_mul(LDF(0x01), fe_sub(o[0], o[1])));
        // DROP4 (0x04)
        lshift(4, 4, LDF(0x04));
        // SWAP (0x18): both constraints land in slot 0 (manipulation.rs:63-64)
        f = LDF(0x18); agg(0, f, fe_sub(nw[0], o[1])); agg(0, f, fe_sub(nw[1], o[0])); copy_from(2, f);
        // SWAP2 (0x19)
        f = LDF(0x19); agg(0, f, fe_sub(nw[0], o[2])); agg(1, f, fe_sub(nw[1], o[3])); agg(2, f, fe_sub(nw[2], o[0])); agg(3, f, fe_sub(nw[3], o[1])); copy_from(4, f);
        // SWAP4 (0x1A)
        f = LDF(0x1A);
#pragma unroll
        for (int i = 0; i < 4; i++) { agg(i, f, fe_sub(nw[i], o[4 + i])); agg(4 + i, f, fe_sub(nw[4 + i], o[i])); }
        copy_from(8, f);
        // ROLL4 (0x1B), ROLL8 (0x1C)
        f = LDF(0x1B); agg(0, f, fe_sub(nw[0], o[3]));
#pragma unroll
        for (int i = 1; i < 4; i++) agg(i, f, fe_sub(nw[i], o[i - 1]));
        copy_from(4, f);
        f = LDF(0x1C); agg(0, f, fe_sub(nw[0], o[7]));
#pragma unroll
        for (int i = 1; i < 8; i++) agg(i, f, fe_sub(nw[i], o[i - 1]));
        copy_from(8, f);
    }
    if constexpr ((SECT & AS_STACK_ARITH) != 0) {     // low-degree arithmetic / selection ops
        // ADD (0x08), MUL (0x09), AND (0x0A), OR (0x0B): left shift (2,1)
        {
            fe xy = fe_mul(o[0], o[1]);
            agg(0, LDF(0x08), fe_sub(nw[0], fe_add(o[0], o[1])));
            agg(0, fe_add(LDF(0x09), LDF(0x0A)), fe_sub(nw[0], xy));
            agg(0, LDF(0x0B), fe_sub(nw[0], bnot(fe_mul(bnot(o[0]), bnot(o[1])))));
            lshift(2, 1, fe_add(fe_add(LDF(0x08), LDF(0x09)), fe_add(LDF(0x0A), LDF(0x0B))));
            fe b0 = is_bin(o[0]), b1 = is_bin(o[1]);
            fe andor = fe_add(LDF(0x0A), LDF(0x0B));
            aux0 = fe_add(aux0, fe_mul(fe_add(andor, LDF(0x0E)), b0));            // NOT also checks operand 0
            aux1 = fe_add(aux1, fe_mul(andor, b1));
        }
        // INV (0x0C), NEG (0x0D), NOT (0x0E): copy from 1
        agg(0, LDF(0x0C), fe_sub(fe_one(), fe_mul(nw[0], o[0])));
        agg(0, LDF(0x0D), fe_add(nw[0], o[0]));
        agg(0, LDF(0x0E), fe_sub(nw[0], bnot(o[0])));
        copy_from(1, fe_add(fe_add(LDF(0x0C), LDF(0x0D)), LDF(0x0E)));
        // EQ (0x02)
        {
            f = LDF(0x02);
            fe diff = fe_sub(o[1], o[2]);
            agg(0, f, fe_sub(nw[0], bnot(fe_mul(diff, o[0]))));
            lshift(3, 2, f);
            aux0 = fe_add(aux0, fe_mul(f, fe_mul(nw[0], diff)));
        }
        // BINACC (0x1D)
        {
            f = LDF(0x1D);
            agg(0, f, is_bin(nw[0])); agg(1, f, nw[1]);
            agg(2, f, fe_sub(nw[2], fe_double(o[2])));
            agg(3, f, fe_sub(nw[3], fe_add(o[3], fe_mul(nw[0], o[2]))));
            copy_from(4, f);
        }
        // CHOOSE (0x05), CHOOSE2 (0x06), CSWAP2 (0x07)
        {
            f = LDF(0x05);
            fe c = o[2], nc = bnot(c);
            agg(0, f, fe_sub(nw[0], fe_add(fe_mul(c, o[0]), fe_mul(nc, o[1]))));
            lshift(3, 2, f);
            aux0 = fe_add(aux0, fe_mul(f, is_bin(c)));
            c = o[4]; nc = bnot(c);
            fe binc = is_bin(c);
            f = LDF(0x06);
            agg(0, f, fe_sub(nw[0], fe_add(fe_mul(c, o[0]), fe_mul(nc, o[2]))));
            agg(1, f, fe_sub(nw[1], fe_add(fe_mul(c, o[1]), fe_mul(nc, o[3]))));
            lshift(6, 4, f);
            aux0 = fe_add(aux0, fe_mul(f, binc));
            f = LDF(0x07);
            agg(0, f, fe_sub(nw[0], fe_add(fe_mul(c, o[2]), fe_mul(nc, o[0]))));
            agg(1, f, fe_sub(nw[1], fe_add(fe_mul(c, o[3]), fe_mul(nc, o[1]))));
            agg(2, f, fe_sub(nw[2], fe_add(fe_mul(c, o[0]), fe_mul(nc, o[2]))));
            agg(3, f, fe_sub(nw[3], fe_add(fe_mul(c, o[1]), fe_mul(nc, o[3]))));
            lshift(6, 2, f);
            aux0 = fe_add(aux0, fe_mul(f, binc));
        }
    }
    if constexpr ((SECT & AS_STACK_HIGH) != 0) {      // PUSH, CMP, BEGIN / NOOP
        rshift(1, fl.hdf[0]);                                          // PUSH (input.rs:6)
        // CMP (hd 1) (comparison.rs:64-105)
        {
            f = fl.hdf[1];
            fe x_bit = nw[1], y_bit = nw[2], not_set = nw[3];
            agg(0, f, is_bin(x_bit)); agg(1, f, is_bin(y_bit));
            fe bit_gt = fe_mul(x_bit, bnot(y_bit)), bit_lt = fe_mul(y_bit, bnot(x_bit));
            agg(2, f, fe_sub(nw[4], fe_add(o[4], fe_mul(bit_gt, not_set))));
            agg(3, f, fe_sub(nw[5], fe_add(o[5], fe_mul(bit_lt, not_set))));
            agg(4, f, fe_sub(nw[6], fe_add(o[6], fe_mul(y_bit, o[0]))));
            agg(5, f, fe_sub(nw[7], fe_add(o[7], fe_mul(x_bit, o[0]))));
            agg(6, f, fe_sub(not_set, fe_mul(bnot(o[5]), bnot(o[4]))));
            agg(7, f, fe_sub(fe_double(nw[0]), o[0]));
            copy_from(8, f);
        }
        // BEGIN and NOOP leave the stack untouched
        copy_from(0, fe_add(fl.begin_flag, fl.noop_flag));
    }
    if constexpr ((SECT & AS_STACK_RESCR) != 0) {     // RESCR (hd 2) (hash.rs:9-35)
        f = fl.hdf[2];
        fe os[6], ns[6];
#pragma unroll
        for (int i = 0; i < 6; i++) os[i] = fe_cube(fe_add(o[i], per[8 + i]));
        matmul<6>(os, consts->hasher_mds);
#pragma unroll
        for (int i = 0; i < 6; i++) ns[i] = nw[i];
        matmul<6>(ns, consts->hasher_inv_mds);
#pragma unroll
        for (int i = 0; i < 6; i++) ns[i] = fe_sub(fe_cube(ns[i]), per[14 + i]);
#pragma unroll
        for (int i = 0; i < 6; i++) agg(i, f, fe_sub(ns[i], os[i]));
        copy_from(6, f);
    }

    if constexpr ((SECT & AS_STACK_AUX) != 0) { acc.emit(sbase, 4, aux0); acc.emit(sbase + 1, 4, aux1); }    // only low-degree ops touch the aux constraints
#pragma unroll
    for (int i = 0; i < SL; i++) if (i < sd) acc.emit(sbase + 2 + i, 4, ev[i]);
}
