// TEST INFRASTRUCTURE (host build, -DFE_EMULATE_GFX950: the limb-level dataflow of fe.h on plain integers): the one-sided lazy addition of
// the coset DIT.  Reads lines "u r w" (three 128-bit values in hex: u any value, r and w canonical) and prints, per line,
//   fe_add_lazy(u, r)   fe_addsub_lazy sum   fe_addsub_lazy dif   fe_mul_tw(sum, w)   fe_mul_wide(sum, w)   fe_mul_tw(dif, w)   fe_mul_wide(dif, w)
// tests/test_ntt_lazy_dit.py makes the operands and checks every figure against Python integers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../distaff_amd/csrc/fe.h"

static fe parse(const char* s) {
    unsigned __int128 v = 0;
    for (; *s; s++) v = (v << 4) | (unsigned)(*s <= '9' ? *s - '0' : (*s | 32) - 'a' + 10);
    return fe_make((uint32_t)v, (uint32_t)(v >> 32), (uint32_t)(v >> 64), (uint32_t)(v >> 96));
}
static void put(const fe& a, char end) { printf("%08x%08x%08x%08x%c", a.v[3], a.v[2], a.v[1], a.v[0], end); }

int main() {
    char u[64], r[64], w[64];
    while (scanf("%40s %40s %40s", u, r, w) == 3) {
        const fe U = parse(u), R = parse(r), Wv = parse(w);
        const fe_tw T = fe_tw_make(Wv);
        fe sum, dif;
        fe_addsub_lazy(U, R, sum, dif);
        put(fe_add_lazy(U, R), ' '); put(sum, ' '); put(dif, ' ');
        put(fe_mul_tw(sum, T), ' '); put(fe_mul_wide(sum, Wv), ' '); put(fe_mul_tw(dif, T), ' '); put(fe_mul_wide(dif, Wv), '\n');
    }
    return 0;
}
