/* Host-side check of a proof before it leaves the box: stark::verify through the C-ABI (dst_verify), C99, the header and
 * libdistaff_hip.so only.  No GPU is touched: the call works on a machine without one.
 *
 *   cc -std=c99 -I include -o verify_proof examples/verify_proof.c -L distaff_amd -ldistaff_hip -Wl,-rpath,$PWD/distaff_amd
 *   ./verify_proof proof.bin <program hash, 64 hex digits> --inputs 1 0 --outputs <decimal> ...
 *
 * Prints "accepted" (exit 0), or the reference's error string / why the call was refused (exit 1).  Public values are decimal field
 * elements, at most 8 of each; the library refuses one that is not below p = 2^128 - 45 * 2^40 + 1. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "distaff_hip.h"

/* decimal -> 16 little-endian bytes */
static int parse_element(const char* s, uint8_t out[16]) {
    memset(out, 0, 16);
    if (!*s) return -1;
    for (; *s; s++) {
        unsigned carry;
        int i;
        if (*s < '0' || *s > '9') return -1;
        carry = (unsigned)(*s - '0');
        for (i = 0; i < 16; i++) { unsigned v = out[i] * 10u + carry; out[i] = (uint8_t)v; carry = v >> 8; }
        if (carry) return -1;
    }
    return 0;
}

static int hex_nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

int main(int argc, char** argv) {
    uint8_t program_hash[32];
    dst_public pub;
    dst_proof_info_t info;
    uint8_t* proof;
    long size;
    FILE* f;
    int i, accepted = 0, rc, mode = 0;
    char err[256];
    if (argc < 3 || strlen(argv[2]) != 64) { fprintf(stderr, "usage: %s proof.bin <program hash: 64 hex digits> [--inputs v ...] [--outputs v ...]\n", argv[0]); return 2; }
    for (i = 0; i < 32; i++) {
        int hi = hex_nibble(argv[2][2 * i]), lo = hex_nibble(argv[2][2 * i + 1]);
        if (hi < 0 || lo < 0) { fprintf(stderr, "program hash: not a hex digit\n"); return 2; }
        program_hash[i] = (uint8_t)(hi * 16 + lo);
    }
    memset(&pub, 0, sizeof(pub));
    for (i = 3; i < argc; i++) {
        if (!strcmp(argv[i], "--inputs")) { mode = 1; continue; }
        if (!strcmp(argv[i], "--outputs")) { mode = 2; continue; }
        if (mode == 1 && pub.num_inputs < 8 && !parse_element(argv[i], pub.inputs[pub.num_inputs])) { pub.num_inputs++; continue; }
        if (mode == 2 && pub.num_outputs < 8 && !parse_element(argv[i], pub.outputs[pub.num_outputs])) { pub.num_outputs++; continue; }
        fprintf(stderr, "cannot use argument '%s'\n", argv[i]);
        return 2;
    }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    size = ftell(f);
    fseek(f, 0, SEEK_SET);
    proof = (uint8_t*)malloc(size > 0 ? (size_t)size : 1);
    if (!proof || size < 0 || fread(proof, 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    rc = dst_verify(program_hash, &pub, proof, (size_t)size, &accepted, err, sizeof(err));
    if (rc != DST_OK) { printf("refused: %s\n", err); free(proof); return 1; }                 /* not a StarkProof, or a public value >= p */
    if (!accepted) { printf("rejected: %s\n", err); free(proof); return 1; }
    dst_proof_info(proof, (size_t)size, &info);
    printf("accepted: 2^%u steps, %u registers, extension %u, %u queries, grinding %u, security level %u bits\n", info.log_trace_length, info.register_count,
           info.extension_factor, info.num_queries, info.grinding_factor, info.security_level);
    free(proof);
    return 0;
}
