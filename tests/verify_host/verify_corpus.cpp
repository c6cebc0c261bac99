// TEST INFRASTRUCTURE: the library's host-side verifier (distaff_amd/csrc/verify/host_verify.h) as a program of its own, compiled by g++ for the
// CPU -- with -fsanitize=address,undefined by tests/test_verify_host.py, and without any HIP library on the link line (that it links shows the
// verifier makes no hip* call).  Reads a corpus file
//     program_hash[32] | u32 num_inputs | u32 num_outputs | inputs x16 | outputs x16 | u32 count | count x (u64 length | bytes)
// and prints one line per item: "A" accepted, "R <reason>" rejected, "M <reason>" malformed.  Exit status 0 unless the corpus itself is unreadable.
#include <stdio.h>
#include <stdlib.h>
#include "verify/host_verify.h"
using namespace dsth;
using namespace dsth::hver;

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> data;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + k);
    fclose(f);
    size_t o = 0;
    auto need = [&](size_t n) { if (n > data.size() - o) { fprintf(stderr, "corpus truncated\n"); exit(2); } };
    need(40);
    uint8_t program_hash[32];
    memcpy(program_hash, data.data(), 32); o = 32;
    uint32_t nin, nout, count;
    memcpy(&nin, data.data() + o, 4); memcpy(&nout, data.data() + o + 4, 4); o += 8;
    if (nin > 8 || nout > 8) { fprintf(stderr, "too many public values\n"); return 2; }
    u128 in[8], out[8];
    need((size_t)(nin + nout) * 16 + 4);
    memcpy(in, data.data() + o, nin * 16); o += nin * 16;
    memcpy(out, data.data() + o, nout * 16); o += nout * 16;
    memcpy(&count, data.data() + o, 4); o += 4;
    for (uint32_t i = 0; i < count; i++) {
        need(8);
        uint64_t len;
        memcpy(&len, data.data() + o, 8); o += 8;
        need(len);
        std::vector<uint8_t> item(data.begin() + o, data.begin() + o + len);   // a copy of exactly `len` bytes: a read past the end is a heap overflow the sanitizer sees
        o += len;
        VProof p;
        std::string why;
        if (parse_proof(item.data(), item.size(), p, why)) { printf("M %s\n", why.c_str()); continue; }
        VerifyResult r = verify_proof(program_hash, in, nin, out, nout, p);
        if (r.ok) printf("A\n"); else printf("R %s\n", r.error.c_str());
    }
    return 0;
}
