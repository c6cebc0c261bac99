// host_proof.h alone, as a filter: the opening plan the library derives from a set of indices, printed so that a test can hold it against
// the oracle's MerkleTree::prove_batch and against the Python statement of the same plan (distaff_amd/sharded.py).  One request per line
// of stdin, one line of JSON per request on stdout:
//   batch <num_leaves> <count> <index>...           -> {"values": [...], "nodes": [[[is_leaf, index], ...], ...], "depth": d}
//   positions <domain_size> <layers> <count> <p>... -> {"constraint": [...], "augmented": [[...] per layer, each from the one before]}
// Built with sanitizers and run by tests/test_openings_plan_host.py.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "host_proof.h"

static void print_list(const std::vector<uint64_t>& v) {
    printf("[");
    for (size_t i = 0; i < v.size(); i++) printf("%s%" PRIu64, i ? ", " : "", v[i]);
    printf("]");
}

int main() {
    std::string line;
    size_t served = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string what;
        uint64_t size = 0, layers = 0, count = 0;
        in >> what >> size;
        if (what == "positions") in >> layers;
        in >> count;
        std::vector<uint64_t> idx(count);
        for (uint64_t& v : idx) in >> v;
        if (!in || (what != "batch" && what != "positions")) { fprintf(stderr, "bad request: %s\n", line.c_str()); return 2; }
        if (what == "batch") {
            const dsth::BatchPlan p = dsth::plan_batch(idx, size);
            printf("{\"values\": ");
            print_list(p.values);
            printf(", \"nodes\": [");
            for (size_t i = 0; i < p.nodes.size(); i++) {
                printf("%s[", i ? ", " : "");
                for (size_t k = 0; k < p.nodes[i].size(); k++) printf("%s[%d, %" PRIu64 "]", k ? ", " : "", p.nodes[i][k].is_leaf ? 1 : 0, p.nodes[i][k].index);
                printf("]");
            }
            printf("], \"depth\": %u}\n", (unsigned)p.depth);
        } else {
            printf("{\"constraint\": ");
            print_list(dsth::constraint_positions(idx));
            printf(", \"augmented\": [");
            std::vector<uint64_t> pos = idx;
            for (uint64_t d = 0; d < layers; d++, size /= 4) {             // as the proof's FRI layers chain them
                pos = dsth::augmented_positions(pos, size);
                if (d) printf(", ");
                print_list(pos);
            }
            printf("]}\n");
        }
        served++;
    }
    printf("{\"served\": %zu}\n", served);                                  // stderr stays empty unless a sanitizer speaks
    return 0;
}
