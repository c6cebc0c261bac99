// AIR kernel instances for traces with <= 2 context registers, no loop register and a user stack of depth 4 (the
// Fibonacci shape): the depth-4 nested-sum formulation (air_kernel.h air_stack, air_stack_nested.h).  The evaluation is cut into five
// launches by constraint section (AS_*) and, for the stack, by operation group (AG_*): every one stays inside the register file without
// scratch and inside the 64 KiB instruction cache of a CU pair.
#include "air_kernel.h"
// the launches of the set, stated once: walked by the evaluation (air_kernel) and by the check of the trace rows (air_check_kernel)
template <class CHAIN>
static void air_chain_sd4(const CHAIN& ch) {
    ch.template boundary<2, 1, 4, 8>();                                          // boundary combinations by evaluation (test build only)
    ch.template run<2, 1, 4, 8, AS_OP_BITS | AS_FLOW, 0, AF_FIRST>();                // op bits, loop image, context / loop stacks (starts the partial sums)
    ch.template run<2, 1, 4, 8, AS_SPONGE, 0, 0>();                                  // sponge
    ch.template run<2, 1, 4, 8, 0, AG_HIGH, AF_EV_OUT>();                            // stack: PUSH, CMP, RESCR, BEGIN / NOOP
    ch.template run<2, 1, 4, 8, 0, AG_LOW0, AF_EV_IN | AF_EV_OUT>();                 // stack: low-degree operations 0x00 .. 0x0F, both auxiliary constraints
    ch.template run<2, 1, 4, 8, 0, AG_LOW1, AF_EV_IN | AF_LAST>();                   // stack: low-degree operations 0x10 .. 0x1F; emits the stack constraints; combination
}
void air_launch_sd4(dst_ctx* c, const AirArgs& a, uint32_t Q) { air_chain_sd4(AirEvalChain{c, a, Q}); }
void air_check_sd4(dst_ctx* c, const AirArgs& a, hipStream_t stream) { air_chain_sd4(AirCheckChain{c, a, stream}); }
