// The relayed dataflow sweep kernels with the order changes of a smooth! call folded in (csrc/hip/gs_relay.hpp, template flags
// PB / PX) for both value types, and nothing else: what tools/flow_asm_linear.py compiles to assembly when given this file, and
// what tools/relay_regs.py reads the register counts of (tests/test_flow_asm_perm_io.py).
#include "../algebraicmultigrid.jl_amd/csrc/hip/gs_relay.hpp"
namespace amgh { namespace bw {
template hipError_t sweep_relay_io<double>(const FlowArgs<double>&, int, size_t, size_t, bool, bool, hipStream_t);
template hipError_t sweep_relay_io<float>(const FlowArgs<float>&, int, size_t, size_t, bool, bool, hipStream_t);
} }
