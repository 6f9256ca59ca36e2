// almpc_tu_dare.hip -- one translation unit of libalmpc.so: k_dare (batched DARE, one wave per instance) and
// k_dare_vjp (its adjoint).
// Device code only; the launch logic is in almpc_api.hip, which declares these instantiations `extern template` (see there).
#include "almpc_dare_vjp.hip.h"
#define ALMPC_KERNEL_INSTANCE(...) template __global__ __VA_ARGS__;
#include "instances/dare.inc"
