// almpc_tu_c2d.hip -- one translation unit of libalmpc.so: k_c2d (batched zero-order-hold discretisation, one wave per instance).
// Device code only; the launch logic is in almpc_api.hip, which declares these instantiations `extern template` (see there).
#include "almpc_c2d.hip.h"
#define ALMPC_KERNEL_INSTANCE(...) template __global__ __VA_ARGS__;
#include "instances/c2d.inc"
