// almpc_tu_cert.hip -- one translation unit of libalmpc.so: k_cert (cost, costates, input gradient and KKT residual of a step, one
// wave per instance).
// Device code only; the launch logic is in almpc_api.hip, which declares these instantiations `extern template` (see there).
#include "almpc_cert.hip.h"
#define ALMPC_KERNEL_INSTANCE(...) template __global__ __VA_ARGS__;
#include "instances/cert.inc"
