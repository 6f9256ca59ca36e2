// almpc_tu_cert_ltv.hip -- one translation unit of libalmpc.so: k_cert_ltv (predicted states, cost, costates, input gradient and KKT
// residual of a step of a time-varying design, one wave per instance).
// Device code only; the launch logic is in almpc_api.hip, which declares these instantiations `extern template` (see there).
#include "almpc_cert_ltv.hip.h"
#define ALMPC_KERNEL_INSTANCE(...) template __global__ __VA_ARGS__;
#include "instances/cert_ltv.inc"
