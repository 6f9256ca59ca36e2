// almpc_tu_sens_ltv.hip -- one translation unit of libalmpc.so: k_sens_ltv (K0, du/dx0, dx/dx0 and the VJP of a step of a time-varying
// design in its initial deviation: the Riccati recursion on the face with one model per stage, one wave per instance).
// Device code only; the launch logic is in almpc_api.hip, which declares these instantiations `extern template` (see there).
#include "almpc_sens_ltv.hip.h"
#define ALMPC_KERNEL_INSTANCE(...) template __global__ __VA_ARGS__;
#include "instances/sens_ltv.inc"
