// almpc_tu_sens.hip -- one translation unit of libalmpc.so: k_sens and k_sens_pz (solution sensitivities and parameter gradients
// after a step, two tiers each), k_sens_face and k_sens_face_rate (the same on structured handles, without and with S).
// Device code only; the launch logic is in almpc_api.hip, which declares these instantiations `extern template` (see there).
#include "almpc_sens.hip.h"
#define ALMPC_KERNEL_INSTANCE(...) template __global__ __VA_ARGS__;
#include "instances/sens.inc"
