// almpc_tu_ltv_stage.hip -- one translation unit of libalmpc.so: k_ltv_stage_prepare and k_ltv_stage_finish (the trajectory data of
// almpc_design_ltv_stagewise / almpc_ltv_stagewise_update in the shape the stage-wise solvers read, and the step's absolute results).
// Device code only; the launch logic is in almpc_api.hip, which sees the declarations.
#define ALMPC_LTV_STAGE_TU
#include "almpc_ltv_stage.hip.h"
