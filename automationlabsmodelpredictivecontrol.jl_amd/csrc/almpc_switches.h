// almpc_switches.h -- the ALMPC_* diagnostic switches of libalmpc.so, host only (plain C++, no HIP).
//
// A switch is a property of a HANDLE: almpc_create reads the whole block once (almpc_handle::sw) and no later call into the library
// looks at the environment again.  The two calls without a handle (almpc_fnn_linearize, almpc_densenet_linearize) read a block at
// their entry.  read_switches() is the only function under csrc/ that reads the environment.
//
// ONE table: the variable, the member of Switches it fills, its parsing rule and what it does ("Diagnostic
// switches", holds the same list; tests/test_host_logic.py compares the names).  The rules are the ones each variable has always had:
//   ON_IF_1    on when the value starts with '1' (unset, empty or "0": off)
//   ON_IF_SET  on when the variable exists, whatever its value ("=0" switches it ON)
//   INTEGER    atol of the value when the variable exists, else no value (the code's own default applies)
#pragma once

#include <cstdlib>
#include <optional>

namespace almpc {

#define ALMPC_SWITCH_TABLE(X)                                                                                                                 \
    /* step path: the route of a step */                                                                                                      \
    X(ALMPC_NO_SHARED_WAVE, no_shared_wave, ON_IF_1, "small shared problems take the two-launch path, not the one-wave-per-instance step")     \
    X(ALMPC_SHARED_WAVE_MAX_BATCH, shared_wave_max_batch, INTEGER, "largest batch of the one-wave-per-instance shared step (default: 2 per CU)") \
    X(ALMPC_NO_INST_WAVE, no_inst_wave, ON_IF_1, "small per-instance problems take the two-launch path, not the one-wave-per-instance step")   \
    X(ALMPC_NO_FUSED_STEP, no_fused_step, ON_IF_1, "a handle starts with step fusion off (almpc_set_step_fusion still overrides)")            \
    X(ALMPC_POLISH_NO_GLDS, polish_no_glds, ON_IF_1, "the finish reads G through L2 (k_polish<false>), never from LDS")                       \
    X(ALMPC_POLISH_SG_GLOBAL, polish_sg_global, ON_IF_SET, "the finish keeps its second-tier inverse in the global scratch, not in LDS")      \
    X(ALMPC_NO_GUESS_WS, no_guess_ws, ON_IF_SET, "an SQP iteration's guess does not build the inverse of its working set (k_guess_iterate)")  \
    X(ALMPC_NO_REDO_START, no_redo_start, ON_IF_SET, "the finish does not keep the working sets it gave up with for a stage-wise redo")       \
    X(ALMPC_X0_UPLOAD, x0_upload, ON_IF_1, "the copy engine uploads x0 into a device slot; default: the kernels read the pinned slot in place") \
    /* step path: the redo of what a step left undecided */                                                                                   \
    X(ALMPC_EAGER_REDO, eager_redo, ON_IF_SET, "the redo is enqueued behind every step instead of deferred to the next look at the results")  \
    X(ALMPC_NO_GATED_REDO, no_gated_redo, ON_IF_SET, "no gated redo on the stream: a deferred redo waits for a synchronous look")             \
    X(ALMPC_NO_PREDICTED_REDO, no_predicted_redo, ON_IF_SET, "no gated redo ahead of a wait after a step that left instances undecided")      \
    X(ALMPC_DBG_NO_SDUAL_FB, dbg_no_sdual_fb, ON_IF_SET, "the redo skips the stage-wise dual solver")                                         \
    X(ALMPC_DBG_NO_PRIMAL_NET, dbg_no_primal_net, ON_IF_SET, "the redo skips the primal Riccati active set")                                  \
    X(ALMPC_RICCATI_GENERIC, riccati_generic, ON_IF_SET, "k_riccati in its generic build, not the one specialised for (n, m)")                \
    /* stage-wise dual solver (k_sdual) */                                                                                                    \
    X(ALMPC_SDUAL_NO_GHAT, sdual_no_ghat, ON_IF_SET, "no table of cached sweep responses: every working-set change costs two sweeps")         \
    X(ALMPC_SDUAL_NO_GH, sdual_no_gh, ON_IF_SET, "the table is built but the solve runs the kernel variant without it")                       \
    X(ALMPC_SDUAL_NO_SINV_HANDOVER, sdual_no_sinv_handover, ON_IF_SET, "tiers do not hand each other the inverse of their working set")       \
    X(ALMPC_SDUAL_NO_SCREEN, sdual_no_screen, ON_IF_SET, "no reachability screen of the state box in front of the solve")                     \
    X(ALMPC_SDUAL_REDO_128, sdual_redo_128, ON_IF_SET, "a single-launch redo is the one 128-row launch, not the 64-row build first")          \
    X(ALMPC_SDUAL_NO_START_BUILD, sdual_no_start_build, ON_IF_SET, "a redo's start is not built from the cached responses (k_sdual_start)")   \
    /* design: shared and structured handles */                                                                                               \
    X(ALMPC_NO_S0_BASIS, no_s0_basis, ON_IF_SET, "no table of the state rows' s0: the finish rolls v0 out")                                   \
    X(ALMPC_NO_EQ_PROJECTION, no_eq_projection, ON_IF_SET, "the constraint-space matrix is not projected on the terminal equality")           \
    X(ALMPC_ROLLOUT_STAGEWISE, rollout_stagewise, ON_IF_SET, "the stage-by-stage rollout, not the blocked one")                               \
    X(ALMPC_STRUCTURED_PRIMAL, structured_primal, ON_IF_SET, "a structured handle does not use the stage-wise dual solver")                   \
    X(ALMPC_DESIGN_TRACE, design_trace, ON_IF_SET, "almpc_design_shared prints the time of each of its phases")                               \
    /* design: per-instance models, time-varying models, SQP */                                                                               \
    X(ALMPC_INV_TILE, inv_tile, ON_IF_SET, "the batched inverse in its register-tile kernels (no one-wave, no column-split kernel)")           \
    X(ALMPC_INV_CW, inv_columns_per_wave, INTEGER, "columns per wave of the column-split inverse: 8, 16 or 32 (default: by grid size)")       \
    X(ALMPC_NO_RHO_FUSION, no_rho_fusion, ON_IF_SET, "the penalty profile by k_design_rho, not inside the inverse's launch")                  \
    X(ALMPC_NO_PACKED_MINV, no_packed_minv, ON_IF_SET, "the KKT inverse of per-instance models as a full matrix, not a packed triangle")      \
    X(ALMPC_DBG_SPLIT_NEGGM, dbg_split_neggm, ON_IF_SET, "V = -G F' by a launch of its own, not inside the inverse's")                        \
    X(ALMPC_DBG_SPLIT_INVERSES, dbg_split_inverses, ON_IF_SET, "the two inverses of a per-instance design in two launches")                   \
    X(ALMPC_DBG_SPLIT_SCALE, dbg_split_scale, ON_IF_SET, "the Jacobi scaling by k_design_scale, not inside the design kernel")                \
    X(ALMPC_DBG_SPLIT_PREPARE, dbg_split_prepare, ON_IF_SET, "an SQP iteration's stage data by a launch of its own, not inside k_design_ltv")  \
    X(ALMPC_DBG_SPLIT_JACOBIAN, dbg_split_jacobian, ON_IF_SET, "the network's Jacobians by a launch in front of the design, not inside it")   \
    X(ALMPC_LTV_LDS, ltv_lds, ON_IF_SET, "k_design_ltv with its accumulators in LDS, not in registers")                                       \
    X(ALMPC_FNN_WG, fnn_wg, ON_IF_SET, "network Jacobians by one workgroup per point, not one wave per point")                                \
    X(ALMPC_FNN_ONE_POINT_PER_WAVE, fnn_one_point_per_wave, ON_IF_SET, "small networks: one point per wave, not one per half-wave")           \
    X(ALMPC_SQP_ADMM_ALWAYS, sqp_admm_always, ON_IF_1, "every SQP iteration runs the ADMM phase, not only the first")                         \
    X(ALMPC_SQP_REDO_DUAL_FIRST, sqp_redo_dual_first, ON_IF_SET, "an SQP iteration's redo runs the dual solver even where the primal one suffices")

#define ALMPC_SWITCH_TYPE_ON_IF_1 bool
#define ALMPC_SWITCH_TYPE_ON_IF_SET bool
#define ALMPC_SWITCH_TYPE_INTEGER std::optional<long>
#define ALMPC_SWITCH_READ_ON_IF_1(v) ((v) != nullptr && (v)[0] == '1')
#define ALMPC_SWITCH_READ_ON_IF_SET(v) ((v) != nullptr)
#define ALMPC_SWITCH_READ_INTEGER(v) ((v) != nullptr ? std::optional<long>(std::atol(v)) : std::nullopt)

struct Switches {
#define X(name, member, rule, text) ALMPC_SWITCH_TYPE_##rule member{};
    ALMPC_SWITCH_TABLE(X)
#undef X
};

inline Switches read_switches() {
    Switches sw;
#define X(name, member, rule, text) { const char* v = std::getenv(#name); sw.member = ALMPC_SWITCH_READ_##rule(v); }
    ALMPC_SWITCH_TABLE(X)
#undef X
    return sw;
}

}  // namespace almpc
