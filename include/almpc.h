/*
 * almpc.h -- C ABI of libalmpc.so, the MI355X (gfx950) batched condensed-QP MPC solve engine.
 *
 * Drop-in boundary for ONE path of AutomationLabsModelPredictiveControl.jl (reference paths are
 * relative to /root/reference): the per-step solve that the reference runs through
 *   JuMP.Model(OSQP.Optimizer)             src/sub/solver_selection.jl:92-98   (solver slot)
 *   update_initialization!(C, x0)           src/main/computation_mpc.jl:17-29
 *   calculate!(C)                           src/main/computation_mpc.jl:38-55
 * on the QP posed by
 *   _model_predictive_control_modeler_implementation(::LinearProgramming, ...)
 *                                           src/sub/model_modeler_implementation/linear/mpc_modeler_implementation_linear.jl:20-103
 *   _create_weights_coefficients            src/sub/design_mpc.jl:264-283
 *   _create_terminal_ingredient             src/sub/design_mpc.jl:298-394
 *   _create_quadratic_cost_function         src/sub/design_mpc.jl:405-468
 * for a BATCH of independent controller instances that share (A, B, weights, box).
 *
 * Conventions
 *  - every matrix is column-major Float64, i.e. the memory of a Julia Matrix{Float64}
 *    (zero-copy `ccall` with Ptr{Float64}); batch is the slowest axis:
 *    x0[batch][n], u[batch][N][m], x[batch][N+1][n]  ==  Julia Array{Float64,3}(m, N, batch) etc.
 *  - the caller owns every host buffer; the library owns device memory behind the handle.
 *  - every entry point returns 0 (ALMPC_OK) or a negative almpc_status; nothing throws across
 *    the boundary; almpc_last_error(h) gives the message of the last failure on that handle.
 *  - per-instance solver outcome goes to status[] (almpc_solve_status), never to the return code.
 *  - a handle is bound to one HIP device and one stream; it is not thread-safe; distinct handles
 *    are independent.  One process per GPU: multi-GPU runs create one handle per rank on its own
 *    shard of the batch (instances never interact, so there is no data-path collective).
 *  - there is NO CPU fallback: if no gfx950 device is usable almpc_create fails with
 *    ALMPC_ERR_NO_DEVICE.
 */
#ifndef ALMPC_H
#define ALMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALMPC_VERSION_MAJOR 0
#define ALMPC_VERSION_MINOR 1

typedef struct almpc_handle almpc_handle;

typedef enum almpc_status {
    ALMPC_OK = 0,
    ALMPC_ERR_INVALID = -1,      /* bad argument (null pointer, non-positive size, ...)          */
    ALMPC_ERR_NO_DEVICE = -2,    /* no usable HIP device / device id out of range                */
    ALMPC_ERR_HIP = -3,          /* a HIP runtime call failed (message in almpc_last_error)      */
    ALMPC_ERR_UNSUPPORTED = -4,  /* size or option outside what the kernels are built for        */
    ALMPC_ERR_NOT_DESIGNED = -5, /* calculate/get before design                                  */
    ALMPC_ERR_NUMERIC = -6       /* design-time numerical failure (DARE / Cholesky)              */
} almpc_status;

/* per-instance outcome written by almpc_calculate */
typedef enum almpc_solve_status {
    ALMPC_SOLVED = 0,          /* KKT conditions hold: ADMM met its tolerance and/or the polish certified */
    ALMPC_MAX_ITER = 1,        /* ADMM hit max_iter and polish was off or hit its own cap                   */
    ALMPC_NON_FINITE = 2,      /* a non-finite value appeared (bad inputs)                                  */
    ALMPC_INFEASIBLE = 3       /* state rows only: no point satisfies the box / terminal equality           */
} almpc_solve_status;

/*
 * Solver options.  The ADMM fields are OSQP's settings of the same name (the reference builds
 * OSQP.Optimizer without attributes, src/sub/solver_selection.jl:94-95, i.e. OSQP defaults:
 * rho 0.1, sigma 1e-6, alpha 1.6, eps_abs = eps_rel = 1e-3, check_termination 25, max_iter 4000,
 * polish off).  Defaults here differ in two documented places: `polish` is ON (it is what brings
 * u* within 1e-5 of the exact optimum) and `max_iter` is 25, one check interval (ADMM only has to
 * identify the active set for the polish).  almpc_default_opts fills the defaults.
 */
typedef struct almpc_opts {
    double rho;
    double sigma;
    double alpha;
    double eps_abs;
    double eps_rel;
    int32_t max_iter;
    int32_t check_every;
    int32_t polish;           /* 0 off, 1 on                                                   */
    int32_t polish_max_iter;  /* cap on active-set changes per instance; <=0 -> 2*nz+50        */
    int32_t warm_start;       /* 1: start ADMM from the previous step's (x, z, y) of each instance */
    int32_t reserved[3];      /* reserved[0]: flag bits ALMPC_OPT_*; the others must be 0            */
} almpc_opts;

/* opts.reserved[0] bits */
/* The ADMM state (x, y) of this step is NOT kept for a warm start of the next one (a cold-start-every-step caller, e.g. a Monte-Carlo
 * sweep, saves their 2 * nz doubles of HBM writes per instance; the polish gets the signs of y as 4 bytes per 16 rows).  Results
 * are identical.  The next almpc_calculate on the handle must then not ask for warm_start (ALMPC_ERR_INVALID).  Shared-model
 * steps with polish = 1 only; ignored otherwise. */
#define ALMPC_OPT_NO_WARM_STATE 0x1
/* A/B control of the cold start's first ADMM iterate.  With x = z = y = 0 the first iterate -Minv f' is affine in e0 = x0 - x_ref[:,1]
 * and a shared-model step takes it from an n-column product (W e0 + wS, W = -Minv F' from the design, wS = -Minv fS from
 * almpc_set_reference).  With this bit the first iterate is a full nz x nz product like the others (the same iteration, summed in
 * another order: results agree to rounding).  The affine form needs wS and exists for SHARED references only: per-instance references
 * (almpc_set_reference with per_instance = 1), warm starts, per-instance models, and shapes whose design workspace has no room for wS
 * behind W (fewer than n + 9 rows of n * N rounded up to 32: N = 1 with large n) always take the full product; the bit is ignored there. */
#define ALMPC_OPT_FULL_FIRST_PRODUCT 0x2
/* A/B control of the one-kernel step's hand-off.  A shared-model step that runs as one kernel and keeps no warm state
 * (ALMPC_OPT_NO_WARM_STATE) passes the ADMM results (z, v0, the signs of y, the status, the processing order) to its finish through
 * the workgroup's LDS.  With this bit they make the round trip through global memory that every other step makes: the same
 * arithmetic on the same values, identical results.  Ignored by steps that keep the warm state, by the two-kernel path, by
 * per-instance models and by shapes without the finish's shared second-tier slot in LDS. */
#define ALMPC_OPT_HBM_HANDOFF 0x4

void almpc_default_opts(almpc_opts* opts);

/* flags for almpc_create */
#define ALMPC_FLAG_TIMING 0x1u /* record HIP events around every kernel of almpc_calculate */
/*
 * Structured (non-condensed) solve: the handle solves the multiple-shooting form the reference itself builds (states and inputs per
 * stage, dynamics as constraints: ..linear.jl:48-60) stage by stage -- no condensed Hessian, so no m*N <= 128 limit and no loss of
 * definiteness for open-loop unstable models over long horizons.  Solver: k_sdual, a dual active-set
 * method in constraint space whose Ghat columns are affine Riccati sweeps with the unconstrained feedback gains (the Riccati
 * recursion runs once per model, a working-set change costs two O(N (n^2 + n m)) sweeps): input box, STATE BOX on every stage
 * (..linear.jl:62-70), TERMINAL EQUALITY (src/sub/design_mpc.jl:330-331) and the INPUT-RATE WEIGHT S (src/sub/design_mpc.jl:423-446:
 * the stage state is then [e_k; v_{k-1}]); working sets up to 128 rows; infeasible instances are reported as ALMPC_INFEASIBLE.
 * Behind it, for an input box without S, k_riccati (primal active set with Riccati-recursion subproblems) takes the instances the dual
 * method leaves without a certificate (a saturated open-loop unstable plant: Ghat_WW numerically singular).
 * Limits: n + m <= 64 lanes (n <= 48 without S, n + m <= 48 with S; m <= 16), (N + 1)(n + m) doubles twice in 160 KB of LDS
 * (quadrotor: N <= 255); shapes outside them but inside n <= 32, m <= 16, m*N <= 1024 run k_riccati alone (input box only).
 * Entry points of such a handle: almpc_design_shared (xmin / xmax, almpc_set_terminal_equality, S honoured; rho / sigma unused),
 * almpc_design_batched (+ almpc_set_state_box), almpc_sqp_fnn_* (every QP of the loop in its stage-wise form), almpc_set_reference,
 * almpc_update_initialization(_device), almpc_calculate(_async) (opts.polish_max_iter caps the working-set changes; <= 0: 20 rows + 50),
 * almpc_get_results (iters: 0, polish_iters: scans + steps of the dual method), almpc_get_design (P only), almpc_comm_*.
 */
#define ALMPC_FLAG_STRUCTURED 0x2u

/*
 * Create a solver for `batch` instances of an (n states, m inputs, horizon N) controller on HIP
 * device `device_id`.  Supported: 1 <= m*N <= 128, 1 <= n <= 64 (ALMPC_FLAG_STRUCTURED: see there).
 */
int almpc_create(almpc_handle** out, int n, int m, int N, int batch, int device_id, uint32_t flags);
void almpc_destroy(almpc_handle* h);
const char* almpc_last_error(const almpc_handle* h);

/*
 * Design for a model shared by all instances (replaces _model_predictive_control_design for the
 * linear system, src/sub/design_mpc.jl:54-129).
 *   A n*n, B n*m, Q n*n, R m*m, S m*m (NULL -> 0), P n*n (NULL -> DARE(A,B,Q,R) as
 *   src/sub/design_mpc.jl:327), umin/umax m.  xmin/xmax n, or NULL: non-NULL adds the state box
 *   x_min <= x[:,k] <= x_max for k = 1..N+1, i.e. the reference's kw `mpc_state_constraint`
 *   (..linear.jl:62-70); needs n*N + m*N <= 512.  rho/sigma are fixed at design time because the
 *   shared KKT inverse depends on them.
 * Builds Phi, Gamma blocks, H = 2(Gamma' Qbar Gamma + Rbar + D'SbarD), F = 2 Gamma' Qbar Phi,
 * the Jacobi scaling, (H' + (sigma+rho) I)^-1 and H'^-1 on the device.
 */
/*
 * Terminal constraint e_x[:,N+1] == 0 (mpc_terminal_ingredient = "equality", src/sub/design_mpc.jl:330-331):
 * call with 1 BEFORE almpc_design_shared.  Problems with state rows (state box and/or terminal equality) are
 * finished by a dual active-set method in constraint space (k_polish_gen, working sets up to 32 rows; instances beyond that are
 * redone by k_polish_gen64, up to 64 rows; what is still undecided goes to the stage-wise redo of almpc_set_structured_fallback,
 * up to 128 rows); they require opts.polish = 1.
 */
int almpc_set_terminal_equality(almpc_handle* h, int on);

/*
 * ADMM penalty profile, call BEFORE almpc_design_shared.  0 (default): one scalar rho for every row, as OSQP does for
 * inequality rows.  1: stiffness-matched rho_i = rho / G_ii with G = H'^-1 (a diagonal preconditioning of the
 * constraint rows, the role OSQP's Ruiz scaling E plays): rows in soft directions of the Hessian get a small penalty.
 * On the benchmark plant this cuts the active-set work after 10 ADMM iterations by ~3x; `rho` of
 * almpc_design_shared is then the numerator (the benchmark uses 45 with 6 iterations: sweep in DESIGN.md section 4).
 */
int almpc_set_rho_profile(almpc_handle* h, int mode);

/*
 * Step fusion (default on): when the tile of 16 instances is 8 waves (nz in 113..128), polish = 1, no state rows and the
 * buffers fit LDS, a step is ONE kernel (ADMM phase, then the polish of the same 16 instances by the same workgroup).
 * 0 restores the two-kernel path (k_admm, k_polish), whose stage times the timing entry points can then separate.
 * Results are identical.  May be changed at any time.
 */
int almpc_set_step_fusion(almpc_handle* h, int on);

/*
 * Redo of the instances a condensed step leaves without a certificate in the multiple-shooting form, by the stage-wise solvers of
 * ALMPC_FLAG_STRUCTURED, starting from the step's own result.  Which instances, exactly:
 *   - status ALMPC_MAX_ITER (1: an active-set finish that ran into its cap or out of room -- in practice per-instance linearisations
 *     that are open-loop unstable, and state-row instances at the edge of feasibility) go to the dual solver k_sdual (input box,
 *     state box, terminal equality, S);
 *   - with an input box only and S = 0 the primal solver k_riccati then takes everything that is still not ALMPC_SOLVED, i.e. also
 *     status ALMPC_NON_FINITE (2) instances whose condensed problem was flagged indefinite to working precision (a design flag, not
 *     a non-finite input: the stage-wise form does not form that Hessian).  With state rows or S such an instance keeps status 2.
 * Instances that were solved are not touched; an instance the finish has already found infeasible keeps its verdict
 * (ALMPC_INFEASIBLE); an undecided state-row instance that turns out infeasible comes back as ALMPC_INFEASIBLE.
 *   DEFAULT: ON wherever those solvers cover the design (shape limits of ALMPC_FLAG_STRUCTURED), for every design of a condensed
 *   handle: shared (incl. state rows, terminal equality, S), per instance, re-linearisation pipeline, SQP loop (the QP of an iteration
 *   in its stage-wise form for the instances whose condensed Hessian came out indefinite, instead of skipping them).
 *     - the SQP loop: the redo kernels are enqueued inside every iteration.
 *     - every other condensed design (shared model -- the headline path, tens of microseconds per step --, per-instance models,
 *       re-linearisation pipeline; input box or state rows): LAZILY -- the finish counts the instances it leaves with ALMPC_MAX_ITER
 *       into a host-visible word and the redo runs at the next point where the host looks at results through a synchronous call
 *       (almpc_calculate, almpc_synchronize, almpc_get_results, almpc_get_first_input, almpc_relin_fnn_step): no launch on the
 *       step path (two idle redo launches cost 14 us -- of a 61 us step on the headline path; with state rows a stage-wise solve
 *       of ONE edge-of-feasibility instance takes about a millisecond, and 1 - 12 instances in 4096 need one).  The redo takes x0
 *       from the step's own result (x[:, 1]), so handing over the next x0 before looking at the results is safe; references and
 *       models must still be the step's.  A caller that reads results only through the asynchronous tickets, or consumes them on
 *       the device (almpc_advance_plant / almpc_relin_fnn_advance loops), asks for the eager form with on = 1.
 *   on = 1: required (a design the stage-wise solvers cannot serve is an error) and always eager;  on = 0: off.
 * Call BEFORE the design.
 */
int almpc_set_structured_fallback(almpc_handle* h, int on);

/*
 * Start of the NEXT almpc_calculate(_async) of a structured handle `h` from the inputs of `src`'s last step (any handle on the
 * same device with the same n, m, batch and a horizon <= h's; enqueued on h's stream behind src's step, no host wait): the stages
 * `src` has start at its inputs, the ones beyond at the input reference.  Horizon continuation: the active bounds of an MPC problem
 * with the DARE terminal weight sit in the early stages, so the condensed path at a short horizon (tens of microseconds) hands the
 * stage-wise path at a long one its working set -- the quadrotor at N = 50 from N = 30: at most 4 working-set changes instead of up
 * to 123 from the clipped LQR start.  The optimum does not depend on the start.  A structured handle also honours opts.warm_start = 1:
 * the start is then its own previous inputs shifted by one stage (the receding-horizon shift, last stage repeated).
 */
int almpc_set_start_from(almpc_handle* h, almpc_handle* src);

/*
 * State box of the designs that have no xmin / xmax arguments of their own -- almpc_design_batched, almpc_design_ltv, the
 * re-linearisation pipeline: x_min <= x[:,k] <= x_max for stages 1..N+1, the rows kw `mpc_state_constraint` adds in every delegate
 * of the reference (src/sub/model_modeler_implementation/linear/mpc_modeler_implementation_linear.jl:62-70,
 * .../fnn/mpc_modeler_implementation_fnn.jl:146-153).  Takes effect at the next such design; NULL, NULL removes it.  Together with
 * almpc_set_terminal_equality these designs then build one constraint-space matrix per instance (k_ghat_inst) and the step's exact
 * finish is the dual active-set kernel of the shared-model state rows with per-instance operands.  Time-varying designs and the SQP
 * loop: the box is on xbar + dx, the terminal equality reads xbar + dx = x_ref at stage N+1; an SQP iteration whose QP is infeasible
 * is skipped for that instance (almpc_sqp_fnn_skipped) -- there is no elastic mode.  The SQP loop's stopping test and exact Hessian
 * need the multipliers of these rows: almpc_sqp_fnn_set_row_multipliers below.  Structured handles (ALMPC_FLAG_STRUCTURED) take the
 * same calls: there the rows are coordinates of the stage-wise trajectory (k_sdual), no constraint-space matrix is built.
 */
int almpc_set_state_box(almpc_handle* h, const double* xmin, const double* xmax);

int almpc_design_shared(almpc_handle* h, const double* A, const double* B, const double* Q,
                        const double* R, const double* S, const double* P, const double* umin,
                        const double* umax, const double* xmin, const double* xmax, double rho,
                        double sigma);

/*
 * Design with a model PER INSTANCE: A_batch [batch][n*n], B_batch [batch][n*m] (each block column-major).  This is the
 * linear-programming design of the reference applied to the linearisation of a black-box model at every instance's own
 * point (the reference linearises once, at the first reference, src/sub/model_modeler_implementation/fnn/
 * mpc_modeler_implementation_fnn.jl:38-46, and then builds the QP of ..linear.jl:48-100 from (A, B): given (A_i, B_i)
 * the QP of instance i is that QP; BASELINE.json configs[3] re-linearises every step, SURVEY.md section 8b
 * `almpc_design_batched`).  Q, R, S, umin, umax as in almpc_design_shared.  P: NULL -> DARE(A_i, B_i, Q, R) per instance
 * (src/sub/design_mpc.jl:327): by default one host solve per instance in a serial loop, 0.5 ms per 12-state instance -- seconds for
 * thousands of instances; after almpc_set_terminal_weight(h, ALMPC_TERMINAL_DARE_DEVICE) one kernel on the uploaded models (k_dare);
 * else one n*n matrix (P_per_instance = 0) or [batch][n*n] (P_per_instance = 1).
 * Prediction matrices, condensed Hessian (FP64 MFMA contraction), scaling and both inverses are built on the device for
 * every instance; the step then runs one workgroup per instance with the instance's KKT inverse in LDS.  State rows:
 * almpc_set_state_box / almpc_set_terminal_equality before the design.  Not available with per-instance models:
 * almpc_advance_plant.  A later
 * almpc_design_shared switches the handle back to the shared-model path.
 */
int almpc_design_batched(almpc_handle* h, const double* A_batch, const double* B_batch, const double* Q,
                         const double* R, const double* S, const double* P, int P_per_instance,
                         const double* umin, const double* umax, double rho, double sigma);

/*
 * The same with one weight set PER INSTANCE (a condensed handle): Q_batch [batch][n*n], R_batch [batch][m*m], S_batch [batch][m*m] or
 * NULL (S = 0 everywhere), each block column-major.  One plant with thousands of candidate tunings in one batch; and the design
 * that can take back the per-instance g_Q, g_R, g_S of almpc_sensitivity_params_vjp(_dare).  Everything else is almpc_design_batched:
 * layouts, P (NULL -> DARE(A_i, B_i, Q_i, R_i), host loop or k_dare after almpc_set_terminal_weight), almpc_set_model_time,
 * almpc_set_state_box / almpc_set_terminal_equality, almpc_set_rho_profile; every Q_i, R_i, S_i is symmetrised where almpc_design_batched
 * symmetrises its Q, R, S, so a batch of equal sets gives the bits of almpc_design_batched.  The step, almpc_sensitivity(_vjp) and
 * almpc_sensitivity_params_vjp(_dare) run on the design as they do on almpc_design_batched's; almpc_set_reference forms the
 * input-rate part of the gradient from each instance's S_i.
 * Branch rule: R[1,1] == 0 and S[1,1] == 0 (src/sub/design_mpc.jl:423-456) are one choice per design, so every instance must take the
 * same branch: a batch in which R_i[1,1] (or S_i[1,1]) is zero for some instances and not for others is ALMPC_ERR_INVALID, the lowest
 * instance that differs from instance 0 named in almpc_last_error.
 * The weights live in device buffers of the handle that only this call allocates.  A later almpc_design_batched or almpc_design_shared
 * puts the handle back on shared weights.
 * Not built (ALMPC_ERR_UNSUPPORTED, or as said):
 *  - ALMPC_FLAG_STRUCTURED handles: their solvers and screens (k_sgains, k_riccati, k_sdual, k_sens_face) take shared weights;
 *  - the stage-wise redo of a condensed handle, which runs the same kernels: after almpc_set_structured_fallback(h, 1) this call is
 *    refused; under the default ("auto") the redo counts as not covering the design, no redo launch follows a step, and an instance
 *    the finish leaves with ALMPC_MAX_ITER keeps that status;
 *  - per-instance input boxes: umin, umax are shared (the step kernels read the box);
 *  - the re-linearisation pipeline, almpc_design_ltv and the SQP loop keep shared weights: there is no weighted form of them.
 */
int almpc_design_batched_weighted(almpc_handle* h, const double* A_batch, const double* B_batch, const double* Q_batch /* [batch][n*n] */,
                                  const double* R_batch /* [batch][m*m] */, const double* S_batch /* [batch][m*m] or NULL */, const double* P,
                                  int P_per_instance, const double* umin, const double* umax, double rho, double sigma);
/* parity hook: the weights instance i is designed on, as the design kernels read them (symmetrised; S zeros where the design has none);
 * Q n*n, R m*m, S m*m column-major, any may be NULL.  On a design with shared weights (condensed almpc_design_shared / _batched) every
 * instance gets that set. */
int almpc_get_weights_instance(almpc_handle* h, int instance, double* Q, double* R, double* S);

/*
 * Design with TIME-VARYING models per instance: the QP of one SQP / multiple-shooting iteration around the trajectory
 * (xbar, ubar) of every instance (BASELINE.json configs[4]: SQP outer loop around the condensed-QP kernel; the reference has no
 * such path -- its NLP methods were removed, CHANGELOG.md:5 -- so only the QP itself has a reference meaning: with
 * A_k = A, B_k = B, c = 0 it is the QP of almpc_design_batched written in v = u - ubar).
 *   A_all [batch][N][n*n], B_all [batch][N][n*m]: Jacobians of x+ = f(x, u) at (xbar_k, ubar_k), k = 0..N-1 (column-major blocks);
 *   c_all [batch][N][n] or NULL: defects f(xbar_k, ubar_k) - xbar_{k+1};  xbar [batch][N+1][n] (xbar_0 = x0), ubar [batch][N][m];
 *   xref [N+1][n] / uref [N][m] or NULL (zeros): references of the tracking cost, shared;  Q, R, S, umin, umax as in
 *   almpc_design_shared;  P: terminal weight, n*n (P_per_instance = 0) or [batch][n*n] (required).
 * Linearised dynamics dx_{k+1} = A_k dx_k + B_k v_k + c_k, dx_0 = 0, cost of src/sub/design_mpc.jl:405-468 in (xbar + dx, ubar + v),
 * bounds umin <= ubar + v <= umax.  almpc_calculate then solves for v; almpc_get_results returns u = ubar + v and e_u = v
 * (x / e_x of almpc_get_results are not defined for an LTV design: the predicted states xbar + dx, the cost, the costates and a KKT
 * residual of the step come from almpc_certificate_ltv below, "Certificate of a step of a time-varying design").  almpc_set_reference is
 * not used with this design.  Needs nz^2 + 3 n nz + 4 n^2 + ... doubles <= 160 KB of LDS (nz <= ~120 for n = 12).
 */
int almpc_design_ltv(almpc_handle* h, const double* A_all, const double* B_all, const double* c_all, const double* xbar,
                     const double* ubar, const double* xref, const double* uref, const double* Q, const double* R,
                     const double* S, const double* P, int P_per_instance, const double* umin, const double* umax,
                     double rho, double sigma);

/* Gradient q (nz, unscaled, in v) of one instance's QP after almpc_design_ltv (parity hook; H: almpc_get_design_instance). */
int almpc_get_gradient_instance(almpc_handle* h, int instance, double* q);

/*
 * The same design on the STAGE-WISE solvers (ALMPC_FLAG_STRUCTURED handles only): nothing is condensed, so there is no m N <= 128
 * limit and an open-loop unstable linearisation over a long horizon is not lost.  The QP, the layouts, the branch rules (R[1,1] == 0,
 * S[1,1] == 0) and the meaning of every NULL are almpc_design_ltv's; there is no rho / sigma because no ADMM runs.
 * almpc_set_state_box and almpc_set_terminal_equality apply as on the SQP loop's stage-wise route: the box is on xbar + dx (stages
 * 1..N), the terminal equality is xbar_N + dx_N = xref_N.
 *   on_device = 0: A_all, B_all, c_all, xbar, ubar are host pointers (the call returns when they have been uploaded);
 *   on_device = 1: they are device memory of the handle's device (almpc_update_initialization_device's convention).  The handle keeps
 *     its own copies (device-to-device copies on its stream): the arrays must be complete before the call and may be overwritten
 *     after almpc_synchronize.  Weights, references, P and the bounds are host pointers in both forms.
 * almpc_design_ltv_stagewise does everything that happens once (buffers, weights, input box, state rows, the solvers' set-up) and
 * waits for it.  almpc_ltv_stagewise_update is the per-iteration call: new trajectory data into the same design -- no allocation, no
 * upload but the five arrays, and in the device form no host wait (copies and k_ltv_stage_prepare are enqueued).  It returns
 * ALMPC_ERR_NOT_DESIGNED before a stage-wise LTV design and ALMPC_ERR_INVALID when c_all is NULL and the design's was not, or the
 * other way round.  The host form of either call uploads into the handle's buffers and then runs what the device form runs.
 * almpc_calculate(_async): an input box alone with S = 0 goes to the primal Riccati active set (k_riccati_t) on the stage models,
 * everything else to k_sgains + k_sdual; the start is v = 0 (the guess is ubar); opts->warm_start is ignored (every call's data is a
 * new problem around a new trajectory), and so is almpc_update_initialization: the initial state is xbar_0 (dx_0 = 0).  ALL outputs of almpc_get_results are defined: u = ubar + v, e_u = v, x = xbar + dx (the
 * predicted states), e_x = dx -- both sums hold bit for bit --, status as on any structured handle (ALMPC_INFEASIBLE: proven).
 * almpc_certificate_ltv, almpc_sensitivity_ltv and _vjp serve such a design within their own limits (n <= 16, m <= 16,
 * (N + 1)(n + m) <= 1024; state rows as they refuse them); the stage models are always kept here (the solver reads them):
 * almpc_set_keep_stage_models is not needed.
 * Refused with ALMPC_ERR_UNSUPPORTED and the reason: a condensed handle (almpc_design_ltv is its call); continuous-time models; with
 * an input box alone and S = 0 a shape outside k_riccati; with state rows or S a shape outside k_sdual OR one that needs its
 * (32, 16) / (48, 16) builds, i.e. n (+ m with S) > 16 or m > 8 -- those two builds have no table of cached responses on a
 * per-instance design and are not launched without it.  The weights are shared: there is no
 * almpc_design_batched_weighted form.  almpc_set_reference afterwards is refused as after almpc_design_ltv.  No group form
 * (almpc_design_ltv has none either).
 */
int almpc_design_ltv_stagewise(almpc_handle* h, const double* A_all, const double* B_all, const double* c_all, const double* xbar,
                               const double* ubar, const double* xref, const double* uref, const double* Q, const double* R,
                               const double* S, const double* P, int P_per_instance, const double* umin, const double* umax,
                               int on_device);
int almpc_ltv_stagewise_update(almpc_handle* h, const double* A_all, const double* B_all, const double* c_all, const double* xbar,
                               const double* ubar, int on_device);
/* parity hook: what k_ltv_stage_prepare left for the current data -- ebar [batch][N][n] = xbar_{k+1} - xref_{k+1}, qadd [batch][N][m]
 * = 2 Rbar (ubar - uref) + 2 D'Sbar D ubar, eq_target [n] = xref_N (terminal equality only); any may be NULL.  Waits for the stream. */
int almpc_get_ltv_stagewise_prepared(almpc_handle* h, double* ebar, double* qadd, double* eq_target);

/*
 * SQP outer loop for a black-box Fnn model, resident on the device (BASELINE configs[4]).  The problem is the reference's
 * NonLinearProgramming branch for Fnn models (.../fnn/mpc_modeler_implementation_fnn.jl:73-189): the quadratic cost of
 * _create_quadratic_cost_function (src/sub/design_mpc.jl:405-468) subject to x[:,k+1] = fnn(x[:,k], u[:,k]) and the input box,
 * which the reference hands to Ipopt (src/sub/solver_selection.jl:100-104).  Here: Gauss-Newton SQP with multiple shooting and
 * steps of length `step_scale`; every iteration = k_fnn_jacobian along the trajectory, the time-varying condensed QP of
 * almpc_design_ltv, the per-instance step kernels, and the trajectory update -- all on the handle's stream, no host round trip.
 * A fixed point (step and defects zero) is a KKT point of the NLP: the QP gradient is the exact NLP gradient.
 * The first iteration after `start` finds its working-set guess by ADMM, the following ones take it from the iterate (inputs
 * that sit on a bound) and skip the ADMM phase and its KKT inverse; the exact finish makes the two equivalent.
 *
 *   setup    network in the layout of almpc_fnn_linearize (`activation`: a network code, ALMPC_NET_CODE), shared references xref n*(N+1) / uref m*N (NULL: zeros), weights,
 *            P (required; shared or per instance), input box, ADMM rho/sigma.  Replaces any earlier design of the handle.
 *   start    x0 [batch][n]; u_guess [batch][N][m] or NULL (the input reference); both clipped to the box.  The state
 *            trajectory starts as the network's own rollout from x0 (zero defects).
 *   iterate  `iters` iterations with QP options `opts` (NULL: defaults).  step_inf[it] / defect_inf[it] (nullable, length
 *            iters): max over the batch of |v|_inf and of |f(xbar,ubar) - xbar+|_inf BEFORE iteration it's update.
 *            Afterwards almpc_get_results returns the iterate: x, u, e_x = x - xref, e_u = u - uref, status/iters of the last QP.
 *            An instance whose condensed Hessian is not positive definite to working precision (open-loop unstable
 *            linearisation over a long horizon) or whose QP solution is non-finite keeps its last good iterate; the call then
 *            returns ALMPC_ERR_NUMERIC after finishing all other instances; almpc_sqp_fnn_skipped tells which.
 *            Shapes: setup checks the loop's own kernels (n <= 64, their LDS); the step behind every QP is the per-instance one of
 *            almpc_design_batched / almpc_design_ltv, whose finish rolls the stages out with n + m <= 8 g lanes, g the largest power
 *            of two with g n <= 64, and (N + 1)(n + m) <= 1024 -- n <= 16 in effect.  Beyond that the first iterate (as
 *            almpc_calculate on those designs) returns ALMPC_ERR_UNSUPPORTED; the stage-wise route (almpc_sqp_fnn_set_structured) has
 *            its own limits.
 */
int almpc_sqp_fnn_setup(almpc_handle* h, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                        const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                        const double* S, const double* P, int P_per_instance, const double* umin, const double* umax, double rho,
                        double sigma);
/* almpc_sqp_fnn_setup for a DenseNet (weight layout and `activation`: almpc_densenet_linearize); the other almpc_sqp_fnn_* calls
 * then run it */
int almpc_sqp_densenet_setup(almpc_handle* h, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                             const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                             const double* S, const double* P, int P_per_instance, const double* umin, const double* umax, double rho,
                             double sigma);
int almpc_sqp_fnn_start(almpc_handle* h, const double* x0, const double* u_guess);
int almpc_sqp_fnn_iterate(almpc_handle* h, int iters, double step_scale, const almpc_opts* opts, double* step_inf,
                          double* defect_inf);
int almpc_sqp_fnn_skipped(almpc_handle* h, int32_t* skipped /* [batch], 1 = some iteration was skipped */);
/*
 * Solve to a tolerance instead of a fixed count: at most max_iters (>= 1) iterations of the loop above (full steps under the handle's
 * step rule), with a first-order stopping test per instance at the top of every iteration, at its iterate:
 *     max_k |f(x_k, u_k) - x_{k+1}|_inf <= 1e-10  and  |U - clip(U - G / (2 R_aa))|_inf <= tol,
 * G the adjoint gradient of the cost at the iterate (with zero defects: the gradient of the single-shooting NLP).  An instance that
 * passes is frozen: no later iteration changes it (its results are bit-identical whatever max_iters is); the call returns when
 * every instance is frozen or max_iters iterations have run (then one last test at the final iterate).  Per instance (nullable):
 *     status  0 converged, 1 iteration limit, 2 an iteration was skipped (see iterate) and it did not converge, 3 the same with an
 *             infeasible QP (state rows)
 *     iters   QP iterations taken before the test that froze it (max_iters when it did not converge)
 *     kkt     the residual of its last test
 * Skipped iterations are reported in `status`, not as ALMPC_ERR_NUMERIC.  ALMPC_ERR_UNSUPPORTED when R[0,0] == 0 (the residual
 * divides by 2 R_aa) or m > 64.  almpc_get_results afterwards returns the iterate as after iterate.
 * State rows (almpc_set_state_box, almpc_set_terminal_equality): the test above knows nothing of their multipliers and never passes
 * at a solution with an active row -- switch almpc_sqp_fnn_set_row_multipliers on.  Then G is the gradient of the Lagrangian
 * (lam_N = 2 P e_N + mu_N, lam_k = 2 Q e_k + A_k' lam_{k+1} + mu_k) and the residual is the maximum of the projected residual above,
 * the complementarity |x - bound| over the box rows with mu != 0, the violation of the box, and |x_{N+1} - x_ref| under the terminal
 * equality.  An x0 outside the box is status 3 at the first iteration.
 */
/*
 * Hessian of every QP of the loop (iterate and solve): ALMPC_SQP_HESSIAN_GAUSS_NEWTON (default) or ALMPC_SQP_HESSIAN_EXACT, the
 * exact Lagrangian Hessian: the stage blocks W_k = d^2/dz^2 (lam_{k+1}' f(z_k)) with the multipliers of the adjoint walk at the
 * iterate, condensed into H and q, plus the Gershgorin bound of the result on the diagonal of every input on a bound at the iterate.
 * An instance whose shifted Hessian is still not positive definite takes that iteration with the Gauss-Newton QP (structured
 * fallback; without it the iteration is skipped).  State rows are linear and add no curvature, but their multipliers are part of lam:
 * EXACT with state rows needs almpc_sqp_fnn_set_row_multipliers switched on and the stage-wise fallback available (the Gauss-Newton QP
 * of an indefinite iteration then goes through k_sgains + k_sdual).  ALMPC_ERR_UNSUPPORTED for EXACT with state rows otherwise, the
 * structured QP route, relu, nz > 128, or a network whose per-wave scratch (n + m + 3 H + H (n + m) + S H (n + m + 2) doubles, S = L activation sites, 2 L for
 * a PolyNet) exceeds 16 KB (checked here once set up, else at the next iterate / solve).
 */
enum { ALMPC_SQP_HESSIAN_GAUSS_NEWTON = 0, ALMPC_SQP_HESSIAN_EXACT = 1 };
int almpc_sqp_fnn_set_hessian(almpc_handle* h, int mode);
int almpc_sqp_fnn_solve(almpc_handle* h, int max_iters, double tol, const almpc_opts* opts, int32_t* status, int32_t* iters,
                        double* kkt);
/*
 * Multipliers of the state rows.  With the switch on (default off; before or after setup, stays in force) whichever exact finish decides
 * an instance's QP of an iteration -- k_polish_gen / k_polish_gen64, or k_sdual behind them -- writes the multipliers of its state rows
 * out: mu [batch][N][n], entry (k, i) the row of x_{k+1}[i], k = 0..N-1; > 0 on an upper bound, < 0 on a lower bound, free on a
 * terminal-equality row, 0 outside the working set; in the units of the gradient of the cost (multiplier of the unscaled row).  An
 * instance whose iteration was void (step rule 1), skipped or frozen keeps those of its last solved QP; zero before the first.
 * almpc_sqp_fnn_solve and the exact Hessian then work with state rows (see there).  On a handle without state rows the switch
 * changes nothing and the read-back gives zeros; with it off every launch is what it was.  The condensed QP route only: with state rows on
 * the stage-wise route (almpc_sqp_fnn_set_structured, ALMPC_FLAG_STRUCTURED) iterate and solve return ALMPC_ERR_UNSUPPORTED while the switch is on.
 */
int almpc_sqp_fnn_set_row_multipliers(almpc_handle* h, int on);
int almpc_sqp_fnn_state_multipliers(almpc_handle* h, double* mu /* [batch][N][n], after iterate / solve */);
/* Step rule of almpc_sqp_fnn_iterate.  0 (default): every instance takes steps of length `step_scale` (full Gauss-Newton steps
 * are not globally convergent: they can end in a cycle when the tracking residual is large).  1: safeguarded by the l1 merit
 * function phi = J + mu |f(x,u) - x+|_1 (mu = 2 max(|P|, |Q|)), tested a posteriori with the network outputs the next
 * linearisation computes anyway: a step after which phi did not decrease is taken back and re-taken at half the length (that
 * iteration's QP is void for the instance), accepted steps double the factor back up to 1, and at 1/64 a step is accepted
 * regardless.  step_inf / defect_inf then cover the instances whose QP counted.  The factor restarts at 1 in `start`. */
int almpc_sqp_fnn_set_step_rule(almpc_handle* h, int rule);

/*
 * QP solver of the SQP loop (call before almpc_sqp_fnn_setup): 0 (default) the condensed path -- k_design_ltv, per-instance factors,
 * the step kernels --, 1 the stage-wise form for EVERY instance and iteration: k_sgains (Riccati recursion of the iteration's
 * unconstrained QP on (A_k, B_k, c_k)) + k_sdual, started from the iterate's own working set (v = 0).  No Hessian is formed or
 * inverted.  Same QP, same optimum (parity: oracle sqp_fnn(structured="dual")); takes the state box, the terminal equality and the
 * input-rate weight as the condensed route does.  Shape limits of ALMPC_FLAG_STRUCTURED.
 */
int almpc_sqp_fnn_set_structured(almpc_handle* h, int on);

/*
 * Per-step re-linearisation of a black-box Fnn model, resident on the device (BASELINE.json configs[3]).  The reference
 * linearises a black-box model ONCE, at the first reference (.../fnn/mpc_modeler_implementation_fnn.jl:38-46), and then runs the
 * linear path; this is the extension in which every instance is re-linearised at its own current state in every step: one call =
 * Jacobians A_i, B_i = d fnn / d(x, u) at (x0_i, u_ref[:,1]) written straight into the handle's per-instance model slots
 * (k_fnn_jacobian) -> the reference's QP for every (A_i, B_i) (the design kernels of almpc_design_batched) -> the step.  No host
 * pointer is touched: x0 comes from almpc_update_initialization(_device), results as after almpc_calculate.
 *   setup   network in the layout of almpc_fnn_linearize (`activation`: a network code, ALMPC_NET_CODE); xref n*(N+1), uref m*N shared (NULL: zeros); weights; P n*n (required:
 *           the reference takes the terminal weight from the linearisation at the LAST reference, src/sub/design_mpc.jl:312-327 --
 *           almpc_fnn_linearize + almpc_dare); input box; rho, sigma.  Replaces any earlier design of the handle.
 *   step    opts as almpc_calculate.  An instance whose condensed Hessian comes out without a positive diagonal / pivot (flagged by
 *           the design kernels) gets status ALMPC_NON_FINITE instead of a host-side error.
 *           opts->warm_start = 1 (after a solved step of this pipeline): the working-set guess is the previous step's input
 *           trajectory shifted by one stage instead of an ADMM phase, and the design needs one inverse per instance instead of two
 *           (the exact finish makes the two starts equivalent).
 *   advance x0 <- fnn(x0, u[:,1]) on the device: the closed loop of the black-box model itself, no host round trip.
 *   timing  (ALMPC_FLAG_TIMING) milliseconds of the last step's three stages.
 * On an ALMPC_FLAG_STRUCTURED handle (round 5; m N beyond the condensed limit -- the reference's delegation has no horizon limit,
 * .../fnn/mpc_modeler_implementation_fnn.jl:23-58) the same calls run the stage-wise route: Jacobians -> the Riccati recursion of
 * every instance's own unconstrained problem (k_sgains) -> the stage-wise dual active set (k_sdual) with the input box, the state box,
 * the terminal equality and S; rho / sigma are not used; opts->warm_start = 1 starts from the previous inputs shifted by one stage.
 * Shape limits of ALMPC_FLAG_STRUCTURED; an instance whose recursion meets a non-positive R + B'PB is left with ALMPC_MAX_ITER.
 */
int almpc_relin_fnn_setup(almpc_handle* h, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                          const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                          const double* S, const double* P, const double* umin, const double* umax, double rho, double sigma);
/* almpc_relin_fnn_setup for a DenseNet (weight layout and `activation`: almpc_densenet_linearize), condensed or structured handle;
 * the other almpc_relin_fnn_* calls then run it */
int almpc_relin_densenet_setup(almpc_handle* h, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                               const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                               const double* S, const double* P, const double* umin, const double* umax, double rho, double sigma);
int almpc_relin_fnn_step(almpc_handle* h, const almpc_opts* opts);
int almpc_relin_fnn_step_async(almpc_handle* h, const almpc_opts* opts);
int almpc_relin_fnn_advance(almpc_handle* h);
int almpc_relin_fnn_timing(almpc_handle* h, float* ms_jacobian, float* ms_design, float* ms_step);

/* H (nz*nz), F (nz*n), d (nz) of one instance after almpc_design_batched (any pointer may be NULL). */
int almpc_get_design_instance(almpc_handle* h, int instance, double* H, double* F, double* d);

/*
 * Where the terminal weight of a design with one model per instance comes from.
 */
#define ALMPC_TERMINAL_GIVEN        0   /* default: the caller's P, or the host DARE loop of almpc_design_batched(P = NULL) */
#define ALMPC_TERMINAL_DARE_DEVICE  1
/* Call BEFORE the design.  With ALMPC_TERMINAL_DARE_DEVICE:
 *  - almpc_design_batched(P = NULL), condensed or structured handle: the per-instance DARE runs on the device on the uploaded models
 *    (k_dare, no host loop).  A failing instance is the same error as on the host path (ALMPC_ERR_NUMERIC, "DARE did not converge for
 *    instance i", lowest i), so a structured handle keeps its stage-invariant records.
 *  - almpc_relin_fnn_* (every network kind, condensed and structured): every step solves DARE(A_i, B_i, Q, R) of the step's own
 *    Jacobians between the Jacobian launch and the design / k_sgains (the Jacobians of an Fnn are then computed by a launch of their
 *    own in front of the design, as those of the other kinds are: two launches more per Fnn step, one more otherwise).  The setup's P
 *    is still required: it is the terminal weight of any instance whose own DARE has no stabilising solution in that step (the loop
 *    goes on as it did before; the instance is reported by almpc_relin_fnn_terminal_status).  R[1,1] == 0 (the reference's branch rule
 *    drops R) leaves no DARE: the setup and almpc_design_batched(P = NULL) then return ALMPC_ERR_NUMERIC.
 *  n <= 48 and m <= 16 (k_dare); a design or setup beyond that returns ALMPC_ERR_UNSUPPORTED while the mode is on.
 *  No effect on almpc_design_shared, almpc_design_ltv, the SQP loop, or any design that is given a P.  Mode 0 and a new design or setup
 *  restore the default path. */
int almpc_set_terminal_weight(almpc_handle* h, int mode);
int almpc_relin_fnn_terminal_status(almpc_handle* h, int32_t* st /* [batch]: 0 own DARE, 1 the setup's P; last step */);
/* parity hook beside almpc_get_design_instance: the terminal weight instance i was designed with (n*n) */
int almpc_get_terminal_weight_instance(almpc_handle* h, int instance, double* P);

/*
 * Continuous-time models.  The reference accepts them (ConstrainedLinearControlContinuousSystem, src/sub/design_mpc.jl:22-41:
 * discretise, then the discrete method; the Discrete | Continuous union of the black-box method, :143-147).  Its
 * proceed_system_discretization lives outside the reference tree; this build's reading is the exact zero-order hold at the sample time,
 * [A_d B_d; 0 I] = exp([A_c B_c; 0 0] Ts) (almpc_c2d).
 */
#define ALMPC_MODEL_DISCRETE        0   /* default: every model is x+ = A x + B u */
#define ALMPC_MODEL_CONTINUOUS_ZOH  1
/* Call BEFORE the design.  With ALMPC_MODEL_CONTINUOUS_ZOH and a sample time Ts > 0:
 *  - almpc_design_shared: (A, B) is x' = A x + B u; it is discretised once on the host, then the design runs as it does today.  The
 *    handle holds the discrete model (almpc_advance_plant steps it).
 *  - almpc_design_batched, condensed or structured handle: the uploaded models are discretised in place by one kernel (k_c2d, one wave
 *    per instance) before anything reads them; with P = NULL the terminal weights are the DAREs of the DISCRETE models (k_dare behind
 *    k_c2d with ALMPC_TERMINAL_DARE_DEVICE, else hm::c2d + hm::dare per instance on the host).  An instance whose discretisation fails
 *    (a model that is not finite, |A_i| Ts beyond 2^59) is ALMPC_ERR_NUMERIC, "discretisation failed for instance i", lowest i.
 *  - almpc_relin_fnn_* (every network kind, condensed and structured): the network is read as x' = net(x, u).  Every step runs
 *    Jacobians -> k_c2d in place on the model slots -> (k_dare) -> design / k_sgains -> step; the Jacobians of an Fnn get a launch of
 *    their own (two launches more per Fnn step, one more otherwise).  The setup's P is a weight of the DISCRETE problem, as it is
 *    with the mode off.  An instance whose discretisation fails in a step leaves that step with ALMPC_NON_FINITE; the others are not
 *    affected.  almpc_relin_fnn_timing counts k_c2d in the design stage.
 *  - refused (ALMPC_ERR_UNSUPPORTED): almpc_relin_fnn_advance (the plant of a continuous-time network is an integrator, and that is
 *    the caller's), almpc_design_ltv, almpc_sqp_*_setup.
 *  n <= 64 and m <= 16 for the per-instance paths (k_c2d).  One sample time per handle.  Mode 0 and a new design or setup restore the
 *  default path; with the mode off every launch and allocation is what it was. */
int almpc_set_model_time(almpc_handle* h, int mode, double Ts);
/* parity hook: the DISCRETE model instance i is designed on (A n*n, B n*m, column-major; either may be NULL): the shared model, or
 * slot i of the per-instance models (after a re-linearisation step: that step's linearisation) */
int almpc_get_model_instance(almpc_handle* h, int instance, double* A, double* B);

/*
 * References (replaces _design_reference_mpc, src/main/main_mpc.jl:105-117, and the JuMP.fix of
 * x_reference/u_reference, ...linear.jl:90-100).  per_instance = 0: xref n*(N+1), uref m*N shared
 * by all instances.  per_instance = 1: xref [batch][N+1][n], uref [batch][N][m].
 * Default after design: all zeros.
 */
int almpc_set_reference(almpc_handle* h, const double* xref, const double* uref, int per_instance);

/* x0: host pointer, [batch][n].  Replaces update_initialization! (src/main/computation_mpc.jl:17-29). */
int almpc_update_initialization(almpc_handle* h, const double* x0);
/* same, x0 already in device memory of h's device (HBM-resident benchmark / closed loop on device) */
int almpc_update_initialization_device(almpc_handle* h, const double* d_x0);

/*
 * One MPC step for every instance: gradient f = F e0, ADMM, polish, rollout.  Replaces
 * JuMP.optimize! + the four JuMP.value reads of calculate! (src/main/computation_mpc.jl:41-53).
 * opts == NULL -> defaults.  opts->rho / opts->sigma must equal the design values (or be 0).
 * Synchronous: results are complete in device memory on return.
 */
int almpc_calculate(almpc_handle* h, const almpc_opts* opts);
/* enqueue only (no host sync); pair with almpc_synchronize */
int almpc_calculate_async(almpc_handle* h, const almpc_opts* opts);
int almpc_synchronize(almpc_handle* h);

/*
 * Closed loop without host round trips: x0 <- A x0 + B u[:,1] on the device, per instance, with the (A, B) of the design
 * and the first input of the last almpc_calculate (enqueued on the handle's stream; no host sync).  Follow with
 * almpc_calculate(_async) -- typically with opts.warm_start = 1 -- for the next receding-horizon step.
 */
int almpc_advance_plant(almpc_handle* h);

/*
 * Copy results to host.  Any pointer may be NULL.  Layouts: x, e_x [batch][N+1][n];
 * u, e_u [batch][N][m]  (ModelPredictiveControlResults, src/types/types.jl:134-139);
 * status, iters, polish_iters [batch].
 */
int almpc_get_results(almpc_handle* h, double* x, double* e_x, double* u, double* e_u,
                      int32_t* status, int32_t* iters, int32_t* polish_iters);

/*
 * Host-facing step path.  The reference's per-step contract is host in / host out (update_initialization!(C, x0),
 * src/main/computation_mpc.jl:17-29; calculate! leaves x, e_x, u, e_u in host matrices, src/main/computation_mpc.jl:50-53), and a
 * receding-horizon caller applies u[:,1] only.  These entry points move exactly what is asked for through pinned staging owned by
 * the handle, on copy streams of their own, so that the transfers of one step run under the kernel of the next:
 *   almpc_update_initialization_async   x0 [batch][n] (host): copied into a pinned slot of the handle, which the kernels of the next
 *                                       almpc_calculate(_async) read in place over the link (393 KB at the benchmark shape, requested
 *                                       under the operands every workgroup loads anyway): no HIP call, no device-side copy.  Returns
 *                                       at once; blocks only if both slots are still being read (two steps in flight).
 *   almpc_x0_staging                    zero-copy variant of the above: *x0_slot = the pinned host buffer ([batch][n]) that the NEXT
 *                                       almpc_update_initialization_async will use.  Write the states there (e.g. straight from the
 *                                       plant simulation) and pass the same pointer to almpc_update_initialization_async: the
 *                                       staging copy is skipped.  The pointer is valid until that call.
 *   almpc_get_results_async             asks for the results of the LAST enqueued step: `want` = mask of ALMPC_WANT_*.  The small
 *                                       ones (first inputs, status, iteration counts) are written by one pack kernel straight into
 *                                       the pinned slot, so the next step may start right behind it; x / e_x / u / e_u go out on a
 *                                       copy stream straight from the result buffers (the next step waits for that read-back).
 *                                       Returns a ticket >= 0 (or a negative almpc_status); the last 2 tickets are kept.
 *   almpc_get_results_wait              blocks until the ticket's read-back has landed, then copies the non-NULL arrays out of the
 *                                       pinned slot (layouts of almpc_get_results; u0 [batch][m] = u[:,1] of every instance).
 *   almpc_host_results                  zero-copy: pointers into the pinned slot of a ticket (NULL for arrays that were not asked
 *                                       for); valid after almpc_get_results_wait(h, ticket, NULL...) until 2 more requests.
 *   almpc_get_first_input               synchronous convenience: u0 [batch][m] of the last step (131 KB at the benchmark shape
 *                                       instead of the 32 MB of almpc_get_results).
 */
#define ALMPC_WANT_X 0x01u
#define ALMPC_WANT_E_X 0x02u
#define ALMPC_WANT_U 0x04u
#define ALMPC_WANT_E_U 0x08u
#define ALMPC_WANT_STATUS 0x10u
#define ALMPC_WANT_ITERS 0x20u
#define ALMPC_WANT_POLISH_ITERS 0x40u
#define ALMPC_WANT_FIRST_INPUT 0x80u
#define ALMPC_WANT_ALL 0xFFu
int almpc_update_initialization_async(almpc_handle* h, const double* x0);
int almpc_x0_staging(almpc_handle* h, double** x0_slot);
int almpc_get_results_async(almpc_handle* h, uint32_t want);
int almpc_get_results_wait(almpc_handle* h, int ticket, double* x, double* e_x, double* u, double* e_u, double* u0,
                           int32_t* status, int32_t* iters, int32_t* polish_iters);
int almpc_host_results(almpc_handle* h, int ticket, const double** x, const double** e_x, const double** u, const double** e_u,
                       const double** u0, const int32_t** status, const int32_t** iters, const int32_t** polish_iters);
int almpc_get_first_input(almpc_handle* h, double* u0);

/*
 * One process, several GPUs (almpc_create(..., n_devices, device_ids, ...); the reference API is one
 * process, one call: proceed_controller, src/main/main_mpc.jl:22-53).  A group is one handle per entry of device_ids (a device may
 * appear more than once), handle i on the contiguous shard [first_i, first_i + count_i) of the batch (sizes differ by at most
 * one); instances never interact, so a group call fans out over the handles and nothing on the step path synchronises across
 * devices: almpc_group_calculate_async enqueues on every device before almpc_group_synchronize waits for any.  Host arrays are
 * those of the single-handle calls with `batch` = the whole batch; per-instance arrays (models, terminal weights, guesses) are cut
 * along the shards.  Everything a handle can do has a group form: the options that are set before a design (almpc_group_set_*), the
 * shared and per-instance designs, the re-linearisation pipeline, the SQP loop, the host-facing read-back (tickets, zero-copy x0
 * slots); the synchronous design entry points run on one host thread per device, so that all devices design at the same time.
 * flags (ALMPC_FLAG_TIMING, ALMPC_FLAG_STRUCTURED) go to every handle; almpc_group_handle(g, i) reaches one handle directly.
 */
typedef struct almpc_group almpc_group;
int almpc_group_create(almpc_group** out, int n, int m, int N, int batch, int n_devices, const int* device_ids, uint32_t flags);
void almpc_group_destroy(almpc_group* g);
const char* almpc_group_last_error(const almpc_group* g);
int almpc_group_size(const almpc_group* g);
almpc_handle* almpc_group_handle(almpc_group* g, int i);
int almpc_group_shard(const almpc_group* g, int i, int* first, int* count);
int almpc_group_design_shared(almpc_group* g, const double* A, const double* B, const double* Q, const double* R, const double* S,
                              const double* P, const double* umin, const double* umax, const double* xmin, const double* xmax,
                              double rho, double sigma);
int almpc_group_set_reference(almpc_group* g, const double* xref, const double* uref, int per_instance);
int almpc_group_update_initialization(almpc_group* g, const double* x0);
int almpc_group_calculate(almpc_group* g, const almpc_opts* opts);
int almpc_group_calculate_async(almpc_group* g, const almpc_opts* opts);
int almpc_group_synchronize(almpc_group* g);
int almpc_group_get_results(almpc_group* g, double* x, double* e_x, double* u, double* e_u, double* u0, int32_t* status,
                            int32_t* iters, int32_t* polish_iters);
/* options of every handle (each takes effect at the next design, as the single-handle call says) */
int almpc_group_set_terminal_equality(almpc_group* g, int on);
int almpc_group_set_rho_profile(almpc_group* g, int mode);
int almpc_group_set_structured_fallback(almpc_group* g, int on);
int almpc_group_set_state_box(almpc_group* g, const double* xmin, const double* xmax);
int almpc_group_set_terminal_weight(almpc_group* g, int mode);
int almpc_group_set_model_time(almpc_group* g, int mode, double Ts);
/* almpc_design_batched: A_batch [batch][n*n], B_batch [batch][n*m], P NULL | n*n | [batch][n*n] (P_per_instance = 1) */
int almpc_group_design_batched(almpc_group* g, const double* A_batch, const double* B_batch, const double* Q, const double* R,
                               const double* S, const double* P, int P_per_instance, const double* umin, const double* umax, double rho,
                               double sigma);
/* almpc_design_batched_weighted: Q_batch [batch][n*n], R_batch, S_batch (or NULL) [batch][m*m] cut along the shards as well; the branch
 * rule holds for the whole batch */
int almpc_group_design_batched_weighted(almpc_group* g, const double* A_batch, const double* B_batch, const double* Q_batch,
                                        const double* R_batch, const double* S_batch, const double* P, int P_per_instance,
                                        const double* umin, const double* umax, double rho, double sigma);
/* almpc_relin_fnn_* (BASELINE configs[3]): the same network and references on every device; step_async + almpc_group_synchronize */
int almpc_group_relin_fnn_setup(almpc_group* g, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                                const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                                const double* S, const double* P, const double* umin, const double* umax, double rho, double sigma);
int almpc_group_relin_densenet_setup(almpc_group* g, int H, int L, int activation, const double* W_in, const double* W_h,
                                     const double* b_h, const double* W_out, const double* xref, const double* uref, const double* Q,
                                     const double* R, const double* S, const double* P, const double* umin, const double* umax, double rho,
                                     double sigma);
int almpc_group_relin_fnn_step(almpc_group* g, const almpc_opts* opts);
int almpc_group_relin_fnn_step_async(almpc_group* g, const almpc_opts* opts);
int almpc_group_relin_fnn_advance(almpc_group* g);
int almpc_group_advance_plant(almpc_group* g);
/* almpc_sqp_fnn_* (BASELINE configs[4]): x0 [batch][n], u_guess [batch][N][m] or NULL, P n*n or [batch][n*n]; iterate runs the devices'
 * loops at the same time, step_inf / defect_inf are maxima over the whole batch; skipped [batch] */
int almpc_group_sqp_fnn_set_structured(almpc_group* g, int on);
int almpc_group_sqp_fnn_set_step_rule(almpc_group* g, int rule);
int almpc_group_sqp_fnn_setup(almpc_group* g, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                              const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                              const double* S, const double* P, int P_per_instance, const double* umin, const double* umax, double rho,
                              double sigma);
int almpc_group_sqp_densenet_setup(almpc_group* g, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                                   const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                                   const double* S, const double* P, int P_per_instance, const double* umin, const double* umax,
                                   double rho, double sigma);
int almpc_group_sqp_fnn_start(almpc_group* g, const double* x0, const double* u_guess);
int almpc_group_sqp_fnn_iterate(almpc_group* g, int iters, double step_scale, const almpc_opts* opts, double* step_inf,
                                double* defect_inf);
int almpc_group_sqp_fnn_skipped(almpc_group* g, int32_t* skipped);
int almpc_group_sqp_fnn_set_hessian(almpc_group* g, int mode);
int almpc_group_sqp_fnn_set_row_multipliers(almpc_group* g, int on);
int almpc_group_sqp_fnn_state_multipliers(almpc_group* g, double* mu /* [batch][N][n] */);
/* almpc_sqp_fnn_solve on every device at the same time; status / iters / kkt [batch] (nullable) */
int almpc_group_sqp_fnn_solve(almpc_group* g, int max_iters, double tol, const almpc_opts* opts, int32_t* status, int32_t* iters,
                              double* kkt);
/* host-facing path of the group: slots[i] = handle i's pinned x0 buffer ([count_i][n], almpc_x0_staging) -> write the shard's states
 * there -> almpc_group_update_initialization_staged(g, slots) (no copy);  read-back by ticket as almpc_get_results_async / _wait, the
 * arrays of _wait being those of almpc_group_get_results */
int almpc_group_x0_staging(almpc_group* g, double** slots /* [almpc_group_size(g)] */);
int almpc_group_update_initialization_staged(almpc_group* g, double* const* slots);
int almpc_group_get_results_async(almpc_group* g, uint32_t want);
int almpc_group_get_results_wait(almpc_group* g, int ticket, double* x, double* e_x, double* u, double* e_u, double* u0, int32_t* status,
                                 int32_t* iters, int32_t* polish_iters);
/* almpc_sensitivity / almpc_get_sensitivity / almpc_sensitivity_vjp of the whole batch: arrays as there with `batch` = the whole batch */
int almpc_group_sensitivity(almpc_group* g, uint32_t want, double act_tol);
int almpc_group_get_sensitivity(almpc_group* g, double* K0, double* dU, double* dX, int32_t* rows);
int almpc_group_sensitivity_vjp(almpc_group* g, const double* g_u, const double* g_x, double act_tol, double* g_x0, int32_t* rows);
int almpc_group_sensitivity_rows(almpc_group* g, uint32_t want, double act_tol_u, double act_tol_x);
int almpc_group_sensitivity_rows_vjp(almpc_group* g, const double* g_u, const double* g_x, double act_tol_u, double act_tol_x,
                                     double* g_x0, int32_t* rows);

/* Design data for parity tests: H nz*nz, F nz*n (both unscaled, column-major), P n*n, d nz. */
int almpc_get_design(almpc_handle* h, double* H, double* F, double* P, double* d);

/*
 * Device pointers of the handle's result buffers (same layouts as almpc_get_results), for callers
 * that keep the loop on the GPU.  Valid until almpc_destroy.
 */
int almpc_device_results(almpc_handle* h, const double** d_x, const double** d_e_x,
                         const double** d_u, const double** d_e_u);

/*
 * Sensitivities of the returned solution to the measured state x0, per instance, after a step (k_sens, DESIGN.md "k_sens"; an
 * extension: the reference hands out x, e_x, u, e_u only, src/main/computation_mpc.jl:50-53).  W = the rows of the returned u at a
 * bound: row (stage k, input i) is in W iff u[i,k] - umin_i <= act_tol * d_j or umax_i - u[i,k] <= act_tol * d_j, d_j the row's Jacobi
 * scale (almpc_get_design); act_tol <= 0 means 1e-9.  The test is on the returned u, not on the finish's internal working set.  With
 * G = H'^-1, V = -G F', S = G[W,W]:  du/dx0 = diag(d) (V - G[:,W] S^-1 V[W,:]) (rows W are zero), dx[:,1]/dx0 = I,
 * dx[:,k+1]/dx0 = A dx[:,k]/dx0 + B du[:,k]/dx0.  Where no multiplier of W is zero this is the derivative of the solution map; at a
 * weakly active row (multiplier zero) the map is only directionally differentiable, and what is returned is the derivative of the face
 * on which EVERY row at its bound is held.
 *   almpc_sensitivity          a synchronous look at the LAST step: does what almpc_synchronize does first (the lazy redo included, so
 *                              redone instances take part), then computes what `want` (a mask of ALMPC_SENS_*) names into device buffers
 *                              of the handle, which exist from the first such call on (ALMPC_SENS_DX also computes dU).
 *   almpc_get_sensitivity      copies them out (NULL = not wanted; asking for one that was not computed, or after a newer step:
 *                              ALMPC_ERR_INVALID); rows [batch] = |W| of every instance.
 *   almpc_device_sensitivity   the device pointers (NULL for what was not computed); valid until the next almpc_sensitivity.
 *   almpc_sensitivity_vjp      for a loss L(x, u) with gradients g_u [batch][N][m] and g_x [batch][N+1][n] (NULL: zeros, bit-identical
 *                              to passing zeros) on the returned trajectories: g_x0 [batch][n] = dL/dx0, without forming a Jacobian
 *                              (adjoint rollout, one solve with S); host pointers, synchronous like almpc_sensitivity.
 * An instance whose status is not ALMPC_SOLVED (or whose S is not positive definite to working precision) gets rows = -1 and zeros.
 * ALMPC_ERR_INVALID before the design's first step.  Served: almpc_design_shared and almpc_design_batched with an input box (shared or
 * per-instance references, S != 0).  ALMPC_ERR_UNSUPPORTED, with the reason in almpc_last_error: state rows (state box, terminal
 * equality; see the rows form below), ALMPC_FLAG_STRUCTURED handles, almpc_design_ltv, the SQP loop and the re-linearisation pipeline.
 *
 * Rows form: almpc_sensitivity_rows / almpc_sensitivity_rows_vjp also serve almpc_design_shared with a state box and / or the terminal
 * equality (shared or per-instance references, S != 0, instances redone by the stage-wise fallback).  W then ranges over the rows of
 * A = [I; C']: input rows by the rule above with act_tol_u; a state-box row (stage k >= 2, state i) is in W iff
 *     x[i,k] - xmin_i <= act_tol_x * max(1, |xmin_i|)   or   xmax_i - x[i,k] <= act_tol_x * max(1, |xmax_i|)
 * on the returned x (act_tol_x <= 0 means 1e-7: a factor 100 above the 1e-9 the returned state rows keep to their bounds; a bound that
 * is not finite or at least 1e300 in size is never active); every terminal-equality row is in W.  A state row's bound moves with x0,
 * so with Ghat = A G A' and T1 = A V + [0; Phi_rows]:  S = Ghat[W,W],  du/dx0 = diag(d) (T1[0:nz] - Ghat[0:nz,W] S^-1 T1[W]) (input
 * rows of W are zero), dX by the same rollout -- with an input box alone the formula above.  As there, at a weakly active row what
 * comes out is the derivative of the face on which every flagged row is held.  rows [batch] = |W| over input, state and equality
 * rows; -1 and zeros for an instance that is not ALMPC_SOLVED or whose S is not positive definite (a working set of more than nz
 * rows among them).  Results go to the same buffers: almpc_get_sensitivity and almpc_device_sensitivity serve them.  On a design
 * without state rows the rows form takes the path of almpc_sensitivity / almpc_sensitivity_vjp with act_tol = act_tol_u: the same
 * bits.  Still ALMPC_ERR_UNSUPPORTED: per-instance models (almpc_design_batched) with state rows, and what is refused above.
 */
#define ALMPC_SENS_K0 0x1u   /* [batch][n][m]        du[:,1]/dx0, column-major m x n per instance       */
#define ALMPC_SENS_DU 0x2u   /* [batch][n][N][m]     Julia Array{Float64,4}(m, N, n, batch)             */
#define ALMPC_SENS_DX 0x4u   /* [batch][n][N+1][n]                                                      */
int almpc_sensitivity(almpc_handle* h, uint32_t want, double act_tol);
int almpc_get_sensitivity(almpc_handle* h, double* K0, double* dU, double* dX, int32_t* rows);      /* NULL = not wanted */
int almpc_device_sensitivity(almpc_handle* h, const double** d_K0, const double** d_dU, const double** d_dX, const int32_t** d_rows);
int almpc_sensitivity_vjp(almpc_handle* h, const double* g_u, const double* g_x /* or NULL */, double act_tol,
                          double* g_x0 /* [batch][n] */, int32_t* rows /* or NULL */);
int almpc_sensitivity_rows(almpc_handle* h, uint32_t want, double act_tol_u, double act_tol_x);
int almpc_sensitivity_rows_vjp(almpc_handle* h, const double* g_u, const double* g_x /* or NULL */, double act_tol_u, double act_tol_x,
                               double* g_x0 /* [batch][n] */, int32_t* rows /* or NULL */);

/*
 * The same on ALMPC_FLAG_STRUCTURED handles (k_sens_face, DESIGN.md "k_sens_face"), which form no G = H'^-1 and need none: on the face
 * where the rows W are held the problem is an LQ problem whose clamped inputs are taken out stage by stage, and its derivative is a
 * Riccati recursion with a masked B -- O(N (n^3 + n^2 m)) per instance, whatever m N and the spectral radius of A.  Input box only,
 * S = 0.  Stages 0-based: x_0 = x0, Qbar_k = Q (1 <= k <= N-1), Qbar_0 = 0, P on stage N; W_k the inputs of stage k in W, f the free:
 *     P+ = P at k = N;  for k = N-1 .. 0:
 *       Lam = R_ff + B_f' P+ B_f                 (R as the design uses it: zero when R[1,1] == 0)
 *       K_k[f,:] = Lam^-1 B_f' P+ A,   K_k[W_k,:] = 0,   Acl_k = A - B K_k
 *       P+ <- Qbar_k + Acl_k' P+ Acl_k + K_k' R K_k            (symmetrised)
 *     Jacobians:  dx_0 = I,  du_k = -K_k dx_k,  dx_{k+1} = A dx_k + B du_k          (K0 = -K_0)
 *     VJP:        lam_N = g_x[N],  lam_k = g_x[k] - K_k' g_u[k] + Acl_k' lam_{k+1},   g_x0 = lam_0
 * W, on the returned u (a structured handle has no Jacobi scale): row (stage k, input i) is in W iff
 *     u[i,k] - umin_i <= act_tol * w_i   or   umax_i - u[i,k] <= act_tol * w_i,     w_i = umax_i - umin_i;
 * act_tol <= 0 means 1e-7: k_riccati writes a working-set row out as the bound itself, but k_sdual's confirmation accepts a
 * working-set row up to 1e-8 of its width away from its bound (csrc/almpc_sdual.hip.h:1012, `resn <= 1e-8`), and the default is ten
 * times that.  At a weakly active row: the derivative of the face on which every flagged row is held, as above.
 *   almpc_sensitivity_stagewise      almpc_sensitivity: synchronous, settles first, results in the same buffers of the handle, so
 *                                    almpc_get_sensitivity and almpc_device_sensitivity serve them; layouts and rows as there.  A call
 *                                    for ALMPC_SENS_K0 alone is one backward sweep and allocates no gain scratch.
 *   almpc_sensitivity_stagewise_vjp  almpc_sensitivity_vjp: the adjoint rides the backward sweep, no gain is stored, no Jacobian formed;
 *                                    g_x = NULL is bit-identical to zeros.
 * An instance that is not ALMPC_SOLVED, or one of whose Lam has a pivot that is not positive and finite, gets rows = -1 and zeros.
 * Served: almpc_design_shared and almpc_design_batched on a structured handle (A_i, B_i, P_i per instance).  ALMPC_ERR_UNSUPPORTED,
 * with the reason in almpc_last_error: a handle that is not structured (almpc_sensitivity serves it), S != 0 in the design, a state box
 * or the terminal equality, the SQP loop and the re-linearisation pipeline, a shape outside k_riccati (n <= 32, m <= 16, m N <= 1024).
 * ALMPC_ERR_INVALID: before the design's first step, a `want` that is no mask of ALMPC_SENS_*, a NULL g_u or g_x0.
 */
int almpc_sensitivity_stagewise(almpc_handle* h, uint32_t want, double act_tol);            /* ALMPC_SENS_K0 | _DU | _DX */
int almpc_sensitivity_stagewise_vjp(almpc_handle* h, const double* g_u, const double* g_x /* or NULL */, double act_tol,
                                    double* g_x0 /* [batch][n] */, int32_t* rows /* or NULL */);
int almpc_group_sensitivity_stagewise(almpc_group* g, uint32_t want, double act_tol);
int almpc_group_sensitivity_stagewise_vjp(almpc_group* g, const double* g_u, const double* g_x, double act_tol, double* g_x0, int32_t* rows);

/*
 * The same with the input-rate weight S (k_sens_face_rate, DESIGN.md "k_sens_face_rate"): every structured input-box design, with or
 * without S.  The cost carries sum_k (u_k - u_{k+1})' S (u_k - u_{k+1}), k = 0 .. N-2, so a stage sees the input before it and the
 * recursion runs in the stage state z_k = [dx_k; du_{k-1}], nt = n + m.  R as the design uses it; S_k = S (symmetrised) for k >= 1 and
 * S_0 = 0, because nothing ties u_0 to an input applied before the horizon:
 *     At = [A 0; 0 0] (nt x nt)    Bt = [B; I] (nt x m)    Nt_k = [0; -S_k] (nt x m)    Rt_k = R + S_k
 *     Qt_k = blkdiag(Qbar_k, S_k),  Qbar_k = Q (1 <= k <= N-1),  Qbar_0 = 0
 *     Pi+ = blkdiag(sym(P), 0) at k = N;  for k = N-1 .. 0:
 *       Lam = (Rt_k + Bt' Pi+ Bt)_ff
 *       K_k[f,:] = Lam^-1 (Bt' Pi+ At + Nt_k')_f,   K_k[W_k,:] = 0   (m x nt),   Acl_k = At - Bt K_k
 *       Pi+ <- Qt_k + K_k' Rt_k K_k - Nt_k K_k - K_k' Nt_k' + Acl_k' Pi+ Acl_k            (symmetrised)
 *     Jacobians:  dz_0 = [I_n; 0],  du_k = -K_k dz_k,  dz_{k+1} = At dz_k + Bt du_k = [A dx_k + B du_k; du_k]      (K0 = -K_0[:, :n])
 *     VJP:        lam_N = [g_x[N]; 0],  lam_k = [g_x[k]; 0] - K_k' g_u[k] + Acl_k' lam_{k+1},   g_x0 = lam_0[:n]
 * Everything else is the pair above: synchronous, settles first, results in the handle's buffers (almpc_get_sensitivity and
 * almpc_device_sensitivity serve them), the same layouts, the same rule for W with act_tol <= 0 meaning 1e-7, g_x = NULL bit-identical
 * to zeros, rows = -1 and zeros for an instance that is not ALMPC_SOLVED or has a pivot that is not positive and finite, no gain
 * scratch for ALMPC_SENS_K0 alone (with dU or dX the scratch is [batch][N][m nt]).
 * On a design without the rate term (S == NULL, S[1,1] == 0 or R[1,1] == 0) the calls take the path of almpc_sensitivity_stagewise /
 * almpc_sensitivity_stagewise_vjp and k_sens_face: the same bits.  Those two calls themselves go on refusing a design with S.
 * Served: almpc_design_shared and almpc_design_batched on a structured handle (S is shared by the batch on both), in the shapes the
 * structured solve serves with S: n <= 32, m <= 16, n + m <= 48, (N + 1)(n + m) <= 4096, m N <= 1024.  ALMPC_ERR_UNSUPPORTED, with the
 * reason in almpc_last_error: a handle that is not structured, a state box or the terminal equality, time-varying and SQP designs and
 * the re-linearisation pipeline, a design without the primal solver's weights, a stage that does not fit LDS.  ALMPC_ERR_INVALID:
 * before the design's first step, a `want` that is no mask of ALMPC_SENS_*, a NULL g_u or g_x0.
 */
int almpc_sensitivity_stagewise_rate(almpc_handle* h, uint32_t want, double act_tol);       /* ALMPC_SENS_K0 | _DU | _DX */
int almpc_sensitivity_stagewise_rate_vjp(almpc_handle* h, const double* g_u, const double* g_x /* or NULL */, double act_tol,
                                         double* g_x0 /* [batch][n] */, int32_t* rows /* or NULL */);
int almpc_group_sensitivity_stagewise_rate(almpc_group* g, uint32_t want, double act_tol);
int almpc_group_sensitivity_stagewise_rate_vjp(almpc_group* g, const double* g_u, const double* g_x, double act_tol, double* g_x0, int32_t* rows);

/*
 * Certificate of the last step (k_cert, DESIGN.md "k_cert"): the objective value, the costates, the gradient of the objective in the
 * inputs and a KKT residual, from the returned trajectories and the design data alone -- no solver internals, so the same kernel and
 * the same numbers serve condensed, per-instance, weighted and structured handles, and an instance is certified whatever its status
 * (an ALMPC_MAX_ITER instance gets the residual of the inputs it returned).  Per instance, stages 0-based, e_k = e_x[:,k],
 * v_k = e_u[:,k], u_k = u[:,k]; Q, R, S, P symmetrised; useR = R[1,1] != 0 and useS = useR && S[1,1] != 0 as the design took them
 * (src/sub/design_mpc.jl:436-465):
 *     cost    J     = e_N'P e_N + sum_{k<N} (e_k'Q e_k + [useR] v_k'R v_k) + [useS] sum_{i<N-1} (u_i - u_{i+1})'S (u_i - u_{i+1})
 *                     (the reference's objective: the constant e_0'Q e_0 included)
 *     costate lam_N = 2 P e_N,  lam_k = 2 Q e_k + A'lam_{k+1};   lam_0 = dJ/dx0 at fixed inputs, = dJ* / dx0 at an optimum
 *     grad    g_k   = B'lam_{k+1} + [useR] 2 R v_k + [useS]([k < N-1] 2 S (u_k - u_{k+1}) - [k > 0] 2 S (u_{k-1} - u_k))
 *                     (stacked: H v + f of the condensed QP; no H is formed)
 *     res           = max_{k,j} |u_k - clip(u_k - g_k, umin, umax)|       (0 at an optimum; the oracle's kkt_residual in unscaled u coordinates)
 * res is as large as |g| at an input inside the box: it measures how far the GRADIENT is from the normal cone of the box, not how far u
 * is from the optimum.  With stiff weights the two differ by many orders (quadrotor, Q = 100 I, N = 30: inputs within 5e-12 of the exact
 * optimum have res up to 1e-2, entries of H being up to 1e9), so judge res against the size of g (res <= 1e-9 max(1, |g|_inf), say).
 * The multipliers of the input box are -g at the inputs that sit at a bound (positive at umax); that mask is the caller's.
 *   almpc_certificate         synchronous, settles first (a lazily redone instance is certified on its redone result); `want` is a mask
 *                             of ALMPC_CERT_*; the results stay in buffers of the handle until the next step or design.
 *   almpc_get_certificate     copies out what the last almpc_certificate computed (NULL: not wanted; a pointer whose bit was not
 *                             asked for is ALMPC_ERR_INVALID).  Layouts: cost, res [batch]; grad [batch][N][m]; costate [batch][N+1][n].
 *   almpc_device_certificate  the device addresses of the same buffers (NULL for a bit that was not computed).
 * Served: almpc_design_shared, almpc_design_batched and almpc_design_batched_weighted on condensed handles, almpc_design_shared and
 * almpc_design_batched on ALMPC_FLAG_STRUCTURED handles; n <= 64, m <= 16 (a structured handle exists only for n <= 32, m <= 16,
 * m N <= 1024 -- almpc_create --, and the kernel reads the weights its designs leave for the primal stage-wise solver).
 * ALMPC_ERR_NOT_DESIGNED before a design;
 * ALMPC_ERR_INVALID before the design's first step, for want = 0 or unknown bits, and from the getters after a new step or design;
 * ALMPC_ERR_UNSUPPORTED, with the reason in almpc_last_error: almpc_design_ltv, the SQP loop and the re-linearisation pipeline (their QP
 * has a defect term and a trajectory of its own), and on designs with a state box or the terminal equality every bit but
 * ALMPC_CERT_COST (the state-row multipliers enter the costates, and the trajectory alone does not determine them).
 */
#define ALMPC_CERT_COST 1u
#define ALMPC_CERT_RES 2u
#define ALMPC_CERT_GRAD 4u
#define ALMPC_CERT_COSTATE 8u
int almpc_certificate(almpc_handle* h, uint32_t want);
int almpc_get_certificate(almpc_handle* h, double* cost /*[batch]*/, double* res /*[batch]*/, double* grad /*[batch][N][m]*/,
                          double* costate /*[batch][N+1][n]*/);   /* NULL = not wanted */
int almpc_device_certificate(almpc_handle* h, const double** d_cost, const double** d_res, const double** d_grad, const double** d_costate);
int almpc_group_certificate(almpc_group* g, uint32_t want);
int almpc_group_get_certificate(almpc_group* g, double* cost, double* res, double* grad, double* costate);

/*
 * Certificate of a step of a time-varying design (k_cert_ltv, DESIGN.md "k_cert_ltv"): what an SQP / multiple-shooting caller of
 * almpc_design_ltv needs to close its outer loop on the device -- the predicted states to take the step with, the cost for a merit
 * function, the costates (the multipliers of the linearised dynamics: an exact Lagrangian Hessian W_k = d2(lam_{k+1}'f)/dz2 is built from
 * them) and a method-independent KKT residual as a stopping test.  From the returned u and e_u = v and the design data alone.  Per
 * instance, stages 0-based, v_k = e_u[:,k], u_k = u[:,k], w_k = u_k - uref_k, d_i = u_i - u_{i+1}; Q, R, S, P symmetrised; useR, useS as
 * the design took them:
 *     forward   dx_0 = 0,  dx_{k+1} = A_k dx_k + B_k v_k + c_k          (c = 0 if the design got NULL)
 *               x_k = xbar_k + dx_k,  e_k = x_k - xref_k
 *     cost      J = e_N'P e_N + sum_{k<N} (e_k'Q e_k + [useR] w_k'R w_k) + [useS] sum_{i<N-1} d_i'S d_i
 *     backward  lam_N = 2 P e_N,  lam_k = 2 Q e_k + A_k'lam_{k+1}
 *               g_k = B_k'lam_{k+1} + [useR] 2 R w_k + [useS]([k < N-1] 2 S d_k - [k > 0] 2 S d_{k-1})
 *     res       max_{k,j} |u_k - clip(u_k - g_k, umin, umax)|
 * With H, q of the design's QP min 1/2 v'Hv + q'v (almpc_get_design_instance, almpc_get_gradient_instance): stacked g = H v + q;
 * J(v) - J(0) = 1/2 v'Hv + q'v; lam_{k+1} = dJ/dc_k at fixed v.  res is to be judged against max(1, |g|_inf), as almpc_certificate's.
 *   almpc_set_keep_stage_models  on != 0: the NEXT almpc_design_ltv moves its copies of A_all, B_all, c_all into the handle instead of
 *                             releasing them behind the design kernels, and uploads the shared xref / uref (xbar, ubar are on the device
 *                             already).  Costs batch N n (n + m + 1) doubles of device memory until the next almpc_design_ltv or
 *                             almpc_destroy.  Default 0: the design is exactly what it was.
 *   almpc_certificate_ltv     synchronous, settles first; `want` is a mask of ALMPC_CERT_* and ALMPC_CERT_STATES; the results stay in
 *                             buffers of the handle (cost, res, grad, costate: those of almpc_certificate) until the next step or design.
 *   almpc_get_certificate_ltv copies out what the last almpc_certificate_ltv computed (NULL: not wanted; a pointer whose bit was not
 *                             asked for is ALMPC_ERR_INVALID; x and e_x both belong to ALMPC_CERT_STATES).
 *   almpc_device_certificate_ltv  the device addresses of the same buffers (NULL for a bit that was not computed).
 * Shapes: those a step of an LTV design runs at -- n <= 16, m <= 16, (N + 1)(n + m) <= 1024 (else ALMPC_ERR_UNSUPPORTED).
 * ALMPC_ERR_NOT_DESIGNED before a design; ALMPC_ERR_INVALID before the design's first step, for want = 0 or unknown bits, from the
 * getters after a new step or design, and after an almpc_design_ltv made with the keep switch off (the message names the switch);
 * ALMPC_ERR_UNSUPPORTED on a design that is not almpc_design_ltv's (the message names almpc_certificate; the SQP loop stays without a
 * certificate: its Jacobians belong to the iterate before the update), and with a state box or the terminal equality for every bit but
 * ALMPC_CERT_COST and ALMPC_CERT_STATES.  almpc_certificate keeps refusing these designs.
 *
 * The re-linearisation pipeline is a per-instance time-invariant design (e_x[:,k+1] = A_i e_x[:,k] + B_i e_u[:,k]), so k_cert serves it:
 *   almpc_relin_fnn_certificate  almpc_certificate's four quantities for the last almpc_relin_fnn_step, with the models (A_i, B_i), the
 *                             terminal weights (one per step after almpc_set_terminal_weight) and the weights that step used; condensed
 *                             and structured handles; with state rows ALMPC_CERT_COST alone.  Fills almpc_certificate's buffers: read
 *                             them with almpc_get_certificate, almpc_device_certificate, almpc_group_get_certificate.  Error codes as
 *                             almpc_certificate's; ALMPC_ERR_UNSUPPORTED on a design that is not the pipeline's.
 */
#define ALMPC_CERT_STATES 16u
int almpc_set_keep_stage_models(almpc_handle* h, int on);
int almpc_certificate_ltv(almpc_handle* h, uint32_t want);            /* ALMPC_CERT_* | ALMPC_CERT_STATES */
int almpc_get_certificate_ltv(almpc_handle* h, double* cost, double* res, double* grad, double* costate,
                              double* x /*[batch][N+1][n]*/, double* e_x /*[batch][N+1][n]*/);
int almpc_device_certificate_ltv(almpc_handle* h, const double** d_cost, const double** d_res, const double** d_grad,
                                 const double** d_costate, const double** d_x, const double** d_ex);
int almpc_relin_fnn_certificate(almpc_handle* h, uint32_t want);      /* k_cert on the step's own (A_i, B_i, P_i) */
int almpc_group_relin_fnn_certificate(almpc_group* g, uint32_t want);

/*
 * Sensitivities of a step of a time-varying design in its initial deviation (k_sens_ltv, DESIGN.md "k_sens_ltv"): what a real-time-
 * iteration caller of almpc_design_ltv needs when the measured state arrives after the QP was prepared around xbar_0 -- the control
 * to apply is clip(u_0 + K0 (x_meas - xbar_0)) -- and what a learning loop around an LTV step backpropagates through.  Let p perturb
 * the initial deviation: the design's QP with dx_0 = p in place of dx_0 = 0, everything else as almpc_design_ltv states it.  All
 * derivatives are taken at p = 0, on the face W of the returned u.  The linearisation trajectory, the defects c_k and the references
 * do not enter (the face problem is linear in p); the derivative of the linearisation itself belongs to the caller's outer loop.
 * Stages 0-based, A_k, B_k the design's stage models, R, S, useR, useS as the design took them (R = 0 without useR), P symmetrised
 * (per instance where the design got one per instance), W_k the inputs of stage k in W, f the free ones.
 * Without the rate term (useS == 0), the recursion of almpc_sensitivity_stagewise with one model per stage:
 *     P+ = sym(P) at k = N;  for k = N-1 .. 0:
 *       Lam = R_ff + B_k,f' P+ B_k,f
 *       K_k[f,:] = Lam^-1 B_k,f' P+ A_k,   K_k[W_k,:] = 0,   Acl_k = A_k - B_k K_k
 *       P+ <- Qbar_k + Acl_k' P+ Acl_k + K_k' R K_k      (symmetrised; Qbar_k = Q for 1 <= k <= N-1; P_0 has no reader)
 *     Jacobians:  dx_0 = I,  du_k = -K_k dx_k,  dx_{k+1} = A_k dx_k + B_k du_k          (K0 = -K_0)
 *     VJP:        lam_N = g_x[N],  lam_k = g_x[k] - K_k' g_u[k] + Acl_k' lam_{k+1},   g_x0 = lam_0
 * With it (useS != 0): the recursion of almpc_sensitivity_stagewise_rate above, unchanged, in the stage state [dx_k; du_{k-1}] with
 * At_k = [A_k 0; 0 0], Bt_k = [B_k; I] and S_0 = 0.
 * dX is the derivative of the predicted states x_k = xbar_k + dx_k of ALMPC_CERT_STATES, g_x a loss gradient on those states.
 * W, on the returned u: row (stage k, input i) is in W iff
 *     u[i,k] - umin_i <= act_tol * w_i   or   umax_i - u[i,k] <= act_tol * w_i,     w_i = umax_i - umin_i;
 * act_tol <= 0 means 1e-7.  At a weakly active row: the derivative of the face on which every flagged row is held.
 *   almpc_sensitivity_ltv      synchronous, settles first; results in the handle's sensitivity buffers in the layouts of
 *                              almpc_sensitivity, so almpc_get_sensitivity and almpc_device_sensitivity serve them until the next step
 *                              or design.  ALMPC_SENS_K0 alone is one backward sweep and allocates no gain scratch; with dU or dX
 *                              the gains of every stage go to a scratch [batch][N][m w], w = n or n + m.
 *   almpc_sensitivity_ltv_vjp  the adjoint rides the backward sweep, no gain is stored, no Jacobian formed; g_x = NULL is bit-identical
 *                              to zeros.
 * An instance that is not ALMPC_SOLVED, or one of whose Lam has a pivot that is not positive and finite, gets rows = -1 and zeros in
 * every output asked for.  Gradients in c_k, in the stage models or in the weights are not formed.  There is no group form, because
 * almpc_design_ltv has none.
 * Shapes: those a step of an LTV design runs at -- n <= 16, m <= 16, (N + 1)(n + m) <= 1024 (else ALMPC_ERR_UNSUPPORTED).
 * ALMPC_ERR_NOT_DESIGNED before a design; ALMPC_ERR_INVALID before the design's first step, for a `want` that is no mask of
 * ALMPC_SENS_*, for a NULL g_u or g_x0, and after an almpc_design_ltv made with the keep switch off (the message names
 * almpc_set_keep_stage_models); ALMPC_ERR_UNSUPPORTED, with the reason in almpc_last_error, on a design that is not almpc_design_ltv's
 * (the message names the call that serves it; the SQP loop stays refused: its Jacobians belong to the iterate before the update) and
 * with a state box or the terminal equality.  almpc_sensitivity and its rows and stage-wise forms keep refusing these designs, with a
 * message that names almpc_sensitivity_ltv.
 */
int almpc_sensitivity_ltv(almpc_handle* h, uint32_t want, double act_tol);          /* ALMPC_SENS_K0 | _DU | _DX */
int almpc_sensitivity_ltv_vjp(almpc_handle* h, const double* g_u, const double* g_x /* or NULL */, double act_tol,
                              double* g_x0 /* [batch][n] */, int32_t* rows /* or NULL */);

/*
 * Parameter gradients of the returned solution: for the loss of almpc_sensitivity_vjp (g_u [batch][N][m], g_x [batch][N+1][n] or NULL),
 * its gradient in the problem data, per instance, on the face where the rows W (same rule, same act_tol) are held -- the backward
 * pass of a step for a caller who learns or tunes the controller (k_sens_pz, k_sens_params; DESIGN.md "k_sens_params").  Stages
 * 1-based, v = e_u, sym(a, b) = a b' + b a', Qbar_1 = 0, Qbar_k = Q (k = 2..N), Qbar_{N+1} = P:
 *     lam_{N+1} = g_x[N+1],  lam_k = A'lam_{k+1} + g_x[k],   q_k = g_u[:,k] + B'lam_{k+1}
 *     z_W = 0,  z_F = -H_FF^-1 q_F;   nu_j = q_j + (H z)_j on the rows of W, 0 elsewhere
 *     zeta_1 = 0,  zeta_{k+1} = A zeta_k + B z_k
 *     mu_{N+1} = g_x[N+1] + 2 P zeta_{N+1},  mu_k = A'mu_{k+1} + g_x[k] + 2 Qbar_k zeta_k
 *     al_{N+1} = 2 P e_x[:,N+1],             al_k = A'al_{k+1} + 2 Qbar_k e_x[:,k]
 *     x0    = mu_1 (= lam_1 + F'z: the bits of almpc_sensitivity_vjp's g_x0)      f = z  (the gradient in the QP's linear term)
 *     Q     = sum_{k=2..N} sym(zeta_k, e_x[:,k])        P = sym(zeta_{N+1}, e_x[:,N+1])        R = sum_{k=1..N} sym(z_k, v_k)
 *     S     = sum_{k=1..N-1} sym(z_k - z_{k+1}, u_k - u_{k+1})                    (the rate cost is on u, not on e_u)
 *     A     = sum_{k=1..N} mu_{k+1} e_x[:,k]' + al_{k+1} zeta_k'                  B = sum_{k=1..N} mu_{k+1} v_k' + al_{k+1} z_k'
 *     u_ref[:,k] = g_u[:,k] - nu_k + 2 S (z_k - z_{k+1}) - 2 S (z_{k-1} - z_k)    (S terms only where S is in the design)
 *     u_min_i = sum_k nu_(k,i) over the rows at the lower bound, u_max_i over those at the upper (a row at both counts as lower)
 * Conventions: the gradient of a symmetric matrix (Q, P, R, S) is the symmetric matrix G with dL = sum_ij G_ij dM_ij for symmetric dM.
 * P is data in this call, also where the design computed it as a DARE; almpc_sensitivity_params_vjp_dare (below) follows its dependence
 * on A, B, Q, R.  Where the design dropped R
 * or S (R[1,1] == 0; S[1,1] == 0: src/sub/design_mpc.jl:423-456) that gradient is zero.  x_ref needs no output:
 * dL/dx_ref[:,1] = g_x[1] - x0, dL/dx_ref[:,k] = g_x[k] for k >= 2.  At a weakly active row: the derivative of the face on which every
 * flagged row is held, as above.  Outputs are per instance also where the design is shared (the caller sums over the batch), and for
 * almpc_design_batched, whose Q, R, S and box are shared by the instances; almpc_design_batched_weighted is the design that takes
 * g_Q, g_R, g_S back instance by instance (each instance's own Q_i, S_i, R_i enter its adjoint).
 * The call is synchronous and settles first like almpc_sensitivity_vjp; only the groups whose pointer is not NULL are computed and
 * copied (without u_ref, Q, P, A, R, S, B the second kernel is not launched).  Refusals are almpc_sensitivity_vjp's: ALMPC_ERR_UNSUPPORTED
 * for state rows, ALMPC_FLAG_STRUCTURED handles, almpc_design_ltv, the SQP loop and the re-linearisation pipeline; ALMPC_ERR_INVALID
 * before the design's first step, for a NULL g_u or out, and for an out whose pointers are all NULL.  An instance that is not
 * ALMPC_SOLVED (or whose S is not positive definite) gets rows = -1 and zeros in every output.
 */
typedef struct almpc_param_grads {      /* host pointers, NULL = not wanted; per instance, batch slowest */
    double *x0;              /* [batch][n]                         */
    double *f;               /* [batch][N][m]                      */
    double *u_ref;           /* [batch][N][m]                      */
    double *u_min, *u_max;   /* [batch][m]                         */
    double *Q, *P, *A;       /* [batch][n*n] column-major          */
    double *R, *S;           /* [batch][m*m]                       */
    double *B;               /* [batch][n*m] column-major n x m    */
    int32_t *rows;           /* [batch] |W|, or -1                 */
} almpc_param_grads;
int almpc_sensitivity_params_vjp(almpc_handle* h, const double* g_u, const double* g_x /* or NULL */, double act_tol,
                                 const almpc_param_grads* out);
/* ... of the whole batch of a group: every array with `batch` = the whole batch, cut along the shards */
int almpc_group_sensitivity_params_vjp(almpc_group* g, const double* g_u, const double* g_x /* or NULL */, double act_tol,
                                       const almpc_param_grads* out);

/*
 * The same with the terminal weight followed: P_i = DARE(A_i, B_i, Q, R) is a function of the model and the weights (the reference has
 * no other P: src/sub/design_mpc.jl:318-327), so Q, R, A, B also gain what the loss gains through P.  With the P group gP of the call
 * above (computed internally when out->P is NULL) one launch of k_dare_vjp (almpc_dare_vjp_batched below, DESIGN.md "k_dare_vjp") adds
 *     Q += X,   R += K X K',   A += 2 P Acl X,   B += -2 P Acl X K'        X = Acl X Acl' + gP,  Acl = A - B K,  K = (R + B'PB)^-1 B'PA
 * per instance, from the design's own A_i, B_i, P_i, Q, R.  out->P is still the gradient in P as data; x0, f, u_ref, u_min, u_max, S,
 * P and rows are bit for bit those of almpc_sensitivity_params_vjp, and so are its refusals and the -1 and zeros of an unsolved
 * instance (dare_status 0).  No flag records where P came from: the kernel tests it.  dare_status[i] = 0: followed; 1: R + B'PB is
 * singular; 2: the closed loop A - B K is not stable (P solves the equation but is not the stabilising solution); 3: P does not solve
 * the equation of the design's model (a P the caller gave that is no DARE solution).  An instance with a non-zero status keeps the
 * P-as-data values in Q, R, A, B bit for bit and the call returns ALMPC_OK; with dare_status == NULL such an instance makes the call
 * ALMPC_ERR_NUMERIC (almpc_last_error names the lowest one) and nothing is copied out.  ALMPC_ERR_UNSUPPORTED: a design that dropped
 * R (R[1,1] == 0: no DARE), n > 48 or m > 16.  Not followed anywhere else: the re-linearisation pipeline, almpc_design_ltv and the
 * SQP loop, and designs with state rows are refused as above.
 */
int almpc_sensitivity_params_vjp_dare(almpc_handle* h, const double* g_u, const double* g_x /* or NULL */, double act_tol,
                                      const almpc_param_grads* out, int32_t* dare_status /* [batch] or NULL */);
int almpc_group_sensitivity_params_vjp_dare(almpc_group* g, const double* g_u, const double* g_x /* or NULL */, double act_tol,
                                            const almpc_param_grads* out, int32_t* dare_status /* [batch] or NULL */);

/*
 * Timing of the last almpc_calculate (needs ALMPC_FLAG_TIMING): milliseconds spent in the ADMM
 * kernel, the polish kernel(s), the rollout kernel, and the whole enqueue->done span, measured
 * with HIP events on the handle's stream.
 */
int almpc_get_timing(almpc_handle* h, float* ms_admm, float* ms_polish, float* ms_rollout,
                     float* ms_total);
/*
 * Timing over many steps: with ALMPC_FLAG_TIMING every almpc_calculate records its own set of events.
 * almpc_timing_reset forgets the recorded steps (and pre-creates events for `reserve_steps` steps so that
 * no event is created inside a timed region); almpc_timing_summary synchronises and returns the number of
 * steps recorded since the reset and the SUM of their per-stage milliseconds.
 */
int almpc_timing_reset(almpc_handle* h, int reserve_steps);
/* Record the events only on every `every`-th almpc_calculate (default 1).  One step's four event records cost ~14 us of
 * stream time on MI355X, so a throughput run samples (bench.py: every 16th step) instead of timing every step. */
int almpc_timing_set_stride(almpc_handle* h, int every);
int almpc_timing_summary(almpc_handle* h, int* steps, double* ms_admm, double* ms_polish,
                         double* ms_rollout, double* ms_total);
/* The individual samples behind almpc_timing_summary: per recorded step its four stage times (arrays of `cap` floats, any may be
 * NULL; the first min(cap, *count) entries are filled); *count = steps recorded since the reset.  Synchronises the stream. */
int almpc_timing_samples(almpc_handle* h, int cap, int* count, float* ms_admm, float* ms_polish, float* ms_rollout,
                         float* ms_total);

/*
 * Discrete algebraic Riccati solution P of  A'PA - P - A'PB (R + B'PB)^-1 B'PA + Q = 0  (host, n x n): what
 * ControlSystems.are(Discrete, A, B, Q, R) returns at src/sub/design_mpc.jl:327.  Exposed because a black-box model takes
 * its terminal weight from the linearisation at the LAST reference while its dynamics come from the FIRST
 * (src/sub/design_mpc.jl:312-327 vs .../fnn/mpc_modeler_implementation_fnn.jl:38-46): pass the result as P to the design.
 */
int almpc_dare(int n, int m, const double* A, const double* B, const double* Q, const double* R, double* P);

/* P_i = DARE(A_i, B_i, Q, R) for a batch of models on device `device_id` (the style of almpc_fnn_linearize: no handle; host pointers,
 * synchronous): A_batch [batch][n*n], B_batch [batch][n*m], shared Q (n*n) and R (m*m), all column-major; the algorithm of almpc_dare,
 * one wave per instance (k_dare).
 * status[i] = 0, or non-zero: no stabilising solution to working precision (P_batch slot i is left untouched).
 * Returns ALMPC_OK even when some instances fail; ALMPC_ERR_NO_DEVICE without a gfx950 device (no CPU path);
 * ALMPC_ERR_NUMERIC when R is singular; ALMPC_ERR_UNSUPPORTED beyond n <= 48, m <= 16. */
int almpc_dare_batched(int device_id, int n, int m, int batch, const double* A_batch, const double* B_batch,
                       const double* Q, const double* R, double* P_batch, int32_t* status);

/*
 * The adjoint of almpc_dare (host math): for P = DARE(A, B, Q, R) and a symmetric g_P = dL/dP (n*n), what the loss gains through P in
 * the four arguments.  Sm = R + B'PB, K = Sm^-1 B'PA, Acl = A - B K, X = Acl X Acl' + g_P (discrete Lyapunov equation, by doubling):
 *     g_Q = X,   g_R = K X K',   g_A = 2 P Acl X,   g_B = -2 P Acl X K'
 * g_Q and g_R are symmetric (the convention of almpc_param_grads).  Outputs may be NULL.  ALMPC_ERR_NUMERIC, nothing written, with
 * the status in almpc_last_error(NULL) (the calling thread's last such failure, handed out once): 1 R + B'PB is singular; 2 the closed
 * loop is not stable to working precision (64 doublings), P is not the stabilising solution; 3 the residual of the equation exceeds
 * almpc_dare's acceptance bound 1e-7 max(1, max|P|, max|Q|), P is no solution for this model.
 */
int almpc_dare_vjp(int n, int m, const double* A, const double* B, const double* Q, const double* R,
                   const double* P, const double* g_P, double* g_A, double* g_B, double* g_Q, double* g_R);

/* The same for a batch on device `device_id` (the style of almpc_dare_batched: no handle; host pointers, synchronous; the same layouts):
 * P_batch, gP_batch, gA_batch, gQ_batch [batch][n*n], gB_batch [batch][n*m], gR_batch [batch][m*m]; the outputs may be NULL; one wave per
 * instance (k_dare_vjp).  status[i] = 0, or 1 / 2 / 3 as above (the output slots i are left untouched).  What the handle calls cannot
 * serve: a black-box design takes P from the linearisation at the LAST reference and its dynamics from the FIRST, so its caller chains
 * out->P of almpc_sensitivity_params_vjp through this call on the last-reference Jacobians.
 * Returns ALMPC_OK even when some instances fail; ALMPC_ERR_NO_DEVICE without a gfx950 device (no CPU path);
 * ALMPC_ERR_NUMERIC when R is singular; ALMPC_ERR_UNSUPPORTED beyond n <= 48, m <= 16. */
int almpc_dare_vjp_batched(int device_id, int n, int m, int batch, const double* A_batch, const double* B_batch,
                           const double* Q, const double* R, const double* P_batch, const double* gP_batch,
                           double* gA_batch, double* gB_batch, double* gQ_batch, double* gR_batch, int32_t* status);

/* Exact zero-order hold of x' = Ac x + Bc u at the sample time Ts (host math, like almpc_dare): [Ad Bd; 0 I] = exp([Ac Bc; 0 0] Ts) by
 * scaling and squaring on the pair (Ad, Bd) -- no augmented matrix, no linear solve, so a singular Ac is no special case (the double
 * integrator gives [[1, 1], [0, 1]] and [0.5, 1] exactly).  Ac n*n, Bc n*m, column-major.  ALMPC_ERR_INVALID: Ts <= 0 or not finite;
 * ALMPC_ERR_NUMERIC: a model that is not finite, or |Ac|_1 Ts beyond 2^59; Ad, Bd are then untouched. */
int almpc_c2d(int n, int m, const double* Ac, const double* Bc, double Ts, double* Ad, double* Bd);

/* The same for a batch of models on device `device_id` (the style of almpc_dare_batched: no handle; host pointers, synchronous; the same
 * layouts): one wave per instance (k_c2d), n <= 64, m <= 16 (beyond: ALMPC_ERR_UNSUPPORTED).
 * status[i] = 0, or non-zero: the discretisation failed (slots i of Ad_batch and Bd_batch are left untouched).
 * Returns ALMPC_OK even when some instances fail; ALMPC_ERR_NO_DEVICE without a gfx950 device (no CPU path, nothing is written). */
int almpc_c2d_batched(int device_id, int n, int m, int batch, const double* Ac_batch, const double* Bc_batch, double Ts,
                      double* Ad_batch, double* Bd_batch, int32_t* status /* [batch] */);

/*
 * Network code: the `activation` argument of almpc_fnn_linearize, almpc_relin_fnn_setup, almpc_sqp_fnn_setup and their
 * almpc_group_* forms is ALMPC_NET_CODE(kind, activation).  The kinds share the weight layout below and differ in the hidden layer
 * (a = W_h[l] y + b_h[l]):
 *     ALMPC_NET_FNN      y' = act(a)                                   (.../fnn/mpc_modeler_implementation_fnn.jl:131-140)
 *     ALMPC_NET_RESNET   y' = y + act(a)                               (.../resnet/mpc_modeler_implementation_resnet.jl:131-140)
 *     ALMPC_NET_POLYNET  p = act(a), y' = y + p + act(W_h[l] p + b_h[l]), the same weights twice
 *                                                                      (.../polynet/mpc_modeler_implementation_polynet.jl:132-148)
 * A bare activation 0..4 is ALMPC_NET_CODE(ALMPC_NET_FNN, activation): the codes of old keep their meaning.  An Icnn is an Fnn.
 * An unknown kind or activation: ALMPC_ERR_UNSUPPORTED.
 */
#define ALMPC_NET_FNN 0
#define ALMPC_NET_RESNET 1
#define ALMPC_NET_POLYNET 2
#define ALMPC_NET_CODE(kind, act) (((kind) << 8) | (act))

/*
 * Batched linearisation of a black-box Fnn model on the GPU: for each of `batch` points (x_i, u_i) the Jacobians
 * A_i = df/dx (n x n), B_i = df/du (n x m), both column-major, and optionally f_i = f(x_i, u_i).  Stands in for
 * AutomationLabsSystems.proceed_system_linearization (.../fnn/mpc_modeler_implementation_fnn.jl:42-46).  Layout as the
 * reference reads it from Flux.params (.../fnn/...:88-107): W_in H x (n+m) without bias or activation, L hidden layers
 * (W_h[l] H x H, b_h[l] H) with `activation` (0 identity, 1 relu, 2 tanh, 3 sigmoid, 4 swish; the
 * reference takes whatever NNlib function sits at f[2][1].sigma, src/sub/design_mpc.jl:472-483), W_out n x H without bias; all column-major.
 * `activation` is a network code (ALMPC_NET_CODE above): ResNet and PolyNet models in the same layout.  Host pointers; synchronous.
 */
int almpc_fnn_linearize(int device_id, int n, int m, int H, int L, int activation, const double* W_in,
                        const double* W_h, const double* b_h, const double* W_out, int batch, const double* x,
                        const double* u, double* A, double* B, double* f);

/*
 * DenseNet (.../densenet/mpc_modeler_implementation_densenet.jl:85-161): its layer widths grow, so it has its own weight layout and
 * its own setup calls (almpc_densenet_linearize, almpc_relin_densenet_setup, almpc_sqp_densenet_setup and their almpc_group_*
 * forms) instead of a network code; `activation` is a bare code 0..4 (anything else: ALMPC_ERR_UNSUPPORTED).  With z = [x; u]:
 *     y_1 = W_in z,   y_{l+2} = [act(W_h[l] y_{l+1} + b_h[l]); y_{l+1}]  (l = 0..L-1: the new features first),   x+ = W_out y_{L+1}
 * so y_{l+1} has (l+1) H rows.  Column-major:
 *     W_in   H x (n+m)
 *     W_h    L blocks; block l is H x (l+1) H at offset H^2 l (l+1) / 2; its column c multiplies entry c of y_{l+1} (newest first)
 *     b_h    [L][H]
 *     W_out  n x (L+1) H
 * After setup the handle runs every other call of its family as for an Fnn.  Exact-Hessian mode has the per-wave scratch budget
 * of almpc_sqp_fnn_set_hessian (y, its adjoint and d y / d z have (L+1) H rows).
 */
int almpc_densenet_linearize(int device_id, int n, int m, int H, int L, int activation, const double* W_in,
                             const double* W_h, const double* b_h, const double* W_out, int batch, const double* x,
                             const double* u, double* A, double* B, double* f);

/*
 * Multi-GPU: one process per GPU, each with its own handle on its contiguous shard of the batch; instances never interact, so no
 * collective is on the data path of a step.  RCCL (over xGMI) runs inside the library (dlopen("librccl.so") at first use) for what a
 * multi-GPU caller needs between steps:
 *   almpc_comm_unique_id   rank 0 makes the 128-byte id and hands it to the other ranks by any channel (file, socket, MPI, ...)
 *   almpc_comm_init        every rank, collectively: ncclCommInitRank on the handle's device
 *   almpc_comm_summary     out4 = {ranks in the job, instances with status != 0 over all ranks (sums); max ADMM iterations, max
 *                          polish iterations over all ranks (max)} of the last step; collective; synchronises the handle's stream
 *   almpc_comm_allgather_first_input   u[:,1] of every instance of every rank: [world][batch][m] doubles (32 B per quadrotor instance,
 *                          never the full trajectories); u0_all: host buffer or NULL; d_u0_all: receives the device pointer or NULL;
 *                          collective, on the handle's stream (synchronous only when u0_all is given)
 * ALMPC_ERR_UNSUPPORTED: librccl could not be loaded.
 */
#define ALMPC_COMM_ID_BYTES 128
int almpc_comm_unique_id(char* id128);
int almpc_comm_init(almpc_handle* h, const char* id128, int rank, int world);
int almpc_comm_summary(almpc_handle* h, int64_t* out4);
int almpc_comm_allgather_first_input(almpc_handle* h, double* u0_all, const double** d_u0_all);

/*
 * Test hook: overwrite the LDS of every compute unit with NaN bit patterns (a kernel that reads LDS it has not written
 * then produces NaNs instead of passing on stale values).  Synchronous.  Not needed by callers.
 */
int almpc_debug_poison_lds(almpc_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* ALMPC_H */
