// almpc_api.hip -- C ABI of libalmpc.so (declared in include/almpc.h) over the gfx950 kernels.
//
// Host side of the drop-in boundary.  Reference entry points this replaces (relative to
// /root/reference): _model_predictive_control_design src/sub/design_mpc.jl:54-129 (-> almpc_design_shared),
// update_initialization! src/main/computation_mpc.jl:17-29, calculate! src/main/computation_mpc.jl:38-55.
// No torch, no BLAS, no CPU solve path: every per-step computation runs in almpc_kernels.hip.h.
#include "almpc_kernels.hip.h"
#include "almpc_design.hip.h"
#include "almpc_polish_gen.hip.h"
#include "almpc_fnn.hip.h"
#include "almpc_instance.hip.h"
#include "almpc_sqp.hip.h"
#include "almpc_comm.hip.h"
#include "almpc_riccati.hip.h"
#include "almpc_sdual.hip.h"
#include "almpc_dare.hip.h"
#include "almpc_dare_vjp.hip.h"
#include "almpc_c2d.hip.h"
#include "almpc_sens.hip.h"
#include "almpc_sens_ltv.hip.h"
#include "almpc_cert.hip.h"
#include "almpc_cert_ltv.hip.h"
#include "almpc_ltv_stage.hip.h"
#include "almpc_host_math.h"
#include "almpc_switches.h"
#include "almpc_devbuf.h"
#include "../../include/almpc.h"

// The heavy kernel templates are compiled by their own translation units (almpc_tu_*.hip, one per kernel family, built in parallel);
// here their instantiations are only DECLARED.  The lists are generated from a unity build (tools/gen_instances.py); an instantiation
// that is missing from them is simply compiled here, as everything is with -DALMPC_UNITY (one translation unit: the diagnostic
// -DALMPC_STAMPS build, whose stamp buffer is a device variable of ONE code object).
#ifndef ALMPC_UNITY
#define ALMPC_KERNEL_INSTANCE(...) extern template __global__ __VA_ARGS__;
#include "instances/sdual_a.inc"
#include "instances/sdual_b.inc"
#include "instances/sdual_c.inc"
#include "instances/polish_gen.inc"
#include "instances/step.inc"
#include "instances/instance.inc"
#include "instances/design_a.inc"
#include "instances/design_b.inc"
#include "instances/dare.inc"
#include "instances/c2d.inc"
#include "instances/sens.inc"
#include "instances/sens_ltv.inc"
#include "instances/cert.inc"
#include "instances/cert_ltv.inc"
#undef ALMPC_KERNEL_INSTANCE
#endif

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

using namespace almpc;

// Memory: every device and pinned buffer of a handle is a DevBuf member (csrc/almpc_devbuf.h) and goes when the handle is deleted
// (destroy_handle); nothing else frees.  The raw pointers below are views that own nothing:
//   dX0                             the handle's own x0 buffer (x0_own) or a slot of the pinned x0 ring (io.x0_slot says which);
//   io.dX0[] / io.dU0[] / io.dInts[], redo.dUnsolved   the device's addresses of pinned memory (io.hX0 / hU0 / hInts, redo.hUnsolved).
// The iterate of an SQP loop lives in the handle's own reference buffers (dXref, dUref); rGuess is filled from another handle's
// inputs (almpc_set_start_from) but belongs to the handle that starts from it.
struct almpc_handle {
    int n = 0, m = 0, N = 0, batch = 0, nz = 0, nzs = 0, nrb = 0, ks = 0, ksf = 0, device = 0;
    uint32_t flags = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool designed = false;
    double rho = 0.1, sigma = 1e-6;
    // host copies of the design (almpc_get_design)
    std::vector<double> H, F, P, d;
    // device: shared design
    DevBuf<double> dMinvFrag, dVFrag, dHFrag, dFFrag, dG;
    // Cold start's affine first ADMM iterate xt1 = W e0 + wS and the prologue's row-constant table.  No allocation of their own: the
    // shared design hands over two of its temporaries instead of freeing them -- the plain Minv [nz][nzs] and a workspace of at least
    // n * nzs doubles, laid out [W = -Minv F': n * nzs | wS = -Minv fS: nzs | table: 8 * nzs].  wS and the table belong to a SHARED
    // reference (almpc_set_reference makes them where the workspace has room for them: cold_ref); per-instance references, which
    // would need batch * nz doubles of wS, take the full first product and the per-row loads.
    DevBuf<double> dMinv, dCold;
    bool cold_ref = false;   // wS and the table in dCold are those of the current (shared) reference
    DevBuf<double> dD, dUmin, dUmax, dA, dB;
    DevBuf<double> dXref, dUref, dFS, dV0S, dRho;
    bool ref_keep = false;   // dXref, dUref, dFS, dV0S are as almpc_set_reference made them: it keeps all four while their sizes stay
    DevBuf<double> wQ, wR, wS;   // design weights on the device (almpc_design_batched / _ltv)
    // almpc_design_batched_weighted: one (Q_i, R_i, S_i) per instance, [batch][n*n] and [batch][m*m] twice, symmetrised as the design
    // takes them.  Made by that call only (wiS: when it is given an S_batch); every other design leaves `weighted` off (drop_lazy_redo)
    DevBuf<double> wiQ, wiR, wiS;
    bool weighted = false, wiS_given = false;   // (wiS_given: wiS holds this design's S_i)
    // ... staged through pinned host buffers of the same sizes (the symmetrised sets: no page faults and no staging copy per design);
    // hSi is also what almpc_set_reference forms fS from while the input-rate term is part of the cost
    PinBuf<double> hQi, hRi, hSi;
    int rho_mode = 0;  // 0 scalar rho (OSQP), 1 stiffness profile rho / G_ii
    // blocked rollout of the shared model (rollout_blocked): [Gamma_s | Phi_s] rows per lane, built at design time
    DevBuf<double> dRollM;
    int roll_s = 0, roll_nb = 0;  // roll_s == 0: shape not covered (n > ROLL_NX or m > ROLL_SMX), the stage-by-stage rollout is used
    long xref_stride = 0, uref_stride = 0, fS_stride = 0;
    // The cost weights a design keeps for its readers (almpc_set_reference's fS, almpc_get_weights_instance, the parameter gradients,
    // k_sens_face_rate, the certificates): the only host copy -- with the shared P above -- and the only device copy made from it;
    // the solvers' own buffers (rQ.., wQ.., wiQ.., sd.dQ.., sqp.Q.., relin.Q..) hold what their kernels take.  keep_weights() fills it
    // in every design and setup path, kept_on_device() is the only writer of W (DESIGN.md "Where a design's weights live").
    // Q, R: as the path takes them (almpc_design_shared's as given, else symmetrised; a weighted design's: instance 0's), empty where
    // it keeps none (structured designs, the SQP setup); S: symmetrised (a structured design's as given, zeros where its branch drops
    // it); useR: R[1,1] != 0, useS: and S[1,1] != 0 -- the input-rate term is part of the cost (src/sub/design_mpc.jl:423-466)
    struct Kept {
        std::vector<double> Q, R, S;
        int useR = 0, useS = 0;
        DevBuf<double> W;         // [Q n*n | R m*m | S m*m | P n*n]
        uint32_t on_device = 0;   // KEPT_* parts of W that hold the current design's matrices (none after a design: drop_lazy_redo)
    } kept;
    // device: per-instance state and results
    double* dX0 = nullptr;   // view: x0_own or a slot of the pinned ring
    DevBuf<double> x0_own, dXs, dZs, dYs, dV0, dW;
    DevBuf<double> dX, dEx, dU, dEu;
    DevBuf<int32_t> dStatus, dIters, dPiters, dPerm;
    DevBuf<uint32_t> dYflags;  // [batch][nrb] signs of the ADMM multipliers (steps run with ALMPC_OPT_NO_WARM_STATE)
    bool state_valid = true;      // xs / ys hold the ADMM state of the last step (a warm start may use them)
    int num_cus = 256;            // persistent-grid size of k_polish<true>
    Switches sw;                  // the ALMPC_* diagnostic switches as almpc_create found them (csrc/almpc_switches.h): fixed for the handle's life
    int fuse_step = 1;            // one kernel per step when the shape allows (almpc_set_step_fusion; starts off with ALMPC_NO_FUSED_STEP=1)
    DevBuf<double> dSglobal;  // polish scratch for working sets beyond 32 rows
    DevBuf<int32_t> dStartRows;   // [batch][65] row list of a guessed working set whose inverse sits in dSglobal (k_guess_iterate_ws)
    // state rows (state box / terminal equality): constraint-space data for k_polish_gen
    int terminal_eq = 0, has_box = 0, mc = 0, R = 0, Rs = 0, np_pairs = 0;
    DevBuf<double> dGhat, dGnorm, dXmin, dXmax;
    DevBuf<int> dRowTraj, dRowEq, dRowXidx, dRowState;
    DevBuf<double> dOvfSinv;    // [batch][32 * 32 + 32] k_polish_gen -> k_polish_gen64: inverse and bounds of a flagged instance
    DevBuf<double> dVsPlain;    // [n][nzs] V = -G F' (shared design with state rows): operand of the s0 table
    DevBuf<double> dPlain;      // small shared designs (nzs <= 64): dense [Minv | H' | F' | V] for the one-wave-per-instance step
    DevBuf<double> dS0Basis;    // [(n + 1)][Rs] PolishGenParams::s0_basis
    bool s0_basis_ok = false;
    DevBuf<int32_t> dOverflow;  // [2 + batch] k_polish_gen: count, cursor and list of instances to redo with the 64-row build
    DevBuf<int> dRowMap;        // [N*n] state (stage k+2, i) -> state-row index or -1 (k_ghat_inst)
    DevBuf<double> dGhatE, dWinvE;  // shared design with the terminal equality: original rows E of Ghat, Ghat_EE^-1
    int eq_proj = 0;               // dGhat is the matrix projected on the terminal equality (k_ghat_project)
    bool ghat_inst = false;        // dGhat / dGnorm hold one constraint-space matrix PER INSTANCE ([batch][R][Rs], [batch][Rs])
    std::vector<double> boxmin, boxmax;  // almpc_set_state_box: the state box of the per-instance / time-varying / SQP designs
    DevBuf<double> lA, lB, lC, lE;  // almpc_design_ltv with state rows: stage models, defects and
                                                                        // state errors kept for the step's rollouts
    // per-instance models (almpc_design_batched): persistent per-instance operands ...
    bool batched = false;
    bool ltv = false;             // almpc_design_ltv: references and gradient are part of the design
    DevBuf<double> bQ;         // [batch][nz] explicit gradient of an LTV design (unscaled)
    DevBuf<double> bA, bB, bMinv, bG, bHs, bFs, bVs, bD, bRho, bH, bF;
    // ... and design temporaries kept for the next re-design (a per-step re-linearisation designs every step)
    DevBuf<double> bPhi, bGk, bGam, bW, bWP, bP;
    DevBuf<int> bFlag;
    bool batched_alloc = false;
    bool minv_packed = false;   // bMinv holds packed lower triangles (stride packed_tri_doubles): k_admm_inst<true>
    // SQP outer loop for a black-box Fnn model (almpc_sqp_fnn_*): the network, the stage data of the current linearisation
    // a black-box network on the device (the SQP loop's and the re-linearisation pipeline's)
    struct Net {
        int H = 0, L = 0, act = 0, net = 0;   // act: activation 0..4, net: NET_* (decode_net)
        DevBuf<double> W_in, W_h, b_h, W_out;
    };
    struct Sqp : Net {
        bool ready = false, started = false;
        int useR = 0, useS = 0;
        long sP = 0;
        DevBuf<double> A, B, c, fval, ebar, qadd;
        DevBuf<double> xref, uref, Q, R, S;
        DevBuf<int> bad;
        DevBuf<double> mer;    // [batch][4] step rule 1: step factor, merit of the last accepted point, redo flag
        DevBuf<double> xback, uback, dxback, vback;  // last accepted point and its step
        double mu = 0.0;          // merit weight of the defects
        int step_rule = 0;        // 0 fixed step, 1 merit-function safeguard (almpc_sqp_fnn_set_step_rule)
        long since_start = 0;     // iterations since almpc_sqp_fnn_start: the first one gets its guess from ADMM, the others from the iterate
        int structured_qp = 0;       // almpc_sqp_fnn_set_structured: every iteration's QP goes to k_riccati in its stage-wise form
                                     // (no condensed design at all: no Hessian build, no inverse, no m N <= 128 limit)
        DevBuf<unsigned long long> stats;  // [iters][2]
        // almpc_sqp_fnn_solve: per-instance done | iters | verdict words and the live count ([3 batch + 1]), last residuals [batch],
        // and a pinned ring of live counts the host reads two iterations behind the device
        DevBuf<int> sv;
        DevBuf<double> kkt;
        PinBuf<int> live_pin;
        // almpc_sqp_fnn_set_hessian: 0 Gauss-Newton, 1 exact Lagrangian Hessian (multipliers [batch][N][n], stage blocks [batch][N][(n+m)^2])
        int hessian = 0;
        DevBuf<double> lam, Wlag;
        // almpc_sqp_fnn_set_row_multipliers: the finishes hand out the state-row multipliers of every iteration's QP ([batch][N][n], zero
        // until the first solved QP); the stopping test and the exact Hessian take them into the adjoint.  Allocated when the handle has state rows.
        int row_mult = 0;
        DevBuf<double> smu;
        void reset_keeping_switches() {   // a new setup: everything goes but what the set_* calls chose
            Sqp fresh; fresh.step_rule = step_rule; fresh.structured_qp = structured_qp; fresh.hessian = hessian; fresh.row_mult = row_mult;
            *this = std::move(fresh);
        }
    } sqp;
    // per-step re-linearisation of a black-box Fnn model on the device (almpc_relin_fnn_*, BASELINE configs[3])
    struct Relin : Net {
        bool ready = false;
        int useR = 0, useS = 0;
        DevBuf<double> ulin;   // [batch][m] linearisation input of every instance (the first input reference)
        DevBuf<double> Q, R, S;
        DevBuf<double> gS;     // [nz] unscaled input-rate gradient 2 D'Sbar D u_ref of the shared reference
        bool have_prev = false;   // a step has been solved since setup: its inputs can seed the next step's working set
        DevBuf<double> u0, xnext;   // [batch][m] applied inputs, [batch][n] next states (almpc_relin_fnn_advance)
        DevBuf<double> Ascr, Bscr;  // Jacobian outputs of the advance's forward pass (not used)
        float ms_jac = 0, ms_design = 0, ms_step = 0;  // last timed step (almpc_relin_fnn_step with timing)
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    } relin;
    // structured (Riccati) solve: the handle's only solver (ALMPC_FLAG_STRUCTURED) or the fallback for instances the condensed path
    // leaves unsolved (almpc_set_structured_fallback)
    bool structured = false;
    // Redo of the instances a condensed step leaves undecided (fallback == 2 on the shared-model / input-box-only path, whose steps are
    // tens of microseconds and leave an instance unsolved only in corner cases).  The finish counts such instances into a pinned word
    // and stores the step's number in the gate word; the redo kernels are launched only when there is work -- no extra launch on the
    // step path (measured: two idle redo launches cost 14 us per 61 us step).  Transitions:
    //  - a step (run_step) numbers itself (step_serial += 1) and, if its redo is deferred, sets lazy_pending;
    //  - resolve_lazy_redo (a synchronous look, stream idle): clears lazy_pending; if the count moved since unsolved_seen, takes the new
    //    count and redoes the undecided instances now; redo_expected = whether it moved;
    //  - enqueue_gated_redo (tickets, almpc_advance_plant, almpc_relin_fnn_advance: results leave without a host look): enqueues the
    //    redo behind the step GATED -- a gated launch returns at once unless the gate word holds its step's number -- and clears
    //    lazy_pending.  Every read path hands out "solution or verdict" (src/main/computation_mpc.jl:41-53) at the cost of two (three
    //    with per-instance stage records) empty launches per step on those paths only;
    //  - wait_and_settle: when redo_expected, the gated redo goes out before the wait (predicted), then the count is taken as above;
    //  - drop_lazy_redo (a new design): clears lazy_pending and redo_expected, takes the count.
    struct Redo {
        DevBuf<int, Mem::PinnedMapped> hUnsolved;   // pinned host word: instances left undecided, counted by the finishes
        int* dUnsolved = nullptr;      // view: the device's address of it
        DevBuf<int> dGate;          // gate word: number of the last step that left an instance undecided
        int unsolved_seen = 0;         // the count at the last look
        int step_serial = 0;           // number of the last enqueued step (1, 2, ...)
        bool lazy_pending = false;     // the last step's redo is deferred and not yet settled
        bool expected = false;         // the last synchronous look found undecided instances (see wait_and_settle)
    } redo;
    int fallback = 2;   // 0 off, 1 asked for (a design it cannot serve is an error), 2 default: on wherever the stage-wise solvers cover the design
    DevBuf<double> rQ, rR, rP, rKst, rPst;   // device copies of Q, R (branch rule applied), shared P; gain scratch
    DevBuf<double> rGuess;   // [batch][N][m] start of the next structured solve (almpc_set_start_from / opts.warm_start), else nullptr
    bool guess_ready = false;   // rGuess was filled for the NEXT almpc_calculate (consumed by it)
    bool r_has_step = false;    // a structured step has run on this design: its inputs can seed a warm start
    hipEvent_t ev_guess = nullptr, ev_guess_done = nullptr;
    long rP_stride = 0;   // per-instance terminal weights (batched designs): doubles between instances of bP, else 0 with rP
    bool r_batched_P = false;
    // almpc_set_terminal_weight: 1 = the terminal weight of a per-instance design is the instance's own DARE solution, computed on the
    // device (k_dare, csrc/almpc_dare.hip.h).  Its buffers exist only once a design or setup has run with the mode on.
    int terminal_mode = 0;
    bool t_step = false;        // the re-linearisation pipeline was set up with the mode on: every step solves its own DAREs into bP
    long bP_stride = 0;         // doubles between the instances of bP as the last per-instance design left it (0: one shared matrix)
    DevBuf<double> tP;          // [n][n] the setup's P: terminal weight of an instance whose own DARE has no stabilising solution
    DevBuf<int32_t> tStat;      // [batch] k_dare's status words of the last design / step
    // almpc_set_model_time: 1 = the models a design is given (almpc_design_shared, almpc_design_batched) and the network of the
    // re-linearisation pipeline are continuous-time; they are discretised by zero-order hold at model_Ts (hm::c2d on the host for a
    // shared model, k_c2d in place on the per-instance model slots, csrc/almpc_c2d.hip.h).  cStat exists only once the mode was used.
    int model_mode = 0;
    double model_Ts = 0.0;
    bool c_step = false;        // the re-linearisation pipeline was set up with the mode on: every step discretises its Jacobians
    DevBuf<int32_t> cStat;      // [batch] k_c2d's status words of the last design / step
    // Solution sensitivities (almpc_sensitivity, almpc_sensitivity_vjp; k_sens, csrc/almpc_sens.hip.h).  Every buffer is made at the
    // first call that needs it (grow): a handle that never asks allocates and launches what it did.
    struct Sens {
        DevBuf<double> K0, dU, dX;      // [batch][n][m], [batch][n][N][m], [batch][n][N+1][n] of the last almpc_sensitivity
        DevBuf<int32_t> rows;           // [batch] its |W| per instance (-1: not solved)
        uint32_t have = 0;              // ALMPC_SENS_* bits the buffers hold for the LAST step (0: none)
        DevBuf<double> V;               // [n][nzs] plain V of a shared design (the handle keeps it in MFMA fragment order only)
        bool v_ok = false;              // ... unpacked from the current design
        DevBuf<double> T1;              // [n][Rs] row values of the unconstrained minimiser (rows form: k_sens_rows_table)
        bool t1_ok = false;             // ... built from the current design
        DevBuf<double> HF;              // [nz][nz] H, [n][nz] F unscaled: what the table kernel refines V against
        DevBuf<int32_t> ovf;            // [SENS_OVF_HEAD + batch] instances beyond the first tier's 32 rows
        DevBuf<double> gu, gx, gx0;     // VJP: uploaded loss gradients, result [batch][n]
        DevBuf<int32_t> vrows;          // [batch] |W| of the last VJP
        bool stepped = false;           // a step has run on the current design
        // parameter gradients (almpc_sensitivity_params_vjp), made at the first such call; the weights are the handle's kept ones
        DevBuf<double> pz;             // [batch][nz] z | [batch][nz] nu | [batch][m] dL/dumin | [batch][m] dL/dumax (k_sens_pz)
        DevBuf<double> pout;            // k_sens_params' outputs: u_ref, Q, P, A, R, S, B, each [batch][its size]
        DevBuf<double> traj;            // [workgroups][3][(N+1) n] zeta, mu, al of the instance a workgroup is at
        DevBuf<int32_t> dstat;          // [batch] k_dare_vjp's status words (almpc_sensitivity_params_vjp_dare)
        DevBuf<double> Kst;             // [batch][N][m n] stage gains of k_sens_face (almpc_sensitivity_stagewise with dU or dX);
                                        // [batch][N][m (n + m)] those of k_sens_face_rate (its S: the kept one, shared on every structured design);
                                        // k_sens_ltv's (almpc_sensitivity_ltv), of either width
    } sens;
    // Certificate of the last step (almpc_certificate, almpc_relin_fnn_certificate: k_cert, csrc/almpc_cert.hip.h; almpc_certificate_ltv:
    // k_cert_ltv, csrc/almpc_cert_ltv.hip.h).  As with sens, every buffer is made at the first call that needs it.
    struct Cert {
        DevBuf<double> cost, res, grad, costate;   // [batch], [batch], [batch][N][m], [batch][N+1][n] of the last certificate call
        DevBuf<double> x, ex;                      // [batch][N+1][n] of the last almpc_certificate_ltv
        uint32_t have = 0;                         // ALMPC_CERT_* (| ALMPC_CERT_STATES) bits the buffers hold for the LAST step (0: none)
        bool ltv_form = false;                     // ... filled by almpc_certificate_ltv: the getters of the other form are refused
        // what a design with almpc_set_keep_stage_models on leaves for almpc_certificate_ltv: lA, lB, lC and the shared references here
        int keep = 0;                             // almpc_set_keep_stage_models: read by the next almpc_design_ltv
        bool kept = false, kept_c = false;         // the current design is almpc_design_ltv's and left its stage models (and defects)
        DevBuf<double> xref, uref;                 // [N+1][n], [N][m] the design's shared references (zeros for NULL)
    } cert;
    // almpc_design_ltv_stagewise (a structured handle): a caller's time-varying design on the stage-wise solvers.  The stage models
    // live in lA, lB, lC (always kept: the solvers read them, and so can almpc_certificate_ltv / almpc_sensitivity_ltv), the shared
    // references in cert.xref / cert.uref, the iterate (xbar, ubar) in dXref / dUref, the weights in wQ, wR, wS, bP.  Every buffer is
    // made by the design call; almpc_ltv_stagewise_update copies into them and launches k_ltv_stage_prepare, nothing else.
    struct Lsw {
        bool ready = false, has_c = false;
        long sP = 0;                         // doubles between the instances' terminal weights in bP (0: one shared matrix)
        DevBuf<double> ebar, qadd, eqt;      // k_ltv_stage_prepare: [batch][N][n], [batch][N][m], [n] (with the terminal equality)
        DevBuf<double> xst, ust;             // host form: xbar, ubar staged in front of the kernel
    } lsw;
    // stage-wise dual active-set solve (k_sdual, csrc/almpc_sdual.hip.h): input box, state box, terminal equality and S in the
    // multiple-shooting form; stage records of the unconstrained problem (shared: host Riccati at design time)
    struct Sd {
        bool ready = false;
        int nt = 0, NT = 0, MC = 0;          // stage-state dimension (n, or n + m with S) and the instantiated (padded) dimensions
        DevBuf<double> rec; long rec_stride = 0, rec_kstride = 0;
        DevBuf<double> base; long base_stride = 0; bool has_base = false;
        DevBuf<double> xmin, xmax, eqt;   // state box [n] (null: none), terminal-equality target [n] zeros (null: none)
        bool has_box = false, has_eq = false, useS = false;
        bool per_instance = false;          // records per instance (k_sgains) instead of the host's shared ones
        int gain_N = 0;                     // stages k_sgains computes (1: stage-invariant records)
        DevBuf<double> dQ, dR, dS, dP;   // weights of k_sgains (R with the branch rule applied; dP: a shared terminal weight)
        DevBuf<int> bad;                 // [batch] k_sgains: R + B'PB not positive definite
        bool sqp = false;                   // the QP of an SQP iteration: stage models, defects and cost terms of the loop (h->sqp)
        DevBuf<double> pc, ct;   // [batch][N][NT] P_{k+1} c_k, c_k
        DevBuf<int32_t> ovf;
        DevBuf<int32_t> wsave;   // [batch][SDUAL_WSAVE] working set of an instance that ran out of room (start of the next tier)
        DevBuf<double> sinv_save;   // [batch][sdual_sinv_doubles(SDUAL_SINV_SAVE)] its inverse (allocated at the first multi-tier solve)
        int tier_serial = 0;           // number of the last launch_sdual_t call (the tiers' gate value)
        DevBuf<double> start_inv;   // [batch][sdual_sinv_doubles(SDUAL_SINV_SAVE)] inverse of a redo's start (k_sdual_start; allocated at the first such redo)
        DevBuf<int32_t> start_ws;   // [batch][64] working sets the state-row finish of the LAST step gave up with (PolishGenParams::redo_ws)
        bool start_ws_fresh = false;   // ... written by the last enqueued step (cleared by every step that does not run that finish)
        DevBuf<double> sinv_glb;   // third tier: Sinv of 128 x 129 per wave of its grid
        DevBuf<double> ghat; bool ghat_ready = false, ghat_wanted = false;   // shared model: cached sweep responses [TP][TP] (k_sdual: SdualParams::ghat)
        std::vector<double> S;               // symmetrised S (base terms of time-varying input references)
        // reachability screen of the state box (k_state_box_screen): tables of the shared model and references, verdicts per instance
        DevBuf<double> scr_phi, scr_g, scr_rm, scr_rp;
        DevBuf<int32_t> scr_verdict;
        bool scr_ready = false;              // tables match the current model / references
    } sd;
    // multi-GPU (almpc_comm_*): this handle's rank in an RCCL communicator of one process per GPU
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    DevBuf<long long> dComm4;       // [4] summary words
    DevBuf<double> dU0, dU0all;  // [batch][m] packed first inputs, [world][batch][m] gathered
    // host-facing step path (almpc_update_initialization_async, almpc_get_results_async / _wait, almpc_get_first_input): pinned
    // staging owned by the handle, copies on their own streams, rings of IO_DEPTH slots so that the transfers of one step run
    // under the kernel of the next (csrc/almpc_hostio.inc.h)
    static constexpr int IO_DEPTH = 2;
    struct Io {
        bool ready = false;
        hipStream_t s_out = nullptr;
        // ALMPC_X0_UPLOAD=1: the pinned slot is copied into a device slot by the copy engine on a stream of its own, under the step that
        // is running, instead of being read in place by the kernels.  Reading in place costs the step +9 us at the benchmark shape
        // (393 KB over the link at its START, tools/dbg_x0_home.py), the upload costs three HIP calls and a copy-engine latency per step:
        // measured 11.7 k (upload) against 12.8 k (in place) batch-steps/s on the pipelined first-move loop, 8.3 k against 10.4 k serial
        hipStream_t s_in = nullptr;
        DevBuf<double, Mem::DeviceTight> dX0dev[IO_DEPTH];
        hipEvent_t ev_in[IO_DEPTH] = {nullptr, nullptr};
        // x0 ring: pinned host slots the kernels read in place (dX0 = the device's address of the slot); h->dX0 points at the latest
        PinBuf<double> hX0[IO_DEPTH];
        double* dX0[IO_DEPTH] = {nullptr, nullptr};           // views: the device's addresses of hX0
        hipEvent_t ev_used[IO_DEPTH] = {nullptr, nullptr};   // the last step that read the slot has finished (recorded on the compute stream)
        bool used_pending[IO_DEPTH] = {false, false};
        int x0_slot = -1;     // slot h->dX0 points at (-1: the handle's own buffer, x0_own)
        long x0_count = 0;
        // result ring: ticket t lives in slot t % IO_DEPTH
        PinBuf<double> hX[IO_DEPTH], hEx[IO_DEPTH], hU[IO_DEPTH], hEu[IO_DEPTH], hU0[IO_DEPTH];
        PinBuf<int32_t> hInts[IO_DEPTH];                     // pinned [3][batch]: status | iters | polish_iters
        double* dU0[IO_DEPTH] = {nullptr, nullptr};          // views: the device's addresses of hU0 / hInts (the pack kernel writes the
        int32_t* dInts[IO_DEPTH] = {nullptr, nullptr};       // pinned slots directly)
        hipEvent_t ev_packed[IO_DEPTH] = {nullptr, nullptr}; // compute stream: the results of the slot's step exist (copy-out stream waits)
        hipEvent_t ev_done[IO_DEPTH] = {nullptr, nullptr};   // everything the slot's request asked for has landed in pinned memory
        hipEvent_t ev_big = nullptr;                          // the last read-back of x / e_x / u / e_u has left the result buffers (the next step waits for it)
        uint32_t want[IO_DEPTH] = {0, 0};
        long ticket[IO_DEPTH] = {-1, -1};
        long next_ticket = 0;
        bool big_copy_pending = false;  // a read-back of x / e_x / u / e_u (straight from the result buffers) may still be running:
        int big_copy_slot = 0;          // the next step waits for it before it overwrites them
    } io;
    // timing (ALMPC_FLAG_TIMING): one set of 4 events per step since the last almpc_timing_reset
    std::vector<hipEvent_t> ev;  // 4 per step
    std::vector<char> ev_two;    // per recorded step: 1 = a one-kernel step, only its events 1 and 2 (around the kernel) were recorded
    size_t ev_used = 0;          // steps recorded
    int timing_stride = 1;       // record events on every timing_stride-th step only (each event costs ~3 us of stream time)
    size_t step_count = 0;
};

namespace {

int fail(almpc_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

#define HIP_TRY(h, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(h, ALMPC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));   \
    } while (0)

// ... and of the library's own calls: anything but ALMPC_OK is the caller's return value (the message is in h->err already)
#define ALMPC_TRY(expr)                        \
    do {                                       \
        const int rc_try_ = (expr);            \
        if (rc_try_ != ALMPC_OK) return rc_try_; \
    } while (0)

int pick_ks(int nz, int nrb) {
    const int exact = (nz + 3) / 4;
    // instantiated (NRB, KS) pairs: KS = 4*NRB always; plus the exact-fit specials below
    if (nrb == 8 && exact <= 30) return 30;
    if (nrb == 3 && exact <= 10) return 10;
    if (nrb == 1 && exact <= 3) return 3;
    return 4 * nrb;
}

template <int NRB, int KS>
hipError_t launch_admm_t(const AdmmParams& p, int grid, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((k_admm<NRB, KS>), dim3(grid), dim3(64 * NRB), lds, st, p);
    return hipGetLastError();
}

hipError_t launch_admm(int nrb, int ks, const AdmmParams& p, int grid, size_t lds, hipStream_t st) {
#define CASE(NRB_, KS_) if (nrb == NRB_ && ks == KS_) return launch_admm_t<NRB_, KS_>(p, grid, lds, st)
    CASE(1, 3); CASE(1, 4); CASE(2, 8); CASE(3, 10); CASE(3, 12); CASE(4, 16); CASE(5, 20); CASE(6, 24);
    CASE(7, 28); CASE(8, 30); CASE(8, 32);
#undef CASE
    return hipErrorInvalidValue;
}

void io_free(almpc_handle* h);   // almpc_hostio.inc.h

// After almpc_update_initialization_async h->dX0 points at a pinned host slot the kernels read in place.  Entry points that WRITE x0
// through a device-side copy go back to the handle's own device buffer first.
void io_release_x0(almpc_handle* h) {
    if (h->io.x0_slot >= 0) {
        h->dX0 = h->x0_own;
        h->io.x0_slot = -1;
    }
}

// The end of a handle, in this order: the host-facing side's streams and events, the other events, the communicator, then the handle
// with every buffer it owns (DevBuf members), the stream last.
void destroy_handle(almpc_handle* h) {
    io_free(h);
    for (auto& e : h->relin.ev)
        if (e) (void)hipEventDestroy(e);
    if (h->comm && rccl_api().ok) (void)rccl_api().CommDestroy(h->comm);
    if (h->ev_guess) (void)hipEventDestroy(h->ev_guess);
    if (h->ev_guess_done) (void)hipEventDestroy(h->ev_guess_done);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    const hipStream_t stream = h->stream;
    delete h;
    if (stream) (void)hipStreamDestroy(stream);
}

// State rows of a design: the state box for stages 2..N+1 (stage 1 is x0 itself, checked per instance) and / or the terminal
// equality on stage N+1 (which then replaces the box rows of that stage).  Fills the row tables and (re)allocates the
// constraint-space matrix: one for the handle (shared model) or one per instance.  mc = 0 afterwards: no state rows.
int setup_state_rows(almpc_handle* h, const double* xmin, const double* xmax, bool per_instance) {
    const int n = h->n, m = h->m, N = h->N, nz = h->nz;
    h->has_box = xmin ? 1 : 0;
    std::vector<int> row_traj, row_eq, row_xidx, row_state, rowmap((size_t)N * n, -1);
    if (h->has_box)
        for (int i = 0; i < n; ++i)
            if (!(xmin[i] <= xmax[i])) return fail(h, ALMPC_ERR_INVALID, "design: xmin > xmax");
    for (int k = 0; k < N; ++k)
        for (int i = 0; i < n; ++i) {
            const bool is_eq = h->terminal_eq && k == N - 1;
            if (!(h->has_box || is_eq)) continue;
            rowmap[(size_t)k * n + i] = (int)row_traj.size();
            row_traj.push_back((k + 1) * (n + m) + i);
            row_eq.push_back(is_eq ? 1 : 0);
            row_xidx.push_back((k + 1) * n + i);
            row_state.push_back(i);
        }
    h->mc = (int)row_traj.size();
    h->R = nz + h->mc;
    h->np_pairs = (h->R + 127) / 128;
    h->Rs = 128 * h->np_pairs;
    h->dGhat.reset(); h->dGnorm.reset(); h->dXmin.reset(); h->dXmax.reset();
    h->dRowTraj.reset(); h->dRowEq.reset(); h->dRowXidx.reset(); h->dRowState.reset(); h->dRowMap.reset();
    h->ghat_inst = false;
    h->dGhatE.reset(); h->dWinvE.reset();
    h->eq_proj = 0;
    if (h->mc == 0) return ALMPC_OK;
    if (h->np_pairs > 4) return fail(h, ALMPC_ERR_UNSUPPORTED, "design: state rows need n*N + m*N <= 512");
    if ((size_t)(N + 1) * (n + m) > 32 * 32) return fail(h, ALMPC_ERR_UNSUPPORTED, "design: state rows need (N+1)*(n+m) <= 1024");
    if (per_instance && n > 32) return fail(h, ALMPC_ERR_UNSUPPORTED, "design: state rows with per-instance models need n <= 32");
    const size_t copies = per_instance ? (size_t)h->batch : 1;
    HIP_TRY(h, h->dGhat.alloc(copies * h->R * h->Rs));
    HIP_TRY(h, h->dGnorm.alloc(copies * h->Rs));
    if (per_instance) HIP_TRY(h, hipMemset(h->dGhat, 0, copies * h->R * h->Rs * sizeof(double)));  // (the padding columns stay zero)
    HIP_TRY(h, h->dXmin.alloc((size_t)n)); HIP_TRY(h, h->dXmax.alloc((size_t)n));
    HIP_TRY(h, h->dRowTraj.alloc((size_t)h->Rs)); HIP_TRY(h, h->dRowEq.alloc((size_t)h->Rs));
    HIP_TRY(h, h->dRowXidx.alloc((size_t)h->Rs)); HIP_TRY(h, h->dRowState.alloc((size_t)h->Rs));
    HIP_TRY(h, h->dRowMap.alloc(rowmap.size()));
    HIP_TRY(h, hipMemcpy(h->dRowMap, rowmap.data(), rowmap.size() * sizeof(int), hipMemcpyHostToDevice));
    auto up = [&](int* dst, const std::vector<int>& v, int fill) {
        std::vector<int> full((size_t)h->Rs, fill);
        for (size_t i = 0; i < v.size(); ++i) full[(size_t)nz + i] = v[i];
        return hipMemcpy(dst, full.data(), full.size() * sizeof(int), hipMemcpyHostToDevice);
    };
    HIP_TRY(h, up(h->dRowTraj, row_traj, 0)); HIP_TRY(h, up(h->dRowEq, row_eq, 0));
    HIP_TRY(h, up(h->dRowXidx, row_xidx, 0)); HIP_TRY(h, up(h->dRowState, row_state, 0));
    std::vector<double> lo(n, -1e300), hi(n, 1e300);
    if (h->has_box) { lo.assign(xmin, xmin + n); hi.assign(xmax, xmax + n); }
    HIP_TRY(h, hipMemcpy(h->dXmin, lo.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->dXmax, hi.data(), n * sizeof(double), hipMemcpyHostToDevice));
    h->ghat_inst = per_instance;
    return ALMPC_OK;
}

// Ghat_i of every instance from the per-instance design in place (G_i, d_i) and the models the rows roll out through: the
// time-invariant slots (bA, bB) or stage models [batch][N][..] (A_all / B_all non-null).  Launch only (handle's stream).
hipError_t launch_ghat_inst(almpc_handle* h, const double* A_all, const double* B_all) {
    GhatInstParams gp;
    gp.n = h->n; gp.m = h->m; gp.N = h->N; gp.nz = h->nz; gp.nzs = h->nzs; gp.mc = h->mc; gp.R = h->R; gp.Rs = h->Rs;
    const long n = h->n, m = h->m, N = h->N;
    if (A_all) { gp.A = A_all; gp.B = B_all; gp.A_stride = N * n * n; gp.B_stride = N * n * m; gp.A_kstride = n * n; gp.B_kstride = n * m; }
    else { gp.A = h->bA; gp.B = h->bB; gp.A_stride = n * n; gp.B_stride = n * m; gp.A_kstride = 0; gp.B_kstride = 0; }
    gp.G = h->bG; gp.G_stride = (long)h->nz * h->nzs; gp.dvec = h->bD; gp.d_stride = h->nzs;
    gp.rowmap = h->dRowMap; gp.Ghat = h->dGhat; gp.Ghat_stride = (long)h->R * h->Rs; gp.gnorm = h->dGnorm; gp.gnorm_stride = h->Rs;
    const size_t lds = (size_t)(n * (n + m) + 2) * sizeof(double);
    const dim3 grid((unsigned)h->batch), block(GHAT_THREADS);
    if (n <= 4) hipLaunchKernelGGL((k_ghat_inst<4>), grid, block, lds, h->stream, gp);
    else if (n <= 8) hipLaunchKernelGGL((k_ghat_inst<8>), grid, block, lds, h->stream, gp);
    else if (n <= 16) hipLaunchKernelGGL((k_ghat_inst<16>), grid, block, lds, h->stream, gp);
    else hipLaunchKernelGGL((k_ghat_inst<32>), grid, block, lds, h->stream, gp);
    return hipGetLastError();
}

// The weights a design or setup path takes, into the handle's record (Q, R null: none kept); what is on the device is the last design's
void keep_weights(almpc_handle* h, const hm::mat* Q, const hm::mat* R, const hm::mat& S, bool useR, bool useS) {
    almpc_handle::Kept& k = h->kept;
    k.Q = Q ? *Q : hm::mat(); k.R = R ? *R : hm::mat(); k.S = S;
    k.useR = useR; k.useS = useS; k.on_device = 0;
}

// The parts of that record (and the shared P) a reader needs, on the device: each goes there once per design, in stream order in
// front of the reading kernel.  d: the needed pointers, null for the rest.  (That a needed matrix is kept is the caller's check.)
enum : uint32_t { KEPT_Q = 1u, KEPT_R = 2u, KEPT_S = 4u, KEPT_P = 8u };
struct KeptDev { const double *Q, *R, *S, *P; };
int kept_on_device(almpc_handle* h, uint32_t need, KeptDev& d) {
    almpc_handle::Kept& k = h->kept;
    const size_t nn = (size_t)h->n * h->n, mm = (size_t)h->m * h->m;
    const std::vector<double>* src[4] = {&k.Q, &k.R, &k.S, &h->P};
    const size_t len[4] = {nn, mm, mm, nn}, off[4] = {0, nn, nn + mm, nn + 2 * mm};
    if (need) HIP_TRY(h, k.W.grow(2 * nn + 2 * mm));
    const double* at[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; ++i) {
        if (!(need >> i & 1u)) continue;
        if (!(k.on_device >> i & 1u)) {
            if (src[i]->size() != len[i]) return fail(h, ALMPC_ERR_INVALID, "the design's weights are not kept");
            HIP_TRY(h, hipMemcpyAsync(k.W + off[i], src[i]->data(), len[i] * sizeof(double), hipMemcpyHostToDevice, h->stream));
        }
        at[i] = k.W + off[i];
    }
    k.on_device |= need;
    d = KeptDev{at[0], at[1], at[2], at[3]};
    return ALMPC_OK;
}

// Device copies of the weights the structured solve uses (R with the reference's branch rule applied: zero if R[1,1] == 0)
int riccati_weights(almpc_handle* h, const hm::mat& Qm, const hm::mat& Rm, const double* Pshared) {
    const int n = h->n, m = h->m;
    hm::mat Qs = hm::symmetrised(Qm.data(), n), Rs = hm::symmetrised(Rm.data(), m);
    if (Rm[0] == 0.0) std::fill(Rs.begin(), Rs.end(), 0.0);
    HIP_TRY(h, h->rQ.once((size_t)n * n));
    HIP_TRY(h, h->rR.once((size_t)m * m));
    HIP_TRY(h, hipMemcpy(h->rQ, Qs.data(), Qs.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->rR, Rs.data(), Rs.size() * sizeof(double), hipMemcpyHostToDevice));
    if (Pshared) {
        HIP_TRY(h, h->rP.once((size_t)n * n));
        HIP_TRY(h, hipMemcpy(h->rP, Pshared, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
    }
    HIP_TRY(h, h->rKst.once((size_t)h->batch * h->N * ((size_t)n * m + m)));
    if ((size_t)h->batch * h->N * ((size_t)n * n + n) * sizeof(double) <= ((size_t)8 << 30))   // value functions of the last sweep
        HIP_TRY(h, h->rPst.once((size_t)h->batch * h->N * ((size_t)n * n + n)));
    return ALMPC_OK;
}

// LDS a workgroup can have on gfx950, in bytes (the stage-wise layer below sizes its launches by it)
constexpr int LDS_BUDGET = 160 * 1024;

bool riccati_shape_ok(const almpc_handle* h) {
    return h->n <= 32 && h->m <= 16 && (long)h->m * h->N <= 1024 && riccati_lds_doubles(h->n, h->m, h->N) * sizeof(double) <= LDS_BUDGET;
}

// Which instances a launch of the stage-wise solvers takes (the kernels compare the int: SdualParams::filter)
// ALL: the whole batch; UNSOLVED: the instances whose status is not 0 (the redo behind a condensed step); SQP_FLAGGED, SQP_ALL: the QP
// of the current SQP iteration, for the instances the condensed path flagged or left unsolved / for every instance
enum SolveFilter : int { FILTER_ALL = 0, FILTER_UNSOLVED = 1, FILTER_SQP_FLAGGED = 2, FILTER_SQP_ALL = 3 };

// One call of launch_riccati / launch_sgains / launch_sdual: the plain solve of the whole batch unless a field says otherwise.
// By value: a nested launch does not inherit it.
struct SolveCall {
    SolveFilter filter = FILTER_ALL;
    const double* guess = nullptr;   // inputs [batch][N][m] whose bounds seed the working set
    int max_iter = 0;                // cap of the working-set changes (0: the solver's own)
    bool x0_from_results = false;    // a deferred redo: x0 = stage 1 of the step's own x (the caller may have handed over the next x0 since)
    bool gated = false;              // enqueued behind the step: returns at once unless the step left an instance undecided (almpc_handle::Redo)
    bool predicted = false;          // a gated redo that is EXPECTED to have work (tier policy of a plain redo)
    // k_sdual only
    bool single_launch = false;      // one launch with room for 64 or 128 rows in place of the tiers (few instances: a redo)
    int first_tier = 0;              // 1: starts that are known to hold many rows skip the 32-row tier
    RowMultOut rows = {};            // the SQP loop's row multipliers
};

// Per-wave slices of LDS: as many waves per workgroup as fit the budget, at most `most`, at least one ...
int waves_in_lds(size_t per_wave, int most) {
    while (most > 1 && per_wave * most > LDS_BUDGET) --most;
    return most;
}
// ... and the workgroups that cover the batch with them, capped (a wave walks the instances beyond the cap)
int capped_grid(int batch, int waves, int cap) { return std::min((batch + waves - 1) / waves, cap); }
// A kernel on such slices: its limit of dynamic LDS raised to `lds` where need be, then the launch (a macro: the launch names the kernel)
#define LAUNCH_WAVES(KERNEL, wgs, waves, lds, st, p)                                          \
    [&]() -> hipError_t {                                                                     \
        const hipError_t e_ = ensure_dyn_lds(reinterpret_cast<const void*>(KERNEL), lds);     \
        if (e_ != hipSuccess) return e_;                                                      \
        hipLaunchKernelGGL(KERNEL, dim3(wgs), dim3(64 * (waves)), lds, st, p);                \
        return hipGetLastError();                                                             \
    }()

// k_riccati over the instances of call.filter, start = call.guess
hipError_t launch_riccati(almpc_handle* h, SolveCall call) {
    RiccatiParams rp;
    rp.n = h->n; rp.m = h->m; rp.N = h->N; rp.batch = h->batch;
    const bool pi = h->batched && !h->structured ? true : h->batched;
    rp.A = pi ? h->bA : h->dA; rp.A_stride = pi ? (long)h->n * h->n : 0;
    rp.B = pi ? h->bB : h->dB; rp.B_stride = pi ? (long)h->n * h->m : 0;
    rp.Q = h->rQ; rp.R = h->rR;
    rp.P = h->r_batched_P ? h->bP : h->rP; rp.P_stride = h->r_batched_P ? h->rP_stride : 0;
    if (!rp.Q || !rp.R || !rp.P || !h->rKst) return hipErrorInvalidValue;   // no riccati_weights() for this design: nothing to launch with
    rp.umin = h->dUmin; rp.umax = h->dUmax;
    rp.uref = h->dUref; rp.uref_stride = h->uref_stride; rp.xref = h->dXref; rp.xref_stride = h->xref_stride;
    rp.x0 = h->dX0; rp.x0_stride = h->n; rp.uguess = call.guess; rp.filter = call.filter; rp.Kst = h->rKst; rp.Pst = h->rPst;
    if (call.x0_from_results) { rp.x0 = h->dX; rp.x0_stride = (long)h->n * (h->N + 1); }
    if (call.gated) { rp.gate = h->redo.dGate; rp.gate_val = h->redo.step_serial; }
    rp.x = h->dX; rp.ex = h->dEx; rp.u = h->dU; rp.eu = h->dEu; rp.status = h->dStatus; rp.piters = h->dPiters;
    rp.max_iter = call.max_iter > 0 ? call.max_iter : 20 * h->N * h->m + 50;
    rp.tol = 1e-9;
    rp.lds_per_wave = riccati_lds_doubles(h->n, h->m, h->N);
    rp.A_kstride = 0; rp.B_kstride = 0; rp.c = nullptr; rp.c_stride = 0; rp.ebar = nullptr; rp.ebar_stride = 0;
    rp.qu = nullptr; rp.qu_stride = 0; rp.qu_scale = 1.0; rp.flag = nullptr; rp.v_only = 0;
    if (h->sqp.ready && call.filter >= FILTER_SQP_FLAGGED) {   // the QP of the current SQP iteration: stage models, defects, state errors, input gradient
        const almpc_handle::Sqp& q = h->sqp;
        const long n = h->n, m = h->m, N = h->N;
        rp.A = q.A; rp.A_stride = N * n * n; rp.A_kstride = n * n;
        rp.B = q.B; rp.B_stride = N * n * m; rp.B_kstride = n * m;
        rp.c = q.c; rp.c_stride = N * n; rp.ebar = q.ebar; rp.ebar_stride = N * n;
        rp.qu = q.qadd; rp.qu_stride = N * m; rp.qu_scale = 0.5;
        rp.P = h->bP; rp.P_stride = q.sP;
        rp.x0 = nullptr; rp.flag = h->bFlag; rp.v_only = 1;
    } else if (h->lsw.ready) {   // almpc_design_ltv_stagewise: the caller's stage models, k_ltv_stage_prepare's vectors; dx_0 = 0 (x0 = xbar_0)
        const almpc_handle::Lsw& l = h->lsw;
        const long n = h->n, m = h->m, N = h->N;
        rp.A = h->lA; rp.A_stride = N * n * n; rp.A_kstride = n * n;
        rp.B = h->lB; rp.B_stride = N * n * m; rp.B_kstride = n * m;
        rp.c = l.has_c ? h->lC.get() : nullptr; rp.c_stride = N * n; rp.ebar = l.ebar; rp.ebar_stride = N * n;
        rp.qu = l.qadd; rp.qu_stride = N * m; rp.qu_scale = 0.5;
        rp.P = h->bP; rp.P_stride = l.sP;
        rp.x0 = h->dXref; rp.x0_stride = n * (N + 1);
    }
    const size_t per = (size_t)rp.lds_per_wave * sizeof(double);
    const int waves = waves_in_lds(per, RICCATI_WAVES);
    const size_t lds = per * waves;
    if (lds > LDS_BUDGET) return hipErrorInvalidValue;
    const int wgs = capped_grid(h->batch, waves, h->num_cus * 2);
#define RICCATI_LAUNCH(NC_, MC_) return LAUNCH_WAVES((k_riccati_t<NC_, MC_>), wgs, waves, lds, h->stream, rp)
    if (h->n == 12 && h->m == 4 && !h->sw.riccati_generic) RICCATI_LAUNCH(12, 4);
    else if (h->n == 4 && h->m == 2 && !h->sw.riccati_generic) RICCATI_LAUNCH(4, 2);
    else if (h->n == 2 && h->m == 1 && !h->sw.riccati_generic) RICCATI_LAUNCH(2, 1);
    else RICCATI_LAUNCH(0, 0);
#undef RICCATI_LAUNCH
}

// ---- stage-wise dual active-set solve (k_sdual) ----------------------------------------------------------------------------
// instantiated (NT, MC): the smallest pair that covers (nt, m)
const int SD_SHAPES[][2] = {{2, 2}, {4, 2}, {6, 2}, {8, 4}, {12, 4}, {16, 4}, {16, 8}, {32, 16}, {48, 16}};
bool sdual_pick_shape(int nt, int m, int* NT, int* MC) {
    for (const auto& s : SD_SHAPES)
        if (nt <= s[0] && m <= s[1]) { *NT = s[0]; *MC = s[1]; return true; }
    return false;
}
constexpr int SD_WCAP1 = 32, SD_WCAP2 = 64, SD_WCAP3 = 96, SD_WCAP4 = 128;   // working-set capacity of the first launch / of the redos of the instances that outgrew it
bool sdual_shape_ok(int n, int m, int N, bool useS) {
    int NT = 0, MC = 0;
    if (!sdual_pick_shape(useS ? n + m : n, m, &NT, &MC)) return false;
    if ((N + 64 / (NT + MC)) / (64 / (NT + MC)) > 64) return false;   // (one bit per coordinate and lane in the working-set mask)
    return (size_t)sdual_lds_doubles(NT, MC, N, SD_WCAP2) * sizeof(double) <= LDS_BUDGET;
}

hipError_t sdual_build_ghat(almpc_handle* h);

// Front of the two set-ups below: whether there is an input-rate term, the size of the stage state and the instantiated shape for it
int sdual_setup_shape(almpc_handle* h, bool useS) {
    almpc_handle::Sd& sd = h->sd;
    sd.ready = false;
    sd.useS = useS;
    sd.nt = useS ? h->n + h->m : h->n;
    if (!sdual_pick_shape(sd.nt, h->m, &sd.NT, &sd.MC) || !sdual_shape_ok(h->n, h->m, h->N, useS))
        return fail(h, ALMPC_ERR_UNSUPPORTED, "stage-wise solve: n (+ m with an input-rate weight) <= 48, m <= 16 and (N + 1)(n + m) <= 4096");
    return ALMPC_OK;
}
// ... and their back: state box, terminal equality, the tiers' overflow words and saved working sets, S, no reference terms yet
int sdual_setup_rows(almpc_handle* h, const hm::mat* Sm, const double* xmin, const double* xmax, bool terminal_eq) {
    const int n = h->n;
    almpc_handle::Sd& sd = h->sd;
    sd.has_box = xmin != nullptr;
    if (sd.has_box) {
        HIP_TRY(h, sd.xmin.once((size_t)n));
        HIP_TRY(h, sd.xmax.once((size_t)n));
        HIP_TRY(h, hipMemcpy(sd.xmin, xmin, n * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(sd.xmax, xmax, n * sizeof(double), hipMemcpyHostToDevice));
    }
    sd.has_eq = terminal_eq;
    HIP_TRY(h, sd.ovf.once((size_t)h->batch + 2));   // (+ the tiers' gate word: SdualParams::ovf_gate)
    HIP_TRY(h, sd.wsave.once((size_t)h->batch * SDUAL_WSAVE));
    HIP_TRY(h, hipMemset(sd.ovf, 0, ((size_t)h->batch + 2) * sizeof(int32_t)));
    sd.S = Sm ? *Sm : hm::mat();
    sd.has_base = false; sd.base_stride = 0;
    return ALMPC_OK;
}

// Stage records of a SHARED model on the device (host Riccati, design time), state box / terminal equality / S of the design.
// Rm: the reference's branch rule applied (zeros when R[1,1] == 0); Sm null: no input-rate term.
int sdual_setup_shared(almpc_handle* h, const hm::mat& Am, const hm::mat& Bm, const hm::mat& Qm, const hm::mat& Rm, const hm::mat* Sm,
                       const hm::mat& Pm, const double* xmin, const double* xmax, bool terminal_eq) {
    const int n = h->n, m = h->m, N = h->N;
    almpc_handle::Sd& sd = h->sd;
    ALMPC_TRY(sdual_setup_shape(h, Sm != nullptr));
    hm::mat rec;
    bool inv = false;
    if (!hm::stage_records(Am, Bm, Qm, Rm, Sm, Pm, n, m, N, sd.NT, sd.MC, rec, inv))
        return fail(h, ALMPC_ERR_NUMERIC, "stage-wise solve: R + B'PB is singular (Riccati recursion of the unconstrained problem)");
    const size_t stage = (size_t)sdual_rec_stage(sd.NT, sd.MC);
    const size_t cnt = inv ? stage : stage * N;
    HIP_TRY(h, sd.rec.grow(cnt));
    HIP_TRY(h, hipMemcpy(sd.rec, rec.data() + (inv ? stage * (N - 1) : 0), cnt * sizeof(double), hipMemcpyHostToDevice));
    sd.rec_stride = 0;
    sd.rec_kstride = inv ? 0 : (long)stage;
    ALMPC_TRY(sdual_setup_rows(h, Sm, xmin, xmax, terminal_eq));
    sd.per_instance = false; sd.gain_N = 0; sd.sqp = false;
    sd.scr_ready = false;
    sd.ready = true;
    // cached responses (sdual_build_ghat): at design time for a structured handle, whose every step uses them; on a condensed handle,
    // where k_sdual is only the redo of what a step leaves undecided, at the first redo -- most such handles (the headline path) never
    // leave an instance undecided and should not pay TP^2 doubles and one sweep per coordinate at every design
    sd.ghat_ready = false;
    sd.ghat_wanted = !h->sw.sdual_no_ghat;
    if (sd.ghat_wanted && (h->flags & ALMPC_FLAG_STRUCTURED)) {
        HIP_TRY(h, sdual_build_ghat(h));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return ALMPC_OK;
}

// Linear cost terms of the stage-wise problem that depend on the references: only the input-rate term does (it is on u = v + u_ref,
// src/sub/design_mpc.jl:423-446): stage k >= 1 carries (w_k - v_k + dU)'S(w_k - v_k + dU), dU = u_ref[k-1] - u_ref[k]  ->
// +S dU on the coordinates of w_k = v_{k-1}, -S dU on those of v_k.  Zero for references that are constant over the horizon.
int sdual_update_base(almpc_handle* h, const double* uref, size_t cnt) {
    almpc_handle::Sd& sd = h->sd;
    sd.has_base = false; sd.base_stride = 0;
    sd.scr_ready = false;   // (the screen's interval table depends on the input reference)
    if (!sd.ready || !sd.useS) return ALMPC_OK;
    const int n = h->n, m = h->m, N = h->N, SP = sd.NT + sd.MC;
    const size_t TP = (size_t)sdual_tp(sd.NT, sd.MC, N), us = (size_t)h->nz;
    std::vector<double> base(cnt * TP, 0.0);
    bool any = false;
    for (size_t c = 0; c < cnt; ++c)
        for (int k = 1; k < N; ++k)
            for (int a = 0; a < m; ++a) {
                double sv = 0.0;
                for (int b = 0; b < m; ++b) sv += sd.S[(size_t)b * m + a] * (uref[c * us + (size_t)(k - 1) * m + b] - uref[c * us + (size_t)k * m + b]);
                if (sv != 0.0) any = true;
                base[c * TP + (size_t)k * SP + n + a] += sv;
                base[c * TP + (size_t)k * SP + sd.NT + a] -= sv;
            }
    if (!any) return ALMPC_OK;
    HIP_TRY(h, sd.base.grow(base.size()));
    HIP_TRY(h, hipMemcpy(sd.base, base.data(), base.size() * sizeof(double), hipMemcpyHostToDevice));
    sd.has_base = true;
    sd.base_stride = cnt > 1 ? (long)TP : 0;
    return ALMPC_OK;
}

// Weights and buffers of the stage-wise solve with a model PER INSTANCE (almpc_design_batched, the re-linearisation pipeline): the stage
// records come from k_sgains (launch_sgains) -- `invariant`: the terminal weight is every instance's own DARE solution and there is
// no input-rate weight, so one stage per instance suffices.  Rm: as given (the branch rule is applied here); Sm null: no rate term.
int sdual_setup_batched(almpc_handle* h, const hm::mat& Qm, const hm::mat& Rm, const hm::mat* Sm, bool invariant,
                        const double* xmin, const double* xmax, bool terminal_eq) {
    const int n = h->n, m = h->m, N = h->N;
    almpc_handle::Sd& sd = h->sd;
    ALMPC_TRY(sdual_setup_shape(h, Sm != nullptr));
    if ((size_t)sgains_lds_doubles(sd.nt, m) * sizeof(double) > LDS_BUDGET) return fail(h, ALMPC_ERR_UNSUPPORTED, "stage-wise solve: the gain recursion does not fit LDS");
    hm::mat Qs = Qm, Rs = Rm;
    if (Rm[0] == 0.0) std::fill(Rs.begin(), Rs.end(), 0.0);
    HIP_TRY(h, sd.dQ.once((size_t)n * n));
    HIP_TRY(h, sd.dR.once((size_t)m * m));
    HIP_TRY(h, hipMemcpy(sd.dQ, Qs.data(), Qs.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(sd.dR, Rs.data(), Rs.size() * sizeof(double), hipMemcpyHostToDevice));
    if (Sm) {
        HIP_TRY(h, sd.dS.once((size_t)m * m));
        HIP_TRY(h, hipMemcpy(sd.dS, Sm->data(), Sm->size() * sizeof(double), hipMemcpyHostToDevice));
    }
    const size_t stage = (size_t)sdual_rec_stage(sd.NT, sd.MC);
    sd.gain_N = invariant ? 1 : N;
    const size_t cnt = (size_t)h->batch * sd.gain_N * stage;
    HIP_TRY(h, sd.rec.grow(cnt));
    sd.rec_stride = (long)(sd.gain_N * stage);
    sd.rec_kstride = invariant ? 0 : (long)stage;
    sd.per_instance = true; sd.sqp = false;   // (scr_ready and the table flags keep what a shared design left: per_instance is asked before them)
    ALMPC_TRY(sdual_setup_rows(h, Sm, xmin, xmax, terminal_eq));
    HIP_TRY(h, sd.bad.once((size_t)h->batch));
    HIP_TRY(h, hipMemset(sd.bad, 0, (size_t)h->batch * sizeof(int)));
    sd.ready = true;
    return ALMPC_OK;
}

// k_dare: P_i = DARE(A_i, B_i, Q, R) of p.batch models, one wave per instance (csrc/almpc_dare.hip.h).  Launch only.
hipError_t launch_dare(DareParams p, hipStream_t st) {
    p.lds_per_wave = dare_lds_doubles(p.n, p.m);
    const int waves = dare_waves(p.n, p.m), d = p.n > p.m ? p.n : p.m;
    const size_t lds = (size_t)p.lds_per_wave * sizeof(double) * waves;
    const int wgs = (p.batch + waves - 1) / waves;
#define DARE_RL(RL_) return LAUNCH_WAVES((k_dare<RL_>), wgs, waves, lds, st, p)
    if (d <= 16) DARE_RL(16);
    else if (d <= 32) DARE_RL(32);
    else DARE_RL(64);
#undef DARE_RL
}

// k_dare_vjp: the adjoint of P_i = DARE(A_i, B_i, Q, R), one wave per instance (csrc/almpc_dare_vjp.hip.h).  Launch only.
hipError_t launch_dare_vjp(DareVjpParams p, hipStream_t st) {
    p.lds_per_wave = dare_lds_doubles(p.n, p.m);
    const int waves = dare_waves(p.n, p.m), d = p.n > p.m ? p.n : p.m;
    const size_t lds = (size_t)waves * p.lds_per_wave * sizeof(double);
    const unsigned wgs = (unsigned)((p.batch + waves - 1) / waves);
#define DARE_VJP_RL(RL_) return LAUNCH_WAVES((k_dare_vjp<RL_>), wgs, waves, lds, st, p)
    if (d <= 16) DARE_VJP_RL(16);
    else if (d <= 32) DARE_VJP_RL(32);
    else DARE_VJP_RL(64);
#undef DARE_VJP_RL
}

// What k_dare cannot be given: a shape beyond its LDS layout, or an R that hm::dare refuses (singular), or R[1,1] == 0 -- the
// reference's branch rule then drops R from the cost and no DARE is left.  ALMPC_OK, or the error code with *why set.
int dare_device_check(int n, int m, const hm::mat& Rm, bool branch_rule, const char** why) {
    if (n > DARE_MAX_N || m > DARE_MAX_M) { *why = "DARE on the device: n <= 48 and m <= 16 (k_dare)"; return ALMPC_ERR_UNSUPPORTED; }
    if (branch_rule && Rm[0] == 0.0) { *why = "DARE on the device: R[1,1] == 0 drops R from the cost, the equation is singular"; return ALMPC_ERR_NUMERIC; }
    hm::mat I = hm::eye(m);
    if (!hm::lu_solve(Rm, I, m, m)) { *why = "DARE on the device: R is singular"; return ALMPC_ERR_NUMERIC; }
    return ALMPC_OK;
}

// almpc_set_terminal_weight(ALMPC_TERMINAL_DARE_DEVICE), almpc_design_batched(P = NULL): bP_i = DARE(bA_i, bB_i, Q, R) by k_dare on
// the handle's stream, behind the uploads of the models and weights (dQ, dR: device).  Waits for it and reports the first instance
// without a stabilising solution as the host loop does.  Pfirst: host copy of instance 0's weight.
// sQ, sR: strides of dQ, dR (0: shared; almpc_design_batched_weighted: one pair per instance -- Rm is then instance 0's, and a singular
// R_i of another instance is k_dare's own status 1, reported like an instance without a stabilising solution)
int design_dare_device(almpc_handle* h, const double* dQ, const double* dR, const hm::mat& Rm, hm::mat& Pfirst, long sQ = 0, long sR = 0) {
    const int n = h->n, m = h->m;
    const size_t b = (size_t)h->batch;
    const char* why = "";
    if (const int bad = dare_device_check(n, m, Rm, true, &why)) return fail(h, bad, std::string("design_batched: ") + why);
    HIP_TRY(h, h->tStat.once(b));
    DareParams dp;
    dp.n = n; dp.m = m; dp.batch = h->batch;
    dp.A = h->bA; dp.A_stride = (long)n * n; dp.B = h->bB; dp.B_stride = (long)n * m; dp.Q = dQ; dp.R = dR;
    dp.Q_stride = sQ; dp.R_stride = sR;
    dp.P = h->bP; dp.P_stride = (long)n * n; dp.fallback = nullptr; dp.status = h->tStat; dp.lds_per_wave = 0;
    HIP_TRY(h, launch_dare(dp, h->stream));
    std::vector<int32_t> stt(b, 0);
    HIP_TRY(h, hipMemcpyAsync(stt.data(), h->tStat, b * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < b; ++i)
        if (stt[i] != 0) return fail(h, ALMPC_ERR_NUMERIC, "design_batched: DARE did not converge for instance " + std::to_string(i));
    Pfirst.resize((size_t)n * n);
    HIP_TRY(h, hipMemcpy(Pfirst.data(), h->bP, Pfirst.size() * sizeof(double), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

// The re-linearisation pipeline with the mode on, setup: the checks, the setup's P in a buffer of its own and the status words
int relin_terminal_setup(almpc_handle* h, const hm::mat& Rm, const hm::mat& Pm) {
    h->t_step = false;
    if (h->terminal_mode != ALMPC_TERMINAL_DARE_DEVICE) return ALMPC_OK;
    const char* why = "";
    if (const int bad = dare_device_check(h->n, h->m, Rm, true, &why)) return fail(h, bad, std::string("relin_fnn_setup: ") + why);
    HIP_TRY(h, h->tP.upload(Pm.data(), Pm.size()));
    HIP_TRY(h, h->tStat.once((size_t)h->batch));
    HIP_TRY(h, hipMemset(h->tStat, 0, (size_t)h->batch * sizeof(int32_t)));
    h->t_step = true;
    return ALMPC_OK;
}
// ... and step: bP_i = DARE(bA_i, bB_i, Q, R) of the step's Jacobians, the setup's P where there is none.  Launch only.
hipError_t launch_relin_dare(almpc_handle* h, const double* dQ, const double* dR) {
    const int n = h->n, m = h->m;
    DareParams dp;
    dp.n = n; dp.m = m; dp.batch = h->batch;
    dp.A = h->bA; dp.A_stride = (long)n * n; dp.B = h->bB; dp.B_stride = (long)n * m; dp.Q = dQ; dp.R = dR;
    dp.P = h->bP; dp.P_stride = (long)n * n; dp.fallback = h->tP; dp.status = h->tStat; dp.lds_per_wave = 0;
    return launch_dare(dp, h->stream);
}

// k_c2d: (Ad_i, Bd_i) = zero-order hold of (Ac_i, Bc_i) at p.Ts, one wave per instance (csrc/almpc_c2d.hip.h).  Launch only.
hipError_t launch_c2d(C2dParams p, hipStream_t st) {
    p.lds_per_wave = c2d_lds_doubles(p.n, p.m);
    const int waves = c2d_waves(p.n, p.m);
    const size_t lds = (size_t)p.lds_per_wave * sizeof(double) * waves;
    const int wgs = (p.batch + waves - 1) / waves;
#define C2D_RL(RL_) return LAUNCH_WAVES((k_c2d<RL_>), wgs, waves, lds, st, p)
    if (p.n <= 16) C2D_RL(16);
    else if (p.n <= 32) C2D_RL(32);
    else C2D_RL(64);
#undef C2D_RL
}

bool model_continuous(const almpc_handle* h) { return h->model_mode == ALMPC_MODEL_CONTINUOUS_ZOH; }

// almpc_set_model_time(ALMPC_MODEL_CONTINUOUS_ZOH): the handle's per-instance model slots bA, bB hold continuous-time models; one
// k_c2d launch on the handle's stream turns them into the discrete ones in place.  Launch only; poison: a failing instance's slots
// are filled with NaN (re-linearisation step) instead of being left alone.
hipError_t launch_model_c2d(almpc_handle* h, bool poison) {
    const int n = h->n, m = h->m;
    C2dParams cp;
    cp.n = n; cp.m = m; cp.batch = h->batch;
    cp.Ac = h->bA; cp.A_stride = (long)n * n; cp.Bc = h->bB; cp.B_stride = (long)n * m; cp.Ts = h->model_Ts;
    cp.Ad = h->bA; cp.Bd = h->bB; cp.poison = poison ? 1 : 0; cp.status = h->cStat; cp.lds_per_wave = 0;
    return launch_c2d(cp, h->stream);
}
int c2d_shape_check(almpc_handle* h, const char* who) {
    if (h->n > C2D_MAX_N || h->m > C2D_MAX_M) return fail(h, ALMPC_ERR_UNSUPPORTED, std::string(who) + ": continuous-time models on the device: n <= 64 and m <= 16 (k_c2d)");
    return ALMPC_OK;
}
// ... almpc_design_batched: behind the uploads of the models, in front of everything that reads them.  Waits for it and reports the
// first instance whose discretisation failed.
int design_c2d_device(almpc_handle* h) {
    const size_t b = (size_t)h->batch;
    HIP_TRY(h, h->cStat.once(b));
    HIP_TRY(h, launch_model_c2d(h, false));
    std::vector<int32_t> stt(b, 0);
    HIP_TRY(h, hipMemcpyAsync(stt.data(), h->cStat, b * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < b; ++i)
        if (stt[i] != 0) return fail(h, ALMPC_ERR_NUMERIC, "design_batched: discretisation failed for instance " + std::to_string(i));
    return ALMPC_OK;
}
// ... almpc_relin_*_setup: the shape check and the status words
int relin_c2d_setup(almpc_handle* h) {
    h->c_step = false;
    if (!model_continuous(h)) return ALMPC_OK;
    ALMPC_TRY(c2d_shape_check(h, "relin_fnn_setup"));
    HIP_TRY(h, h->cStat.once((size_t)h->batch));
    HIP_TRY(h, hipMemset(h->cStat, 0, (size_t)h->batch * sizeof(int32_t)));
    h->c_step = true;
    return ALMPC_OK;
}
// P_i = DARE of the zero-order hold of (A_i, B_i) (host loop of almpc_design_batched(P = NULL) with continuous-time models)
bool host_dare_of(const almpc_handle* h, hm::mat Am, hm::mat Bm, const hm::mat& Qm, const hm::mat& Rm, hm::mat& Pm, const char** what) {
    *what = "DARE did not converge";
    if (model_continuous(h)) {
        hm::mat Ad, Bd;
        if (hm::c2d(Am, Bm, h->model_Ts, h->n, h->m, Ad, Bd) != 0) { *what = "discretisation failed"; return false; }
        Am.swap(Ad); Bm.swap(Bd);
    }
    return hm::dare(Am, Bm, Qm, Rm, h->n, h->m, Pm);
}

// k_sgains over the handle's per-instance models (bA, bB; terminal weights bP, shared or per instance): the instances of call.filter
hipError_t launch_sgains(almpc_handle* h, SolveCall call = {}) {
    const almpc_handle::Sd& sd = h->sd;
    SgainsParams gp;
    std::memset(&gp, 0, sizeof(gp));
    const long n = h->n, m = h->m;
    gp.n = h->n; gp.nt = sd.nt; gp.m = h->m; gp.N = sd.gain_N; gp.batch = h->batch; gp.NT = sd.NT; gp.MC = sd.MC;
    gp.A = h->bA; gp.A_stride = n * n; gp.A_kstride = 0;
    gp.B = h->bB; gp.B_stride = n * m; gp.B_kstride = 0;
    gp.P = h->bP; gp.P_stride = h->rP_stride;   // (one matrix with stride 0, or one per instance)
    gp.Q = sd.dQ; gp.R = sd.dR; gp.S = sd.useS ? sd.dS : nullptr;
    gp.filter = call.filter; gp.status = h->dStatus;
    gp.rec = sd.rec; gp.rec_stride = sd.rec_stride;
    gp.bad = sd.bad;
    if (call.gated) { gp.gate = h->redo.dGate; gp.gate_val = h->redo.step_serial; }
    if (sd.sqp) {   // the QP of the current SQP iteration: stage models, defects, state errors and input gradient of the loop
        const almpc_handle::Sqp& q = h->sqp;
        const long N = h->N;
        gp.A = q.A; gp.A_stride = N * n * n; gp.A_kstride = n * n;
        gp.B = q.B; gp.B_stride = N * n * m; gp.B_kstride = n * m;
        gp.P = h->bP; gp.P_stride = q.sP;
        gp.c = q.c; gp.c_stride = N * n;
        gp.pc = sd.pc; gp.ct = sd.ct; gp.pc_stride = N * sd.NT;
        gp.ebar = q.ebar; gp.ebar_stride = N * n; gp.qadd = q.qadd; gp.qadd_stride = N * m; gp.qscale = 0.5;
        gp.base = sd.base; gp.base_stride = sd.base_stride;
        gp.flag = h->bFlag;
    } else if (h->lsw.ready) {   // almpc_design_ltv_stagewise: the caller's stage models and defects, k_ltv_stage_prepare's cost terms
        const almpc_handle::Lsw& l = h->lsw;
        const long N = h->N;
        gp.A = h->lA; gp.A_stride = N * n * n; gp.A_kstride = n * n;
        gp.B = h->lB; gp.B_stride = N * n * m; gp.B_kstride = n * m;
        gp.P = h->bP; gp.P_stride = l.sP;
        if (l.has_c) { gp.c = h->lC; gp.c_stride = N * n; gp.pc = sd.pc; gp.ct = sd.ct; gp.pc_stride = N * sd.NT; }
        gp.ebar = l.ebar; gp.ebar_stride = N * n; gp.qadd = l.qadd; gp.qadd_stride = N * m; gp.qscale = 0.5;
        gp.base = sd.base; gp.base_stride = sd.base_stride;
    }
    if (!gp.A || !gp.B || !gp.P || !gp.rec) return hipErrorInvalidValue;
    gp.lds_per_wave = sgains_lds_doubles(sd.nt, h->m);
    const size_t per = (size_t)gp.lds_per_wave * sizeof(double);
    const int waves = waves_in_lds(per, SGAINS_WAVES);
    const size_t lds = per * waves;
    const int wgs = capped_grid(h->batch, waves, h->num_cus * 2);
    return LAUNCH_WAVES((k_sgains), wgs, waves, lds, h->stream, gp);
}

// Sinv of SD_WCAP4 rows fits LDS beside the trajectories (else: the global-scratch build)
bool sdual_fits128(int NT, int MC, int N) { return (size_t)sdual_lds_doubles(NT, MC, N, SD_WCAP4, true) * sizeof(double) <= LDS_BUDGET; }

struct SdualTiers { int first, last; };

template <int NT, int MC>
hipError_t launch_sdual_t(almpc_handle* h, SdualParams sp, SdualTiers tiers) {
    // tier 0: every (filtered) instance with room for SD_WCAP1 rows (several waves per workgroup); tier 1: the instances that outgrew it,
    // SD_WCAP2 rows; tier 2: SD_WCAP4 rows, two working-set positions per lane (mostly infeasible instances whose verdict needs that
    // many rows); tier 3: the same with Sinv in a global scratch, for shapes whose trajectories leave no room for it in LDS.
    // (first = last = 1: ONE launch with room for SD_WCAP2 rows -- the redo of the few instances a condensed step left unsolved)
    if (tiers.last > tiers.first && sp.wsave && !h->sw.sdual_no_sinv_handover) {   // tiers hand each other the inverse of their working set
        const hipError_t e_ = h->sd.sinv_save.once((size_t)h->batch * sdual_sinv_doubles(SDUAL_SINV_SAVE));
        if (e_ != hipSuccess) return e_;
        sp.sinv_save = h->sd.sinv_save;
    }
    // the later tiers return at once unless an earlier one of THIS call ran out of room (it stores the call's number in the gate word):
    // their scan for flagged instances alone is 16 dependent loads per wave, 9 us of an idle launch on 4096 instances
    if (sp.ovf) { sp.ovf_gate = sp.ovf + sp.batch; sp.ovf_gate_val = ++h->sd.tier_serial; }
    const bool fits128 = sdual_fits128(NT, MC, sp.N);
    for (int tier = tiers.first; tier <= tiers.last; ++tier) {
        sp.wcap = tier == 0 ? SD_WCAP1 : (tier == 1 ? SD_WCAP2 : SD_WCAP4);
        sp.only_ovf = tier > tiers.first;
        const bool glb = tier == 3;
        if (tier == 2 && !fits128) continue;   // (Sinv of 128 rows does not fit beside the trajectories: the global-scratch build)
        if (tier == 3 && fits128) continue;
        sp.lds_per_wave = sdual_lds_doubles(NT, MC, sp.N, sp.wcap, !glb);
        const size_t per = (size_t)sp.lds_per_wave * sizeof(double);
        const int waves = waves_in_lds(per, tier >= 1 ? 1 : SDUAL_WAVES);   // (the later tiers' few instances: spread over the compute units)
        const size_t lds = per * waves;
        if (lds > LDS_BUDGET) return hipErrorInvalidValue;
        const int per_cu = std::max(1, std::min((int)(LDS_BUDGET / lds), 8 / waves));   // (at most 8 waves on a compute unit)
        const int wgs = capped_grid(sp.batch, waves, glb ? h->num_cus : h->num_cus * per_cu);
        const size_t lds_gh = lds + (size_t)(NT + MC) * (sdual_rec_row(NT, MC) + 2) * sizeof(double);   // (+ the workgroup's copy of a stage-invariant record, rows padded)
        // cached responses: the build whose sweeps fetch their records stage by stage and whose column stream runs four times deeper (see k_sdual)
        const bool gh = sp.ghat != nullptr && lds_gh <= LDS_BUDGET && !h->sw.sdual_no_gh;
        hipError_t e;
        if (tier < 2)
            e = gh ? LAUNCH_WAVES((k_sdual<NT, MC, 1, false, true>), wgs, waves, lds_gh, h->stream, sp) : LAUNCH_WAVES((k_sdual<NT, MC, 1, false, false>), wgs, waves, lds, h->stream, sp);
        else if (!glb)
            e = gh ? LAUNCH_WAVES((k_sdual<NT, MC, 2, false, true>), wgs, waves, lds_gh, h->stream, sp) : LAUNCH_WAVES((k_sdual<NT, MC, 2, false, false>), wgs, waves, lds, h->stream, sp);
        else {
            sp.ghat = nullptr;   // (the global-scratch build has no cached-response variant: sweeps)
            if ((e = h->sd.sinv_glb.grow((size_t)wgs * waves * sdual_sinv_doubles(SD_WCAP4))) != hipSuccess) return e;
            sp.sinv_glb = h->sd.sinv_glb;
            e = LAUNCH_WAVES((k_sdual<NT, MC, 2, true>), wgs, waves, lds, h->stream, sp);
        }
        if (e != hipSuccess) return e;
        sp.filter = 0;   // the later tiers select by the overflow flag alone (the first one has rewritten the statuses)
    }
    return hipSuccess;
}

hipError_t launch_sdual_shape(almpc_handle* h, const SdualParams& sp, SdualTiers tiers) {
#define SD_CASE(NT_, MC_) if (h->sd.NT == NT_ && h->sd.MC == MC_) return launch_sdual_t<NT_, MC_>(h, sp, tiers)
    SD_CASE(2, 2); SD_CASE(4, 2); SD_CASE(6, 2); SD_CASE(8, 4); SD_CASE(12, 4); SD_CASE(16, 4); SD_CASE(16, 8); SD_CASE(32, 16); SD_CASE(48, 16);
#undef SD_CASE
    return hipErrorInvalidValue;
}

// SdualParams of the handle's design, zero but for what the design fixes: shape, stage records, state box, the solver's own cap
SdualParams sdual_design_params(const almpc_handle* h) {
    const almpc_handle::Sd& sd = h->sd;
    SdualParams sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.n = h->n; sp.nt = sd.nt; sp.m = h->m; sp.N = h->N;
    sp.rec = sd.rec; sp.rec_stride = sd.rec_stride; sp.rec_kstride = sd.rec_kstride;
    sp.xmin = sd.has_box ? sd.xmin : nullptr; sp.xmax = sd.has_box ? sd.xmax : nullptr;
    sp.rows_state = (sd.has_box || sd.has_eq) ? 1 : 0;
    sp.max_iter = 20 * (h->N * h->m + (sp.rows_state ? h->N * h->n : 0)) + 50;
    sp.tol = 1e-9;
    return sp;
}

// Cached responses of a shared model: every coordinate that can be a row, one sweep each, once (k_sdual's build mode on
// min(TP, 2048) waves), TP x TP doubles.  Memory cap 256 MB per handle (TP <= 5792: e.g. the quadrotor with S up to N = 361); above it
// the table is not built and a working-set change costs two sweeps again (SdualParams::ghat == null).  Enqueued on the handle's stream.
// A launcher of its own with no SolveCall: the build is never gated, never screened and never started from a working set.
hipError_t sdual_build_ghat(almpc_handle* h) {
    almpc_handle::Sd& sd = h->sd;
    sd.ghat_wanted = false;   // (one attempt per design)
    const size_t TP = (size_t)sdual_tp(sd.NT, sd.MC, h->N);
    if (TP * TP * sizeof(double) > ((size_t)256 << 20)) return hipSuccess;
    hipError_t e;
    if ((e = sd.ghat.grow(TP * TP)) != hipSuccess || (e = hipMemsetAsync(sd.ghat, 0, TP * TP * sizeof(double), h->stream)) != hipSuccess) return e;
    SdualParams sp = sdual_design_params(h);   // + what else the build reads: the waves walk the coordinates, no instance data
    sp.batch = TP < 2048 ? (int)TP : 2048;
    sp.umin = sd.rec; sp.umax = sd.rec; sp.uref = sd.rec;   // (read into the bound tables, not used: the handle's own arrays may not exist yet)
    sp.eqt = sd.has_eq ? sd.rec : nullptr;   // (has_eq decides which coordinates can be rows; the target values are not used)
    sp.x0_stride = h->n; sp.base_stride = sd.base_stride;   // (not read without x0 and base: as every launch before had them)
    sp.build_ghat = 1; sp.ghat_out = sd.ghat;
    e = launch_sdual_shape(h, sp, {0, 0});   // (one launch, SD_WCAP1 rows of LDS: the build holds no working set)
    sd.ghat_ready = e == hipSuccess;
    return e;
}

// SdualParams of a solve: the handle's problem, the call's selection and start, and over them the QP of the current SQP iteration
SdualParams sdual_solve_params(const almpc_handle* h, const SolveCall& call) {
    const almpc_handle::Sd& sd = h->sd;
    SdualParams sp = sdual_design_params(h);
    sp.batch = h->batch;
    sp.base = sd.has_base ? sd.base : nullptr; sp.base_stride = sd.base_stride;
    sp.umin = h->dUmin; sp.umax = h->dUmax; sp.uref = h->dUref; sp.uref_stride = h->uref_stride;
    sp.xbref = h->dXref; sp.xbref_stride = h->xref_stride;
    sp.eqt = sd.has_eq && h->dXref ? h->dXref + (size_t)h->N * h->n : nullptr; sp.eqt_stride = h->xref_stride;   // x_N = x_ref_N
    sp.x0 = h->dX0; sp.x0_stride = h->n; sp.xref = h->dXref; sp.xref_stride = h->xref_stride;
    if (call.x0_from_results) { sp.x0 = h->dX; sp.x0_stride = (long)h->n * (h->N + 1); }
    if (call.gated) { sp.gate = h->redo.dGate; sp.gate_val = h->redo.step_serial; }
    sp.uguess = call.guess; sp.filter = call.filter;
    if (call.filter == FILTER_UNSOLVED && sd.start_ws && sd.start_ws_fresh && !sd.sqp) sp.start_ws = sd.start_ws;   // (the redo behind a state-row finish)
    sp.x = h->dX; sp.ex = h->dEx; sp.u = h->dU; sp.eu = h->dEu; sp.status = h->dStatus; sp.piters = h->dPiters;
    if (sd.sqp) {   // dx_0 = 0, variable v = u - ubar (the handle's per-instance references ARE the iterate xbar, ubar), cost terms per instance
        const almpc_handle::Sqp& q = h->sqp;
        sp.base = sd.base; sp.base_stride = sd.base_stride;
        sp.pc = sd.pc; sp.ct = sd.ct; sp.pc_stride = (long)h->N * sd.NT;
        sp.eqt = sd.has_eq ? q.xref + (size_t)h->N * h->n : nullptr; sp.eqt_stride = 0;
        sp.x0 = nullptr; sp.xref = nullptr; sp.xref_stride = 0;
        sp.flag = h->bFlag; sp.v_only = 1;
        sp.rows = call.rows;
    } else if (h->lsw.ready) {   // almpc_design_ltv_stagewise: dx_0 = 0, v = u - ubar, the references ARE the caller's trajectory; all outputs
        const almpc_handle::Lsw& l = h->lsw;
        sp.base = sd.base; sp.base_stride = sd.base_stride;
        if (l.has_c) { sp.pc = sd.pc; sp.ct = sd.ct; sp.pc_stride = (long)h->N * sd.NT; }
        sp.eqt = sd.has_eq ? l.eqt.get() : nullptr; sp.eqt_stride = 0;
        sp.x0 = nullptr;
    }
    sp.ovf = sd.ovf; sp.wsave = sd.wsave;
    sp.gbad = sd.per_instance ? sd.bad : nullptr;
    sp.ghat = (sd.ghat_ready && !sd.per_instance && !sd.sqp && sd.rec_stride == 0) ? sd.ghat : nullptr;
    if (call.max_iter > 0) sp.max_iter = call.max_iter;
    return sp;
}

// State box of a shared model with shared references, every instance solved from scratch: the reachability screen in front of the
// solve (one table kernel per design / reference change, one small launch per solve) -- instances it certifies infeasible never reach
// a sweep.  The verdicts [batch], or null: no screen for this call (or *err).
const int32_t* launch_sdual_screen(almpc_handle* h, const SolveCall& call, const double* x0, long x0_stride, hipError_t* err) {
    almpc_handle::Sd& sd = h->sd;
    if (!sd.has_box || sd.per_instance || sd.sqp || call.filter != FILTER_ALL || call.first_tier != 0 || !x0 || h->uref_stride != 0 ||
        h->xref_stride != 0 || !h->dA || !h->dB || h->sw.sdual_no_screen) return nullptr;
    const size_t n = (size_t)h->n, m = (size_t)h->m, N = (size_t)h->N;
    hipError_t& e = *err;
    if (sd.scr_phi.size() < N * n * n || sd.scr_g.size() < N * n * m || sd.scr_rm.size() < N * n || sd.scr_rp.size() < N * n)
        sd.scr_ready = false;   // (a table is made or replaced below)
    if ((e = sd.scr_phi.grow(N * n * n)) != hipSuccess || (e = sd.scr_g.grow(N * n * m)) != hipSuccess ||
        (e = sd.scr_rm.grow(N * n)) != hipSuccess || (e = sd.scr_rp.grow(N * n)) != hipSuccess ||
        (e = sd.scr_verdict.once((size_t)h->batch)) != hipSuccess) return nullptr;
    ScreenParams cp;
    cp.n = h->n; cp.m = h->m; cp.N = h->N; cp.batch = h->batch;
    cp.A = h->dA; cp.B = h->dB; cp.umin = h->dUmin; cp.umax = h->dUmax; cp.uref = h->dUref;
    cp.xmin = sd.xmin; cp.xmax = sd.xmax; cp.xref = h->dXref; cp.x0 = x0; cp.x0_stride = x0_stride;
    cp.phi = sd.scr_phi; cp.gtab = sd.scr_g; cp.rm = sd.scr_rm; cp.rp = sd.scr_rp; cp.verdict = sd.scr_verdict;
    if (!sd.scr_ready) {
        hipLaunchKernelGGL(k_screen_tables, dim3(1), dim3(256), 0, h->stream, cp);
        if ((e = hipGetLastError()) != hipSuccess) return nullptr;
        sd.scr_ready = true;
    }
    if ((e = hipMemsetAsync(sd.scr_verdict, 0, (size_t)h->batch * sizeof(int32_t), h->stream)) != hipSuccess) return nullptr;
    const dim3 sg((unsigned)((h->batch + 63) / 64), (unsigned)h->N);
#define SCR_CASE(NT_) if (h->n <= NT_) hipLaunchKernelGGL((k_state_box_screen<NT_>), sg, dim3(64), 0, h->stream, cp)
    SCR_CASE(4); else SCR_CASE(8); else SCR_CASE(12); else SCR_CASE(16); else SCR_CASE(32); else SCR_CASE(48); else e = hipErrorInvalidValue;
#undef SCR_CASE
    if (e == hipSuccess) e = hipGetLastError();
    return e == hipSuccess ? sd.scr_verdict.get() : nullptr;
}

// Which tiers of launch_sdual_t a solve runs.  The tiers from call.first_tier on (1: starts that are known to hold many rows), or
// for call.single_launch (the redo behind a condensed step: few instances, occupancy does not matter): the 128-row build when its
// Sinv fits LDS beside the trajectories, else the 64-row one.
SdualTiers sdual_tiers(const SolveCall& call, bool fits128, const Switches& sw) {
    if (!call.single_launch) return {call.first_tier, 3};
    // (round 5: the 64-row build first -- one working-set position per lane: its Sinv products, borderings and column streams are
    // cheaper per change than the 128-row build's -- and the 128-row build only for what outgrows it, which costs little since the
    // tiers hand over their inverse; ALMPC_SDUAL_REDO_128=1: the one 128-row launch of round 4)
    const bool one_launch = sw.sdual_redo_128 || (call.gated && !call.predicted);   // (a gated redo that is not expected to have work: one launch)
    return {fits128 && one_launch ? 2 : 1, fits128 ? 2 : 1};
}

// The redo's start (the finish's working set + the terminal-equality rows) with its inverse, built in registers from the cached
// responses before the solve: k_sdual_start (csrc/almpc_sdual.hip.h).  Sets sp.start_inv when it ran.
hipError_t launch_sdual_start(almpc_handle* h, SdualParams& sp, SdualTiers tiers) {
    almpc_handle::Sd& sd = h->sd;
    if (!sp.start_ws || !sp.ghat || tiers.first < 1 || h->sw.sdual_no_start_build) return hipSuccess;
    const hipError_t ea = sd.start_inv.once((size_t)h->batch * sdual_sinv_doubles(SDUAL_SINV_SAVE));
    if (ea != hipSuccess) return ea;
    SdualStartParams tp;
    std::memset(&tp, 0, sizeof(tp));
    tp.batch = h->batch; tp.n = h->n; tp.N = h->N; tp.SP = sd.NT + sd.MC; tp.TP = sdual_tp(sd.NT, sd.MC, h->N);
    // (the list is built for the LARGEST tier of this call: the first tier installs it if it leaves room to work, else hands it on)
    tp.wcap = (tiers.first == 1 && tiers.last < 2) ? SD_WCAP2 : SD_WCAP4; tp.has_eq = sd.has_eq ? 1 : 0;
    tp.status = h->dStatus; tp.gate = sp.gate; tp.gate_val = sp.gate_val;
    tp.ghat = sp.ghat; tp.start_ws = sd.start_ws; tp.start_inv = sd.start_inv;
    // (one workgroup per instance at a time; a workgroup looks at up to 64 SDUAL_START_WAVES instances)
    const int wmin = (h->batch + 64 * SDUAL_START_WAVES - 1) / (64 * SDUAL_START_WAVES);
    const int wgs = std::max(std::min(h->batch, h->num_cus * 4), wmin);
    hipLaunchKernelGGL(k_sdual_start, dim3(wgs), dim3(64 * SDUAL_START_WAVES), 0, h->stream, tp);
    sp.start_inv = sd.start_inv;
    return hipGetLastError();
}

// k_sdual over the instances of call.filter, start = call.guess: the cached responses at the first use on a condensed handle, the
// reachability screen, the redo's start, then the tiers of the handle's (NT, MC)
hipError_t launch_sdual(almpc_handle* h, SolveCall call) {
    almpc_handle::Sd& sd = h->sd;
    if (!sd.ready) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (sd.ghat_wanted && !sd.ghat_ready && !sd.per_instance && !sd.sqp && (e = sdual_build_ghat(h)) != hipSuccess) return e;
    SdualParams sp = sdual_solve_params(h, call);
    sp.screen = launch_sdual_screen(h, call, sp.x0, sp.x0_stride, &e);
    if (e != hipSuccess) return e;
    const SdualTiers tiers = sdual_tiers(call, sdual_fits128(sd.NT, sd.MC, h->N), h->sw);
    if ((e = launch_sdual_start(h, sp, tiers)) != hipSuccess) return e;
    return launch_sdual_shape(h, sp, tiers);
}

// Wait for the handle's stream: poll for a while before the blocking wait, whose wake-up (interrupt + scheduler) costs 0.1 - 15 ms on
// this pool -- more than the kernels waited for.
hipError_t stream_wait_polling(almpc_handle* h) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(h->stream);
        if (q != hipErrorNotReady) return q;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
    }
    return hipStreamSynchronize(h->stream);
}

// The primal Riccati active set can redo this design: an input box alone, no input-rate weight, riccati_weights() done
bool primal_redo_ready(const almpc_handle* h) { return h->mc == 0 && !h->kept.useS && h->rKst; }

// The redo of the instances a condensed step left undecided, from the step's own result: k_sdual (behind k_sgains for per-instance
// models, whose last step's models are still in the model slots) and / or k_riccati, as the caller says and the design allows.
//   caller               dual   primal           why
//   resolve_lazy_redo    yes    yes, behind it   the primal method takes what the dual one left without a certificate
//   enqueue_gated_redo   else   if ready         ONE of the two: an empty gated launch still costs 3 - 4 us of stream time
//   step_redo (eager)    yes    yes, behind it   as the lazy look; ALMPC_DBG_NO_SDUAL_FB / ALMPC_DBG_NO_PRIMAL_NET take one out
int launch_redo(almpc_handle* h, SolveCall call, bool dual, bool primal) {
    call.filter = FILTER_UNSOLVED; call.guess = h->dU; call.single_launch = true;
    if (dual && h->sd.ready) {
        if (h->sd.per_instance) HIP_TRY(h, launch_sgains(h, call));
        HIP_TRY(h, launch_sdual(h, call));
    }
    if (primal && primal_redo_ready(h)) HIP_TRY(h, launch_riccati(h, call));
    return ALMPC_OK;
}

// Lazy redo (see almpc_handle::Redo): called where the host is about to look at results and the stream is idle.  If the finish of
// a step since the last look left instances unsolved, the stage-wise solvers redo them now (from the step's own result).
int resolve_lazy_redo(almpc_handle* h) {
    almpc_handle::Redo& r = h->redo;
    if (!r.lazy_pending) return ALMPC_OK;
    r.lazy_pending = false;
    if (!r.hUnsolved) return ALMPC_OK;
    const int cur = *reinterpret_cast<volatile int*>(r.hUnsolved.get());
    r.expected = cur != r.unsolved_seen;
    if (cur == r.unsolved_seen) return ALMPC_OK;
    r.unsolved_seen = cur;
    SolveCall deferred; deferred.x0_from_results = true;
    ALMPC_TRY(launch_redo(h, deferred, true, true));
    HIP_TRY(h, stream_wait_polling(h));   // (a redo is 0.1 - 0.4 ms of kernels: the blocking wait's wake-up alone was seen to double that)
    return ALMPC_OK;
}

// Gated redo behind the last enqueued step (no host look, no synchronisation): see almpc_handle::Redo.  Called where the step's
// results are about to be consumed without a synchronous call; does nothing unless a lazily deferred redo is pending.
int enqueue_gated_redo(almpc_handle* h, bool predicted = false) {
    if (!h->redo.lazy_pending || !h->redo.dGate || h->sw.no_gated_redo) return ALMPC_OK;
    SolveCall gated; gated.x0_from_results = true; gated.gated = true; gated.predicted = predicted;
    // As few launches as possible.  An input box alone (no state rows, no S): the primal Riccati active set by itself -- it is the
    // solver that needs no certificate from another one (slower per instance than the dual method, but what it gets here is rare) --,
    // ONE launch.  Otherwise the dual method's 128-row build in one launch (+ the stage records of per-instance models).
    const bool primal = primal_redo_ready(h);
    ALMPC_TRY(launch_redo(h, gated, !primal, primal));
    h->redo.lazy_pending = false;   // (this step is settled on the stream; a later synchronous look has nothing left to do for it)
    return ALMPC_OK;
}

// Synchronous look: wait for the handle's stream, then settle the last step's deferred redo.  A closed loop that leaves instances
// undecided tends to leave them step after step (the same plants sit at the edge of feasibility), and a redo enqueued AFTER the host has
// seen the count pays a wake-up and a launch latency with the GPU idle: when the previous look found undecided instances, the redo goes
// on the stream GATED behind the step before the wait -- it runs without the host in between if the step left anything, and costs two
// idle launches if it did not.  The look itself then only reads the count, to know what to expect of the next step.
int wait_and_settle(almpc_handle* h, bool blocking_only = false) {
    almpc_handle::Redo& r = h->redo;
    bool predicted = false;
    if (r.lazy_pending && r.expected && r.dGate && r.hUnsolved && !h->sw.no_predicted_redo) {
        const int rc = enqueue_gated_redo(h, true);
        if (rc != ALMPC_OK) return rc;
        predicted = !r.lazy_pending;
    }
    if (blocking_only) HIP_TRY(h, hipStreamSynchronize(h->stream));
    else HIP_TRY(h, stream_wait_polling(h));
    if (predicted) {
        const int cur = *reinterpret_cast<volatile int*>(r.hUnsolved.get());
        r.expected = cur != r.unsolved_seen;
        r.unsolved_seen = cur;
        return ALMPC_OK;
    }
    return resolve_lazy_redo(h);
}

// A new design voids a redo that was deferred for a step of the previous one (its models, references and results are about to go)
void drop_lazy_redo(almpc_handle* h) {
    h->sens.stepped = false; h->sens.v_ok = false; h->sens.t1_ok = false; h->sens.have = 0;   // (what a sensitivity call looks at goes with the design as well)
    h->cert.have = 0; h->cert.kept = false;
    h->kept.on_device = 0;
    h->redo.lazy_pending = false;
    h->redo.expected = false;
    h->weighted = false;   // (almpc_design_batched_weighted sets it again behind this call)
    if (h->redo.hUnsolved) h->redo.unsolved_seen = *reinterpret_cast<volatile int*>(h->redo.hUnsolved.get());
}

// Lanes of the rollout fused into a finish: g lanes per trajectory row, cpl columns per lane (a power of two); fits: the trajectory
// fits the finish's 32 x 32 buffer with at most 8 columns per lane
struct RollGeom { int g = 1, cpl = 1; bool fits = false; };
RollGeom roll_geom(const almpc_handle* h) {
    RollGeom r;
    while (2 * r.g * h->n <= 64) r.g *= 2;
    const int C = h->n + h->m;
    r.cpl = (C + r.g - 1) / r.g;
    r.fits = (size_t)(h->N + 1) * C <= 32 * 32 && r.cpl <= 8;
    r.cpl = r.cpl <= 1 ? 1 : (r.cpl <= 2 ? 2 : (r.cpl <= 4 ? 4 : 8));
    return r;
}

// Table of the state rows' s0 (PolishGenParams::s0_basis) for a shared design: after the design and after every change of the shared
// references (v0S).  Leaves s0_basis_ok false where the table does not apply (the finish then rolls v0 out).
int build_s0_basis(almpc_handle* h) {
    h->s0_basis_ok = false;
    if (h->mc <= 0 || h->batched || h->ltv || h->structured || !h->dVsPlain || !h->dRowTraj || h->sw.no_s0_basis) return ALMPC_OK;
    const RollGeom roll = roll_geom(h);
    if (!roll.fits) return ALMPC_OK;
    HIP_TRY(h, h->dS0Basis.once((size_t)(h->n + 1) * h->Rs));
    S0BasisParams bp;
    bp.n = h->n; bp.m = h->m; bp.N = h->N; bp.nz = h->nz; bp.nzs = h->nzs; bp.R = h->R; bp.Rs = h->Rs; bp.roll_g = roll.g; bp.roll_cpl = roll.cpl;
    bp.A = h->dA; bp.B = h->dB; bp.Vs = h->dVsPlain; bp.v0S = (h->dV0S && h->fS_stride == 0) ? h->dV0S : nullptr; bp.dvec = h->dD;
    bp.row_traj = h->dRowTraj; bp.out = h->dS0Basis;
    hipLaunchKernelGGL(k_s0_basis, dim3((unsigned)(h->n + 1)), dim3(64), (size_t)(h->N + 1) * (h->n + h->m) * sizeof(double), h->stream, bp);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->s0_basis_ok = true;
    return ALMPC_OK;
}

// ---- building blocks of the design and setup entry points (almpc_design_*, almpc_relin_*_setup, almpc_sqp_*_setup) -----------------

// The state box of almpc_set_state_box (both null: none)
struct StateBox { const double *min = nullptr, *max = nullptr; };
StateBox state_box(const almpc_handle* h) {
    StateBox box;
    if (!h->boxmin.empty()) { box.min = h->boxmin.data(); box.max = h->boxmax.data(); }
    return box;
}

// The input box of a design: checked among the arguments (who: the call's name in the message), uploaded behind the first device calls
int check_input_box(almpc_handle* h, const double* umin, const double* umax, const char* who) {
    for (int i = 0; i < h->m; ++i)
        if (!(umin[i] <= umax[i])) return fail(h, ALMPC_ERR_INVALID, std::string(who) + ": umin > umax");
    return ALMPC_OK;
}
int upload_input_box(almpc_handle* h, const double* umin, const double* umax) {
    const int m = h->m;
    HIP_TRY(h, hipMemcpy(h->dUmin, umin, m * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->dUmax, umax, m * sizeof(double), hipMemcpyHostToDevice));
    return ALMPC_OK;
}

// The head of a design or setup call: from here on the handle's previous design is being overwritten (designed again only with the
// call's last statement), with it -- where the caller says so -- an SQP loop and a re-linearisation pipeline set up on the handle;
// WAIT_STREAM: and the handle's stream is idle
enum : unsigned { DROP_SQP = 1u, DROP_RELIN = 2u, WAIT_STREAM = 4u };
int begin_redesign(almpc_handle* h, unsigned what) {
    h->designed = false;
    h->lsw.ready = false;   // (almpc_design_ltv_stagewise sets it again behind this call)
    if (what & DROP_SQP) h->sqp.ready = h->sqp.started = false;
    if (what & DROP_RELIN) h->relin.ready = false;
    HIP_TRY(h, hipSetDevice(h->device));
    if (what & WAIT_STREAM) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return ALMPC_OK;
}

// Terminal weights of a per-instance design, into Pall: the caller's (one matrix, or one per instance), else -- unless k_dare makes
// them behind the uploads (dev_dare: Pall stays empty) -- the DARE solution of every instance's model (src/sub/design_mpc.jl:327)
// Qi, Ri (almpc_design_batched_weighted): [batch] weights, instance i's DARE from its own pair instead of (Qm, Rm)
int terminal_weights(almpc_handle* h, const double* A_batch, const double* B_batch, const hm::mat& Qm, const hm::mat& Rm, const double* P,
                     int P_per_instance, bool dev_dare, const char* who, hm::mat& Pall, const double* Qi = nullptr, const double* Ri = nullptr) {
    const size_t n = (size_t)h->n, m = (size_t)h->m, b = (size_t)h->batch;
    if (P) Pall.assign(P, P + (P_per_instance ? b : 1) * n * n);
    else if (!dev_dare) {
        Pall.resize(b * n * n);
        for (size_t i = 0; i < b; ++i) {
            hm::mat Am(A_batch + i * n * n, A_batch + (i + 1) * n * n), Bm(B_batch + i * n * m, B_batch + (i + 1) * n * m), Pm;
            const char* what = "";
            const bool ok = Qi ? host_dare_of(h, Am, Bm, hm::mat(Qi + i * n * n, Qi + (i + 1) * n * n), hm::mat(Ri + i * m * m, Ri + (i + 1) * m * m), Pm, &what)
                               : host_dare_of(h, Am, Bm, Qm, Rm, Pm, &what);
            if (!ok) return fail(h, ALMPC_ERR_NUMERIC, std::string(who) + ": " + what + " for instance " + std::to_string(i));
            std::copy(Pm.begin(), Pm.end(), Pall.begin() + i * n * n);
        }
    }
    return ALMPC_OK;
}

// k_sdual's set-up from a shared model with its terminal weight (stage records by the host, at design time) or -- null -- for the
// handle's per-instance model slots (records by k_sgains; one_stage: the terminal weight is the instance's own DARE solution)
struct SharedModel { const hm::mat &A, &B, &P; };
int setup_sdual(almpc_handle* h, const SharedModel* shared, bool one_stage, const hm::mat& Qm, const hm::mat& Rm, const hm::mat* Sm, StateBox box) {
    if (!shared) return sdual_setup_batched(h, Qm, Rm, Sm, one_stage, box.min, box.max, h->terminal_eq != 0);
    hm::mat Rb = Rm;   // the reference's branch rule (src/sub/design_mpc.jl:423-466): R enters only with a non-zero [1,1] element
    if (Rm[0] == 0.0) std::fill(Rb.begin(), Rb.end(), 0.0);
    return sdual_setup_shared(h, shared->A, shared->B, Qm, Rb, Sm, shared->P, box.min, box.max, h->terminal_eq != 0);
}

bool primal_redo_covers(const almpc_handle* h, bool rows, bool useS) { return riccati_shape_ok(h) && !rows && !useS; }

// The redo of the instances a condensed step leaves without a certificate, and the stage-wise QP of an SQP iteration: the stage-wise
// dual active set (k_sdual: also state rows and the input-rate weight, Sm non-null) and behind it -- input box only, no S -- the primal
// Riccati active set.  must: a solver that cannot be set up is the call's error (refusal: the text for a shape outside k_sdual), else
// the design goes on without it.  h->sd.ready says afterwards whether k_sdual is set up; what follows from that is the caller's.
int setup_redo_solvers(almpc_handle* h, const SharedModel* shared, bool one_stage, const hm::mat& Qm, const hm::mat& Rm, const hm::mat* Sm,
                       StateBox box, bool must, const char* refusal) {
    const bool useS = Sm != nullptr, rows = box.min || h->terminal_eq;
    h->sd.ready = false;
    if (sdual_shape_ok(h->n, h->m, h->N, useS)) {
        const int rc = setup_sdual(h, shared, one_stage, Qm, Rm, Sm, box);
        if (rc != ALMPC_OK && must) return rc;
    } else if (must && (rows || useS))
        return fail(h, ALMPC_ERR_UNSUPPORTED, refusal);
    if (primal_redo_covers(h, rows, useS)) ALMPC_TRY(riccati_weights(h, Qm, Rm, shared ? shared->P.data() : nullptr));
    return ALMPC_OK;
}

// The solvers of a design on an ALMPC_FLAG_STRUCTURED handle, which has no others: k_sdual (input box, state box, terminal equality,
// input-rate weight) and the primal k_riccati (input box only) -- the solver of shapes k_sdual does not cover and the safety net for
// instances the dual method leaves without a certificate (a saturated open-loop unstable plant: Ghat_WW numerically singular)
int setup_structured_solvers(almpc_handle* h, const SharedModel* shared, bool one_stage, const hm::mat& Qm, const hm::mat& Rm, const hm::mat* Sm,
                             StateBox box) {
    const bool useS = Sm != nullptr;
    h->sd.ready = false;
    if (sdual_shape_ok(h->n, h->m, h->N, useS) && !h->sw.structured_primal)
        ALMPC_TRY(setup_sdual(h, shared, one_stage, Qm, Rm, Sm, box));
    else if (box.min || h->terminal_eq || useS)
        return fail(h, ALMPC_ERR_UNSUPPORTED, "structured solve: state rows / input-rate weight need the stage-wise dual solve (n + m <= 48, (N + 1)(n + m) <= 4096)");
    if (riccati_shape_ok(h)) ALMPC_TRY(riccati_weights(h, Qm, Rm, shared ? shared->P.data() : nullptr));
    else if (!h->sd.ready) return fail(h, ALMPC_ERR_UNSUPPORTED, "structured solve: shape outside both stage-wise solvers");
    return ALMPC_OK;
}

// The tail of a design: default references (zeros, shared).  A design whose references cannot be set is not left "designed".
int set_zero_reference(almpc_handle* h) {
    std::vector<double> xr((size_t)h->n * (h->N + 1), 0.0), ur((size_t)h->nz, 0.0);
    const int rc = almpc_set_reference(h, xr.data(), ur.data(), 0);
    if (rc != ALMPC_OK) h->designed = false;
    return rc;
}

}  // namespace

extern "C" {

void almpc_default_opts(almpc_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->rho = 0.1;
    o->sigma = 1e-6;
    o->alpha = 1.6;
    o->eps_abs = 1e-3;
    o->eps_rel = 1e-3;
    o->max_iter = 25;
    o->check_every = 25;
    o->polish = 1;
    o->polish_max_iter = 0;
    o->warm_start = 0;
}

// (without a handle: the text of the calling thread's last failed almpc_dare_vjp, handed out once)
static thread_local std::string g_nohandle_err, g_nohandle_err_out;
const char* almpc_last_error(const almpc_handle* h) {
    if (h) return h->err.c_str();
    if (g_nohandle_err.empty()) return "null handle";
    g_nohandle_err_out.swap(g_nohandle_err);
    g_nohandle_err.clear();
    return g_nohandle_err_out.c_str();
}

int almpc_create(almpc_handle** out, int n, int m, int N, int batch, int device_id, uint32_t flags) {
    if (!out) return ALMPC_ERR_INVALID;
    *out = nullptr;
    if (n < 1 || m < 1 || N < 1 || batch < 1) return ALMPC_ERR_INVALID;
    const bool structured = (flags & ALMPC_FLAG_STRUCTURED) != 0;
    if (structured) {
        if (n > 32 || m > 16 || (long)m * N > 1024 || riccati_lds_doubles(n, m, N) * sizeof(double) > 160 * 1024) return ALMPC_ERR_UNSUPPORTED;
    } else if (n > 64 || (long)m * N > 128) return ALMPC_ERR_UNSUPPORTED;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return ALMPC_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= count) return ALMPC_ERR_NO_DEVICE;
    almpc_handle* h = new almpc_handle();
    h->sw = read_switches();
    h->fuse_step = h->sw.no_fused_step ? 0 : 1;
    h->n = n; h->m = m; h->N = N; h->batch = batch; h->device = device_id; h->flags = flags;
    h->structured = structured;
    h->nz = m * N;
    h->nrb = (h->nz + 15) / 16;
    h->nzs = 16 * h->nrb;
    h->ks = pick_ks(h->nz, h->nrb);
    h->ksf = (n + 3) / 4;
    auto bail = [&](int code, const std::string& msg) {
        std::fprintf(stderr, "almpc_create: %s\n", msg.c_str());
        destroy_handle(h);
        return code;
    };
#define TRY(call)                                                                  \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) return bail(ALMPC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)
    TRY(hipSetDevice(device_id));
    TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    {
        int cus = 0;
        TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id));
        if (cus > 0) h->num_cus = cus;
    }
    const size_t fr = (size_t)h->nrb * h->ks * 64, b = (size_t)batch;
    if (structured) {   // no condensed matrices: models, references, inputs / outputs and the gain scratch only
        TRY(h->dUmin.alloc((size_t)m)); TRY(h->dUmax.alloc((size_t)m));
        TRY(h->dA.alloc((size_t)n * n)); TRY(h->dB.alloc((size_t)n * m));
        TRY(h->x0_own.alloc(b * n)); h->dX0 = h->x0_own;
        TRY(h->dX.alloc(b * n * (N + 1))); TRY(h->dEx.alloc(b * n * (N + 1)));
        TRY(h->dU.alloc(b * h->nz)); TRY(h->dEu.alloc(b * h->nz));
        TRY(h->dStatus.alloc(b)); TRY(h->dIters.alloc(b)); TRY(h->dPiters.alloc(b));
        TRY(hipMemset(h->dIters, 0, b * sizeof(int32_t)));
        TRY(hipMemset(h->dX0, 0, b * n * sizeof(double)));
        *out = h;
        return ALMPC_OK;
    }
    TRY(h->dMinvFrag.alloc(fr)); TRY(h->dVFrag.alloc((size_t)h->nrb * h->ksf * 64)); TRY(h->dHFrag.alloc(fr));
    TRY(h->dFFrag.alloc((size_t)h->nrb * h->ksf * 64));
    TRY(h->dG.alloc((size_t)h->nz * h->nzs));
    TRY(h->dD.alloc((size_t)h->nzs)); TRY(h->dRho.alloc((size_t)h->nzs)); TRY(h->dUmin.alloc((size_t)m)); TRY(h->dUmax.alloc((size_t)m));
    TRY(h->dA.alloc((size_t)n * n)); TRY(h->dB.alloc((size_t)n * m));
    TRY(h->x0_own.alloc(b * n)); h->dX0 = h->x0_own;
    TRY(h->dXs.alloc(b * h->nzs)); TRY(h->dZs.alloc(b * h->nzs)); TRY(h->dYs.alloc(b * h->nzs));
    TRY(h->dV0.alloc(b * h->nzs)); TRY(h->dW.alloc(b * h->nzs));
    TRY(h->dX.alloc(b * n * (N + 1))); TRY(h->dEx.alloc(b * n * (N + 1)));
    TRY(h->dU.alloc(b * h->nz)); TRY(h->dEu.alloc(b * h->nz));
    TRY(h->dSglobal.alloc(b * POLISH_GLB_PER_INST));
    TRY(h->dPerm.alloc(((b + 15) / 16) * 16));
    TRY(hipMemset(h->dPerm, 0xFF, ((b + 15) / 16) * 16 * sizeof(int32_t)));
    TRY(h->dStatus.alloc(b)); TRY(h->dIters.alloc(b)); TRY(h->dPiters.alloc(b));
    TRY(h->dYflags.alloc(b * h->nrb));
    TRY(hipMemset(h->dXs, 0, b * h->nzs * sizeof(double)));
    TRY(hipMemset(h->dZs, 0, b * h->nzs * sizeof(double)));
    TRY(hipMemset(h->dYs, 0, b * h->nzs * sizeof(double)));
    TRY(hipMemset(h->dX0, 0, b * n * sizeof(double)));
#undef TRY
    *out = h;
    return ALMPC_OK;
}

void almpc_destroy(almpc_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    destroy_handle(h);
}

int almpc_set_rho_profile(almpc_handle* h, int mode) {
    if (!h) return ALMPC_ERR_INVALID;
    if (mode != 0 && mode != 1) return fail(h, ALMPC_ERR_INVALID, "rho profile: 0 (scalar) or 1 (stiffness)");
    h->rho_mode = mode;
    h->designed = false;  // takes effect at the next design
    return ALMPC_OK;
}

int almpc_set_step_fusion(almpc_handle* h, int on) {
    if (!h) return ALMPC_ERR_INVALID;
    h->fuse_step = on ? 1 : 0;
    return ALMPC_OK;
}

int almpc_set_terminal_equality(almpc_handle* h, int on) {
    if (!h) return ALMPC_ERR_INVALID;
    h->terminal_eq = on ? 1 : 0;
    h->designed = false;  // takes effect at the next design
    return ALMPC_OK;
}

int almpc_set_state_box(almpc_handle* h, const double* xmin, const double* xmax) {
    if (!h) return ALMPC_ERR_INVALID;
    if ((xmin == nullptr) != (xmax == nullptr)) return fail(h, ALMPC_ERR_INVALID, "set_state_box: give both xmin and xmax or neither");
    if (xmin) {
        for (int i = 0; i < h->n; ++i)
            if (!(xmin[i] <= xmax[i])) return fail(h, ALMPC_ERR_INVALID, "set_state_box: xmin > xmax");
        h->boxmin.assign(xmin, xmin + h->n); h->boxmax.assign(xmax, xmax + h->n);
    } else { h->boxmin.clear(); h->boxmax.clear(); }
    h->designed = false;  // takes effect at the next per-instance / time-varying / SQP design
    h->sqp.ready = h->sqp.started = false;
    h->relin.ready = false;
    return ALMPC_OK;
}

int almpc_set_structured_fallback(almpc_handle* h, int on) {
    if (!h) return ALMPC_ERR_INVALID;
    if (on && !riccati_shape_ok(h) && !sdual_shape_ok(h->n, h->m, h->N, false))
        return fail(h, ALMPC_ERR_UNSUPPORTED, "structured fallback: the shape is outside both stage-wise solvers");
    h->fallback = on ? 1 : 0;
    h->designed = false;  // takes effect at the next design (which prepares the weights on the device)
    return ALMPC_OK;
}

int almpc_set_start_from(almpc_handle* h, almpc_handle* src) {
    if (!h || !src) return ALMPC_ERR_INVALID;
    if (!h->structured) return fail(h, ALMPC_ERR_UNSUPPORTED, "set_start_from: the handle must be a structured one (ALMPC_FLAG_STRUCTURED)");
    if (!h->designed || !src->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, "set_start_from before design (of either handle)");
    if (src->n != h->n || src->m != h->m || src->batch != h->batch || src->N > h->N || src->device != h->device)
        return fail(h, ALMPC_ERR_INVALID, "set_start_from: the source must have the same n, m, batch and device and a horizon <= this handle's");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->rGuess.once((size_t)h->batch * h->nz));
    if (!h->ev_guess) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_guess, hipEventDisableTiming));
    // the source's last step must be done before its inputs are read on this handle's stream (no host wait)
    HIP_TRY(h, hipEventRecord(h->ev_guess, src->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_guess, 0));
    const long cnt = (long)h->batch * h->nz;
    hipLaunchKernelGGL(k_guess_from_inputs, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, h->batch, h->m, src->N, h->N, 0,
                       (const double*)src->dU, (const double*)h->dUref, h->uref_stride, h->rGuess);
    HIP_TRY(h, hipGetLastError());
    // ... and src's NEXT step must not overwrite its inputs before that kernel has read them: src's stream waits for it
    if (!h->ev_guess_done) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_guess_done, hipEventDisableTiming));
    HIP_TRY(h, hipEventRecord(h->ev_guess_done, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(src->stream, h->ev_guess_done, 0));
    h->guess_ready = true;
    return ALMPC_OK;
}

// ALMPC_FLAG_STRUCTURED: no condensed matrices at all; rho / sigma are not used
static int design_shared_structured(almpc_handle* h, const double* A, const double* B, const double* Q, const double* R, const double* S,
                                    const double* P, const double* umin, const double* umax, const double* xmin, const double* xmax) {
    const int n = h->n, m = h->m;
    if ((xmin == nullptr) != (xmax == nullptr)) return fail(h, ALMPC_ERR_INVALID, "design: give both xmin and xmax or neither");
    ALMPC_TRY(check_input_box(h, umin, umax, "design"));
    if (xmin)
        for (int i = 0; i < n; ++i)
            if (!(xmin[i] <= xmax[i])) return fail(h, ALMPC_ERR_INVALID, "design: xmin > xmax");
    h->r_has_step = false; h->guess_ready = false;
    ALMPC_TRY(begin_redesign(h, DROP_SQP | DROP_RELIN));   // (an SQP loop or pipeline set up on this handle is gone with its references)
    hm::mat Am(A, A + (size_t)n * n), Bm(B, B + (size_t)n * m), Qm(Q, Q + (size_t)n * n), Rm(R, R + (size_t)m * m), Pm;
    if (P) Pm.assign(P, P + (size_t)n * n);
    else if (!hm::dare(Am, Bm, Qm, Rm, n, m, Pm)) return fail(h, ALMPC_ERR_NUMERIC, "design: DARE did not converge");
    h->P = Pm; h->H.clear(); h->F.clear(); h->d.clear();
    // the reference's branch rules (src/sub/design_mpc.jl:423-466): R and S enter only with a non-zero [1,1] element, S only with R
    const bool useS = R[0] != 0.0 && S && S[0] != 0.0;
    hm::mat Sm;
    if (useS) Sm.assign(S, S + (size_t)m * m);
    const SharedModel model{Am, Bm, Pm};
    ALMPC_TRY(setup_structured_solvers(h, &model, false, Qm, Rm, useS ? &Sm : nullptr, StateBox{xmin, xmax}));
    ALMPC_TRY(upload_input_box(h, umin, umax));
    HIP_TRY(h, hipMemcpy(h->dA, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->dB, B, (size_t)n * m * sizeof(double), hipMemcpyHostToDevice));
    h->batched = false; h->ltv = false; h->r_batched_P = false; h->rP_stride = 0;
    keep_weights(h, nullptr, nullptr, useS ? Sm : hm::mat((size_t)m * m, 0.0), R[0] != 0.0, useS);
    h->has_box = xmin ? 1 : 0;
    h->designed = true;
    return set_zero_reference(h);
}

// The n terminal-equality rows (the last n state rows) of a shared design are in every working set: eliminated here, once
static int project_terminal_equality(almpc_handle* h) {
    const int n = h->n;
    if (!(h->terminal_eq && h->mc >= n && !h->sw.no_eq_projection)) return ALMPC_OK;
    const int ne = n, eq0 = h->R - n, Rs = h->Rs;
    std::vector<double> GE((size_t)ne * Rs), GEE((size_t)ne * ne), Y;
    HIP_TRY(h, hipMemcpy(GE.data(), h->dGhat + (size_t)eq0 * Rs, GE.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int a = 0; a < ne; ++a)
        for (int b = 0; b < ne; ++b) GEE[(size_t)b * ne + a] = GE[(size_t)a * Rs + eq0 + b];
    hm::mat Winv = hm::eye(ne);
    bool ok = hm::lu_solve(GEE, Winv, ne, ne);
    for (double v : Winv) ok = ok && std::isfinite(v);
    if (!ok) return ALMPC_OK;   // (a singular Ghat_EE -- terminal state not reachable in N steps -- keeps the row-by-row path, which reports it)
    Y.assign((size_t)ne * Rs, 0.0);   // Y = Winv GhatE, row-major [ne][Rs]
    for (int a = 0; a < ne; ++a)
        for (int e = 0; e < ne; ++e) {
            const double wv = Winv[(size_t)e * ne + a];   // Winv(a, e)
            for (int b = 0; b < Rs; ++b) Y[(size_t)a * Rs + b] += wv * GE[(size_t)e * Rs + b];
        }
    std::vector<double> Wrow((size_t)ne * ne);
    for (int a = 0; a < ne; ++a)
        for (int e = 0; e < ne; ++e) Wrow[(size_t)a * ne + e] = Winv[(size_t)e * ne + a];
    DevBuf<double> dY;
    HIP_TRY(h, h->dGhatE.alloc(GE.size())); HIP_TRY(h, h->dWinvE.alloc(Wrow.size())); HIP_TRY(h, dY.alloc(Y.size()));
    HIP_TRY(h, hipMemcpy(h->dGhatE, GE.data(), GE.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->dWinvE, Wrow.data(), Wrow.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(dY, Y.data(), Y.size() * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_ghat_project, dim3(512), dim3(256), 0, h->stream, h->R, Rs, ne, eq0, h->dGhatE, dY, h->dGhat, h->dGnorm);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->eq_proj = 1;
    return ALMPC_OK;
}

// Blocked rollout of a shared model: s stages per block with one lane per (stage, state row); lane (j, i) holds row i of
// [A^j B, ..., A B, B (stages t = 0..j), 0 ... | A^(j+1)]  (design-time host math, n x n products)
static int build_rollout_table(almpc_handle* h, const hm::mat& Am, const hm::mat& Bm) {
    const int n = h->n, m = h->m, N = h->N;
    int sblk = std::min(N, std::min(64 / n, ROLL_SMX / m));
    h->roll_s = 0;
    if (!(sblk >= 1 && n <= ROLL_NX && !h->sw.rollout_stagewise)) return ALMPC_OK;
    std::vector<double> M((size_t)(ROLL_SMX + ROLL_NX) * 64, 0.0);
    std::vector<hm::mat> Apow(sblk + 1), ApB(sblk);  // A^j, A^j B
    Apow[0] = hm::eye(n);
    for (int j = 1; j <= sblk; ++j) Apow[j] = hm::mul(Am, Apow[j - 1], n, n, n);
    for (int j = 0; j < sblk; ++j) ApB[j] = hm::mul(Apow[j], Bm, n, n, m);
    for (int j = 0; j < sblk; ++j)
        for (int i = 0; i < n; ++i) {
            const int lane = j * n + i;
            for (int t = 0; t <= j; ++t)
                for (int a = 0; a < m; ++a) M[(size_t)(t * m + a) * 64 + lane] = ApB[j - t][(size_t)a * n + i];
            for (int c = 0; c < n; ++c) M[(size_t)(ROLL_SMX + c) * 64 + lane] = Apow[j + 1][(size_t)c * n + i];
        }
    HIP_TRY(h, h->dRollM.alloc(M.size()));
    HIP_TRY(h, hipMemcpy(h->dRollM, M.data(), M.size() * sizeof(double), hipMemcpyHostToDevice));
    h->roll_s = sblk; h->roll_nb = (N + sblk - 1) / sblk;
    return ALMPC_OK;
}

static int design_shared_condensed(almpc_handle* h, const double* A, const double* B, const double* Q, const double* R, const double* S,
                                   const double* P, const double* umin, const double* umax, const double* xmin, const double* xmax,
                                   double rho, double sigma) {
    if ((xmin == nullptr) != (xmax == nullptr)) return fail(h, ALMPC_ERR_INVALID, "design: give both xmin and xmax or neither");
    if (!(rho > 0.0) || !(sigma >= 0.0)) return fail(h, ALMPC_ERR_INVALID, "design: rho must be > 0 and sigma >= 0");
    ALMPC_TRY(begin_redesign(h, DROP_SQP | DROP_RELIN));
    const int n = h->n, m = h->m, N = h->N;
    ALMPC_TRY(check_input_box(h, umin, umax, "design"));
    hm::mat Am(A, A + (size_t)n * n), Bm(B, B + (size_t)n * m), Qm(Q, Q + (size_t)n * n), Rm(R, R + (size_t)m * m);
    hm::mat Pm;
    if (P) Pm.assign(P, P + (size_t)n * n);
    else if (!hm::dare(Am, Bm, Qm, Rm, n, m, Pm)) return fail(h, ALMPC_ERR_NUMERIC, "design: DARE did not converge");
    h->P = Pm;
    const hm::mat Sm = hm::symmetrised(S, m);   // S enters the cost as a quadratic form: only its symmetric part counts
    keep_weights(h, &Qm, &Rm, Sm, Rm[0] != 0.0, Rm[0] != 0.0 && Sm[0] != 0.0);  // the reference drops the S term together with R (src/sub/design_mpc.jl:423-466)
    h->rho = rho; h->sigma = sigma;

    // ---- state rows (state box, terminal equality): row tables and the shared constraint-space matrix
    ALMPC_TRY(setup_state_rows(h, xmin, xmax, false));
    std::vector<int> rowsel;   // rows of Gamma the state rows are, in row order
    for (int k = 0; k < N; ++k)
        for (int i = 0; i < n; ++i)
            if (h->has_box || (h->terminal_eq && k == N - 1)) rowsel.push_back(k * n + i);
    h->s0_basis_ok = false;
    if (!rowsel.empty()) HIP_TRY(h, h->dVsPlain.once((size_t)n * h->nzs));
    if (h->nzs <= 64) HIP_TRY(h, h->dPlain.once(2 * (size_t)h->nz * h->nzs + 2 * (size_t)n * h->nzs));
    ALMPC_TRY(design_shared_device(h->stream, n, m, N, h->nzs, h->nrb, h->ks, h->ksf, Am, Bm, Qm, Rm, Sm, Pm, rho, sigma,
                                   h->dMinvFrag, h->dVFrag, h->dHFrag, h->dFFrag, h->dG, h->dD, h->H, h->F, h->d, h->err,
                                   rowsel, h->Rs, h->dGhat, h->dGnorm, h->rho_mode, h->dRho, rowsel.empty() ? nullptr : h->dVsPlain,
                                   h->nzs <= 64 ? h->dPlain : nullptr, &h->dMinv, &h->dCold));
    ALMPC_TRY(project_terminal_equality(h));
    ALMPC_TRY(upload_input_box(h, umin, umax));
    HIP_TRY(h, hipMemcpy(h->dA, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->dB, B, (size_t)n * m * sizeof(double), hipMemcpyHostToDevice));
    ALMPC_TRY(build_rollout_table(h, Am, Bm));
    // redo of the instances a step leaves without a certificate (default on)
    h->sd.ready = false;
    if (h->fallback) {
        const bool useS = h->kept.useS != 0;
        const SharedModel model{Am, Bm, Pm};
        ALMPC_TRY(setup_redo_solvers(h, &model, false, Qm, Rm, useS ? &Sm : nullptr, StateBox{xmin, xmax}, h->fallback == 1,
                                     "structured fallback: state rows / input-rate weight need n + m <= 48 and (N + 1)(n + m) <= 4096"));
        if (primal_redo_covers(h, h->mc > 0, useS)) { h->r_batched_P = false; h->rP_stride = 0; }   // (k_riccati: the shared P)
    }
    h->designed = true; h->batched = false; h->ltv = false;
    return set_zero_reference(h);
}

int almpc_design_shared(almpc_handle* h, const double* A, const double* B, const double* Q, const double* R,
                        const double* S, const double* P, const double* umin, const double* umax,
                        const double* xmin, const double* xmax, double rho, double sigma) {
    if (!h) return ALMPC_ERR_INVALID;
    hm::mat Ad, Bd;
    if (A && B && model_continuous(h)) {
        // almpc_set_model_time: (A, B) is continuous-time; its zero-order hold is the model the handle is designed on and keeps
        // (src/sub/design_mpc.jl:22-41: discretise, then the discrete method)
        const int n = h->n, m = h->m;
        if (hm::c2d(hm::mat(A, A + (size_t)n * n), hm::mat(B, B + (size_t)n * m), h->model_Ts, n, m, Ad, Bd) != 0) {
            h->designed = false;
            return fail(h, ALMPC_ERR_NUMERIC, "design: discretisation of the continuous-time model failed (not finite, or |A| Ts beyond 2^59)");
        }
        A = Ad.data(); B = Bd.data();
    }
    drop_lazy_redo(h);
    if (!A || !B || !Q || !R || !umin || !umax) return fail(h, ALMPC_ERR_INVALID, "design: null matrix pointer");
    return h->structured ? design_shared_structured(h, A, B, Q, R, S, P, umin, umax, xmin, xmax)
                         : design_shared_condensed(h, A, B, Q, R, S, P, umin, umax, xmin, xmax, rho, sigma);
}

}  // extern "C"

namespace {
// Time-varying inputs of almpc_design_ltv (host pointers); nullptr for the time-invariant almpc_design_batched.
struct LtvInputs {
    const double* A_all;   // [batch][N][n*n]
    const double* B_all;   // [batch][N][n*m]
    const double* c_all;   // [batch][N][n] or null
    const double* ebar;    // [batch][N][n]  xbar_{k+1} - x_ref_{k+1}
    const double* qadd;    // [batch][nz]    input part of the gradient
    const double* ubar;    // [batch][nz]    linearisation inputs (become the per-instance input reference)
    const double* xbar;    // [batch][(N+1)*n]
    const double* xref;    // [(N+1)*n] or null   the shared references as the caller gave them (kept for almpc_certificate_ltv)
    const double* uref;    // [nz] or null
};

// Persistent per-instance operands of the batched / LTV / SQP designs (allocated once per handle).
int ensure_batched_alloc(almpc_handle* h) {
    const int n = h->n, m = h->m, N = h->N, nz = h->nz, nzs = h->nzs;
    const size_t b = (size_t)h->batch;
    const int njf = (n + 15) / 16, ps = 16 * njf, gs = nzs;
    const int kr = ((n * N + HESS_KC - 1) / HESS_KC) * HESS_KC;
    if (!h->batched_alloc) {
        HIP_TRY(h, h->bA.alloc(b * n * n)); HIP_TRY(h, h->bB.alloc(b * n * m));
        HIP_TRY(h, h->bMinv.alloc(b * nz * nzs)); HIP_TRY(h, h->bG.alloc(b * nz * nzs)); HIP_TRY(h, h->bHs.alloc(b * nz * nzs));
        HIP_TRY(h, h->bFs.alloc(b * n * nzs)); HIP_TRY(h, h->bVs.alloc(b * n * nzs));
        HIP_TRY(h, h->bD.alloc(b * nzs)); HIP_TRY(h, h->bRho.alloc(b * nzs));
        HIP_TRY(h, h->bH.alloc(b * nz * nz)); HIP_TRY(h, h->bF.alloc(b * nz * n));
        if (design_instance_lds_doubles(n, m, N) * sizeof(double) > 160 * 1024) {  // dense route only: Gamma panels in HBM
            HIP_TRY(h, h->bPhi.alloc(b * N * n * n)); HIP_TRY(h, h->bGk.alloc(b * N * n * m));
            HIP_TRY(h, h->bGam.alloc(b * kr * gs)); HIP_TRY(h, h->bW.alloc(b * kr * gs)); HIP_TRY(h, h->bWP.alloc(b * kr * ps));
            // padding rows / columns of the row-major panels stay zero for the lifetime of the handle
            HIP_TRY(h, hipMemset(h->bGam, 0, b * kr * gs * sizeof(double)));
            HIP_TRY(h, hipMemset(h->bW, 0, b * kr * gs * sizeof(double)));
            HIP_TRY(h, hipMemset(h->bWP, 0, b * kr * ps * sizeof(double)));
        }
        HIP_TRY(h, h->bP.alloc(b * n * n));
        HIP_TRY(h, h->bFlag.alloc(b));
        HIP_TRY(h, hipMemset(h->bHs, 0, b * nz * nzs * sizeof(double)));
        HIP_TRY(h, hipMemset(h->bFs, 0, b * n * nzs * sizeof(double)));
        HIP_TRY(h, hipMemset(h->bVs, 0, b * n * nzs * sizeof(double)));
        HIP_TRY(h, hipMemset(h->bMinv, 0, b * nz * nzs * sizeof(double)));
        HIP_TRY(h, hipMemset(h->bG, 0, b * nz * nzs * sizeof(double)));
        h->batched_alloc = true;
    }
    return ALMPC_OK;
}

// H_i (column-major, in bH) -> Jacobi scaling d_i, H'_i, F'_i, G_i = H'_i^-1, rho_i, Minv_i = (H'_i + sigma I + diag(rho_i))^-1
// (scaled: the producer of H_i has done the scaling as its own tail)
// (with_v: also V_i = -G_i F'_i -- inside the first inverse's launch where that kernel can, else by launch_neg_gm_batched)
// (v1M / v1Out: instead of V_i, ONE column per instance -- the SQP iteration's v0S_i = -G_i fS_i, [batch][nz] each)
// (no_admm: the solve that follows has no ADMM phase -- its guess comes from elsewhere, StepMode::guess -- and needs no KKT inverse)
void launch_batched_factor(almpc_handle* h, const DesignStrides& ds, double rho, double sigma, hipStream_t st, bool no_admm, bool scaled = false,
                           bool with_v = false, const double* v1M = nullptr, double* v1Out = nullptr) {
    const int n = h->n, nz = h->nz, nzs = h->nzs;
    const unsigned gb = (unsigned)h->batch;
    if (!scaled) hipLaunchKernelGGL(k_design_scale, dim3(1, gb), dim3(256), 0, st, nz, nzs, n, h->bH, h->bF, h->bD, h->bHs, h->bFs, h->bFlag, ds);
    const size_t inv_lds = 520 * sizeof(double);
    if (!v1M && !no_admm && h->rho_mode == 0 && design_inverse_makes_rho(h->sw, nz, nzs) && nz <= 64 && design_inverse_makes_v(h->sw, nz) && !h->sw.dbg_split_inverses) {
        // scalar rho: the ADMM's KKT inverse does not need G_i -- both inverses, the penalty profile and V_i in ONE launch
        h->minv_packed = false;
        launch_design_inverse(h->sw, dim3(1, gb), inv_lds, st, nz, nzs, h->bHs, 0.0, (const double*)nullptr, h->bG, h->bFlag, ds.Hs, ds.rho, ds.G, 1L,
                              (const double*)nullptr, 0L, 0, rho, h->bRho, with_v ? h->bFs : nullptr, h->bVs, ds.Fs, n, h->bMinv, ds.Minv, sigma);
        return;
    }
    if (v1M && design_inverse_makes_v(h->sw, nz))   // one column per instance from the rows / columns of G_i the inverse still holds
        launch_design_inverse(h->sw, dim3(1, gb), inv_lds, st, nz, nzs, h->bHs, 0.0, (const double*)nullptr, h->bG, h->bFlag, ds.Hs, 0L, ds.G, 1L,
                              (const double*)nullptr, 0L, 0, 0.0, (double*)nullptr, v1M, v1Out, (long)nz, 1, (double*)nullptr, 0L, 0.0, nz);
    else if (with_v && nz <= 64 && design_inverse_makes_v(h->sw, nz))   // V_i = -G_i F'_i from the rows of G_i the inverse's wave still holds (the
                                                                  // column-split kernel: measured slower than k_neg_gm_cols for n columns)
        launch_design_inverse(h->sw, dim3(1, gb), inv_lds, st, nz, nzs, h->bHs, 0.0, (const double*)nullptr, h->bG, h->bFlag, ds.Hs, 0L, ds.G, 1L,
                              (const double*)nullptr, 0L, 0, 0.0, (double*)nullptr, h->bFs, h->bVs, ds.Fs, n);
    else {
        launch_design_inverse(h->sw, dim3(1, gb), inv_lds, st, nz, nzs, h->bHs, 0.0, (const double*)nullptr, h->bG, h->bFlag, ds.Hs, 0L, ds.G, 1L);
        if (with_v) launch_neg_gm_batched(st, gb, nz, nzs, n, h->bG, h->bFs, h->bVs, ds.G, ds.Fs);
    }
    if (no_admm) return;
    h->minv_packed = design_inverse_can_pack(h->sw, nz);   // the ADMM's KKT inverse as its packed triangle: half the stream of k_admm_inst
    const long sMinv = h->minv_packed ? packed_tri_doubles(nz) : ds.Minv;
    if (design_inverse_makes_rho(h->sw, nz, nzs))   // the penalty profile is made inside the inverse's own launch
        launch_design_inverse(h->sw, dim3(1, gb), inv_lds, st, nz, nzs, h->bHs, sigma, (const double*)nullptr, h->bMinv, h->bFlag, ds.Hs, ds.rho, ds.Minv, 1L,
                              h->bG, ds.G, h->rho_mode, rho, h->bRho);
    else {
        hipLaunchKernelGGL(k_design_rho, dim3(1, gb), dim3(256), 0, st, nz, nzs, h->rho_mode, rho, h->bG, h->bRho, ds.G, ds.rho);
        launch_design_inverse(h->sw, dim3(1, gb), inv_lds, st, nz, nzs, h->bHs, sigma, (const double*)h->bRho, h->bMinv, h->bFlag, ds.Hs, ds.rho, sMinv, 1L,
                              (const double*)nullptr, 0L, 0, 0.0, (double*)nullptr, (const double*)nullptr, (double*)nullptr, 0L, 0, (double*)nullptr, 0L, 0.0, 0,
                              h->minv_packed ? 1 : 0);
    }
}

DesignStrides batched_strides(const almpc_handle* h, bool p_inst) {
    const int n = h->n, m = h->m, N = h->N, nz = h->nz, nzs = h->nzs;
    const int njf = (n + 15) / 16, ps = 16 * njf, gs = nzs;
    const int kr = ((n * N + HESS_KC - 1) / HESS_KC) * HESS_KC;
    DesignStrides ds;
    ds.A = (long)n * n; ds.B = (long)n * m; ds.P = p_inst ? (long)n * n : 0; ds.Phi = (long)N * n * n; ds.Gk = (long)N * n * m;
    ds.Gam = (long)kr * gs; ds.WP = (long)kr * ps; ds.H = (long)nz * nz; ds.F = (long)nz * n; ds.d = nzs; ds.Hs = (long)nz * nzs;
    ds.Fs = (long)n * nzs; ds.G = (long)nz * nzs; ds.Minv = (long)nz * nzs; ds.rho = nzs; ds.flag = 1;
    return ds;
}

// The network code of the calls that take an activation (include/almpc.h: ALMPC_NET_CODE(kind, act) = kind << 8 | act; a bare
// activation 0..4 is an Fnn): false for an unknown kind or activation.
static bool decode_net(int code, int* net, int* act) {
    if (code < 0) return false;
    const int k = code >> 8, a = code & 0xff;
    if (k > NET_POLYNET || a > 4) return false;
    *net = k;
    *act = a;
    return true;
}
// The kind and activation of a network setup call: an ALMPC_NET_CODE (the *_fnn_* calls, dense false) or a bare activation 0..4 (the
// *_densenet_* calls: NET_DENSENET has no network code, its weight layout is its own)
static bool setup_net(bool dense, int code, int* net, int* act) {
    if (!dense) return decode_net(code, net, act);
    if (code < 0 || code > 4) return false;
    *net = NET_DENSENET;
    *act = code;
    return true;
}
static const char* net_name(int net) {
    return net == NET_RESNET ? "ResNet" : (net == NET_POLYNET ? "PolyNet" : (net == NET_DENSENET ? "DenseNet" : "Fnn"));
}
// Element counts of the W_h and W_out arrays of a network of kind net: [L] H x H and n x H in the Fnn layout, the DenseNet's
// growing blocks (include/almpc.h)
static size_t net_wh_doubles(int net, int H, int L) { return net == NET_DENSENET ? densenet_wh_offset(H, L) : (size_t)L * H * H; }
static size_t net_wout_doubles(int net, int n, int H, int L) { return (size_t)n * H * (net == NET_DENSENET ? L + 1 : 1); }
// The network of an SQP loop / a re-linearisation pipeline: its shape and fresh device copies of its weights
static hipError_t upload_net(almpc_handle::Net& q, int n, int m, int H, int L, int act, int net, const double* W_in, const double* W_h,
                             const double* b_h, const double* W_out) {
    q.H = H; q.L = L; q.act = act; q.net = net;
    hipError_t e = q.W_in.upload(W_in, (size_t)H * (n + m));
    if (e == hipSuccess) e = q.W_h.upload(W_h, net_wh_doubles(net, H, L));
    if (e == hipSuccess) e = q.b_h.upload(b_h, (size_t)L * H);
    if (e == hipSuccess) e = q.W_out.upload(W_out, net_wout_doubles(net, n, H, L));
    return e;
}
// The instantiation of a network kernel for the kind net (NET_*, from decode_net): pick(std::integral_constant<int, NET>()) at
// NET = net, as in  with_net(net, [](auto k) { return k_fnn_rollout<k>; })
template <class Pick>
static auto with_net(int net, Pick pick) {
    switch (net) {
        case NET_RESNET: return pick(std::integral_constant<int, NET_RESNET>());
        case NET_POLYNET: return pick(std::integral_constant<int, NET_POLYNET>());
        case NET_DENSENET: return pick(std::integral_constant<int, NET_DENSENET>());
        default: return pick(std::integral_constant<int, NET_FNN>());
    }
}

// Jacobians of the network (kind net: NET_*) at p.batch points: wave-per-point build when weights + 4 waves' buffers fit 64 KB of
// LDS, else one workgroup per point (the caller has checked fnn_wave_scratch_doubles against 160 KB).
hipError_t launch_fnn_jacobian(const Switches& sw, const FnnParams& p, int net, int num_cus, hipStream_t st) {
    const size_t nin = (size_t)p.n + p.m;
    // small networks (H (n + m) <= 192 entries of the Jacobian being propagated): two points per wave, one per half-wave
    // (four points per wave, a quarter-wave each: measured no better, 0.305 against 0.303 ms per SQP iteration)
    const int ppw = ((size_t)p.H * nin <= 192 && !sw.fnn_one_point_per_wave) ? 2 : 1;
    const size_t lw = fnn_w_lds_doubles(p.n, p.m, p.H, p.L, ppw, net) * sizeof(double);
    if (lw <= 64 * 1024 && !sw.fnn_wg) {
        int wgs = (p.batch + FNN_W_WAVES * ppw - 1) / (FNN_W_WAVES * ppw);
        const int cap = num_cus * 8;  // 32 waves per CU: a point is a latency chain on one wave (18 us); 16 waves per CU took 55 us for the
                                      // 12800 points of an SQP iteration, 32 take 48 (52 workgroups per CU: 49.5)
        if (wgs > cap) wgs = cap;
        const dim3 g(wgs), blk(64 * FNN_W_WAVES);
        void (*kern)(FnnParams) = with_net(net, [ppw](auto k) { return ppw == 2 ? k_fnn_jacobian_w<32, k> : k_fnn_jacobian_w<64, k>; });
        hipLaunchKernelGGL(kern, g, blk, lw, st, p);
        return hipGetLastError();
    }
    const size_t lds = fnn_wave_scratch_doubles(p.n, p.m, p.H, p.L, net) * sizeof(double);
    void (*kern)(FnnParams) = with_net(net, [](auto k) { return k_fnn_jacobian<k>; });
    if (lds > 64 * 1024) {
        const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(kern), (size_t)(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(p.batch), dim3(256), lds, st, p);
    return hipGetLastError();
}

// k_design_ltv: accumulators in registers when the shape allows (nz <= 128, one thread per element of (A, B)), else in LDS
bool ltv_reg_path(const almpc_handle* h) {
    const int n = h->n, m = h->m;
    return h->nz <= LTV_REG_NZ && n * n + n * m <= 1024 - n && design_ltv_reg_lds_doubles(n, m, h->N) * sizeof(double) <= 160 * 1024 &&
           !h->sw.ltv_lds;
}

bool ltv_supported(const almpc_handle* h) {
    return ltv_reg_path(h) || design_ltv_lds_doubles(h->n, h->m, h->N) * sizeof(double) <= 160 * 1024;
}

template <int NC>
hipError_t launch_design_ltv_reg(almpc_handle* h, const DesignLtvParams& lp, size_t lds, hipStream_t st) {
    // 4 x 4 register tiles on 1024 threads.  (8 x 8 tiles on 256 threads, k_design_ltv_reg<NC, 8>, were measured SLOWER -- SQP iteration
    // 0.392 against 0.348 ms: the stage is bound by the latency of its dependent LDS steps, which 16 waves hide better than four, not by
    // LDS bytes -- and are not instantiated)
    if (lds > 64 * 1024) {
        const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(k_design_ltv_reg<NC, 4>), (size_t)(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_design_ltv_reg<NC, 4>), dim3((unsigned)h->batch), dim3(1024), lds, st, lp);
    return hipGetLastError();
}

hipError_t launch_design_ltv(almpc_handle* h, const DesignLtvParams& lp, hipStream_t st) {
    const int n = h->n, m = h->m;
    if (ltv_reg_path(h)) {
        const size_t lds = design_ltv_reg_lds_doubles(n, m, h->N) * sizeof(double);
        switch (n) {
            case 2: return launch_design_ltv_reg<2>(h, lp, lds, st);
            case 4: return launch_design_ltv_reg<4>(h, lp, lds, st);
            case 6: return launch_design_ltv_reg<6>(h, lp, lds, st);
            case 12: return launch_design_ltv_reg<12>(h, lp, lds, st);
            default: return launch_design_ltv_reg<0>(h, lp, lds, st);
        }
    }
    const size_t lds = design_ltv_lds_doubles(n, m, h->N) * sizeof(double);
    if (lds > 64 * 1024) {
        const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(k_design_ltv), (size_t)(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_design_ltv, dim3((unsigned)h->batch), dim3(256), lds, st, lp);
    return hipGetLastError();
}

// whether k_design_instance_t can linearise the network itself (LDS route with room for the weights and one wave's scratch).  An Fnn
// only: a ResNet / PolyNet is linearised by k_fnn_jacobian_w in front of the design (the design kernel keeps its Fnn head and code).
bool design_fuses_fnn(const almpc_handle* h, int H, int L, int net) {
    if (net != NET_FNN) return false;
    const size_t lds = (design_instance_lds_doubles(h->n, h->m, h->N) + fnn_weights_doubles(h->n, h->m, H, L) + fnn_wave_scratch_doubles(h->n, h->m, H, L)) * sizeof(double);
    return lds <= 160 * 1024 && !h->sw.dbg_split_jacobian;
}

// The per-instance design from DEVICE-resident operands (bA, bB, bP; weights dQ, dR, dS, shared or -- ds.Q, ds.R, ds.S -- one set per
// instance): prediction matrices, H_i and F_i, scaling, both inverses, V_i.  Launches only (handle's stream); the caller checks bFlag.
// fuse_fnn: the models are linearisations of this network at fuse_fnn->x / u (re-linearisation pipeline): done by the design kernel's
// own workgroups when *fused comes back true -- else the caller launches the Jacobians first
hipError_t launch_batched_design(almpc_handle* h, const DesignStrides& ds, int useR, int useS, const double* dQ, const double* dR,
                                 const double* dS, double rho, double sigma, bool no_admm, const FnnParams* fuse_fnn = nullptr) {
    const int n = h->n, m = h->m, N = h->N, nz = h->nz, nzs = h->nzs, nrb = h->nrb;
    const int njf = (n + 15) / 16, ps = 16 * njf, gs = nzs;
    const int kr = ((n * N + HESS_KC - 1) / HESS_KC) * HESS_KC;
    const unsigned gb = (unsigned)h->batch;
    hipStream_t st = h->stream;
    size_t inst_lds = design_instance_lds_doubles(n, m, N) * sizeof(double);
    hipError_t e = hipSuccess;
    size_t fnn_off = 0;
    if (fuse_fnn) {   // (the caller has checked design_fuses_fnn)
        fnn_off = design_instance_lds_doubles(n, m, N);
        inst_lds += (fnn_weights_doubles(n, m, fuse_fnn->H, fuse_fnn->L) + fnn_wave_scratch_doubles(n, m, fuse_fnn->H, fuse_fnn->L)) * sizeof(double);
    }
    if (inst_lds > 160 * 1024) {   // (the LDS route below clears the flags itself)
        e = hipMemsetAsync(h->bFlag, 0, (size_t)h->batch * sizeof(int), st);
        if (e != hipSuccess) return e;
    }
    bool scaled = false;
    if (inst_lds <= 160 * 1024) {  // structured route: H_i, F_i from the Toeplitz blocks in LDS, no Gamma panels in HBM
        DesignInstParams dp;
        dp.flag = h->bFlag; dp.sFlag = 1;
        dp.n = n; dp.m = m; dp.N = N; dp.nz = nz; dp.useR = useR; dp.useS = useS;
        dp.A = h->bA; dp.B = h->bB; dp.P = h->bP; dp.sA = ds.A; dp.sB = ds.B; dp.sP = ds.P;
        dp.Q = dQ; dp.R = dR; dp.S = dS; dp.sQ = ds.Q; dp.sR = ds.R; dp.sS = ds.S; dp.H = h->bH; dp.F = h->bF; dp.sH = ds.H; dp.sF = ds.F;
        if (nz <= 128 && design_instance_lds_doubles(n, m, N) >= 128 && !h->sw.dbg_split_scale) {   // the scaling rides along (k_design_scale's body, one launch less)
            dp.d = h->bD; dp.Hs = h->bHs; dp.Fs = h->bFs; dp.sd = ds.d; dp.sHs = ds.Hs; dp.sFs = ds.Fs; dp.nzs = nzs;
        }
        scaled = dp.Hs != nullptr;
        if (fuse_fnn) { dp.fnn_on = 1; dp.fnn_off = fnn_off; dp.fnn = *fuse_fnn; }
#define DESIGN_INST(NC_, MC_)                                                                                \
    do {                                                                                                     \
        e = ensure_dyn_lds(reinterpret_cast<const void*>(k_design_instance_t<NC_, MC_>), inst_lds);          \
        if (e != hipSuccess) return e;                                                                       \
        hipLaunchKernelGGL((k_design_instance_t<NC_, MC_>), dim3(gb), dim3(256), inst_lds, st, dp);          \
    } while (0)
        if (n == 12 && m == 4) DESIGN_INST(12, 4);
        else if (n == 4 && m == 2) DESIGN_INST(4, 2);
        else if (n == 2 && m == 1) DESIGN_INST(2, 1);
        else DESIGN_INST(0, 0);
#undef DESIGN_INST
    } else {
        hipLaunchKernelGGL(k_design_blocks, dim3(1, gb), dim3(256), (size_t)(3 * n * n + n * m) * sizeof(double), st, n, m, N,
                           h->bA, h->bB, h->bPhi, h->bGk, ds);
        hipLaunchKernelGGL(k_design_gamma, dim3(N, gb), dim3(256), 0, st, n, m, N, dQ, h->bP, h->bPhi, h->bGk, h->bGam, h->bW, h->bWP, gs, ps, ds);
        HessParams hp;
        hp.n = n; hp.m = m; hp.N = N; hp.nz = nz; hp.nrb = nrb; hp.njf = njf; hp.kr = kr;
        hp.Gam = h->bGam; hp.W = h->bW; hp.WP = h->bWP; hp.gs = gs; hp.ps = ps; hp.R = dR; hp.S = dS; hp.useR = useR; hp.useS = useS;
        hp.H = h->bH; hp.F = h->bF; hp.st = ds;
        const size_t hess_lds = (size_t)HESS_KC * (16 + (gs + 16) + (ps + 16)) * sizeof(double);
        hipLaunchKernelGGL(k_design_hessian, dim3(nrb, gb), dim3(64 * (nrb + njf)), hess_lds, st, hp);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    DesignStrides ds2 = ds;
    ds2.h_symmetric = (inst_lds <= 160 * 1024) ? 1 : 0;   // (the LDS route writes both halves of H_i from one value)
    launch_batched_factor(h, ds2, rho, sigma, st, no_admm, scaled, true);
    return hipGetLastError();
}

// almpc_design_batched on an ALMPC_FLAG_STRUCTURED handle: one model per instance, structured solve -- models and terminal weights on
// the device, nothing condensed; rho / sigma are not used
int design_batched_structured(almpc_handle* h, const double* A_batch, const double* B_batch, const double* Q, const double* R,
                              const double* S, const double* P, int P_per_instance, const double* umin, const double* umax) {
    if (!A_batch || !B_batch || !Q || !R || !umin || !umax) return fail(h, ALMPC_ERR_INVALID, "design_batched: null matrix pointer");
    const int n = h->n, m = h->m;
    const size_t b = (size_t)h->batch;
    const bool useS = R[0] != 0.0 && S && S[0] != 0.0;
    ALMPC_TRY(begin_redesign(h, 0));
    hm::mat Qm(Q, Q + (size_t)n * n), Rm(R, R + (size_t)m * m), Sm;
    if (useS) Sm = hm::symmetrised(S, m);
    const bool p_inst = P ? (P_per_instance != 0) : true;
    const bool dev_dare = !P && h->terminal_mode == ALMPC_TERMINAL_DARE_DEVICE;   // (k_dare on the uploaded models, below)
    h->t_step = false; h->c_step = false;
    if (model_continuous(h)) ALMPC_TRY(c2d_shape_check(h, "design_batched"));
    hm::mat Pall;
    ALMPC_TRY(terminal_weights(h, A_batch, B_batch, Qm, Rm, P, p_inst, dev_dare, "design_batched", Pall));
    HIP_TRY(h, h->bA.once(b * n * n));
    HIP_TRY(h, h->bB.once(b * n * m));
    HIP_TRY(h, h->bP.once(b * n * n));
    HIP_TRY(h, hipMemcpy(h->bA, A_batch, b * n * n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->bB, B_batch, b * n * m * sizeof(double), hipMemcpyHostToDevice));
    if (model_continuous(h)) ALMPC_TRY(design_c2d_device(h));   // (in place, in front of every reader)
    if (dev_dare) {
        HIP_TRY(h, h->wQ.once((size_t)n * n));
        HIP_TRY(h, h->wR.once((size_t)m * m));
        HIP_TRY(h, hipMemcpy(h->wQ, Qm.data(), Qm.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->wR, Rm.data(), Rm.size() * sizeof(double), hipMemcpyHostToDevice));
        ALMPC_TRY(design_dare_device(h, h->wQ, h->wR, Rm, Pall));
    } else
        HIP_TRY(h, hipMemcpy(h->bP, Pall.data(), Pall.size() * sizeof(double), hipMemcpyHostToDevice));
    h->batched = true; h->ltv = false; h->r_batched_P = true; h->rP_stride = p_inst ? (long)n * n : 0;
    h->bP_stride = h->rP_stride;
    const StateBox box = state_box(h);
    // (one stage of records per instance when the terminal weight is the instance's own DARE solution)
    ALMPC_TRY(setup_structured_solvers(h, nullptr, P == nullptr && !useS, Qm, Rm, useS ? &Sm : nullptr, box));
    if (h->sd.ready) {
        HIP_TRY(h, launch_sgains(h));   // (every instance)
        std::vector<int> bad(b, 0);
        HIP_TRY(h, hipMemcpyAsync(bad.data(), h->sd.bad, b * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < b; ++i)
            if (bad[i]) return fail(h, ALMPC_ERR_NUMERIC, "design_batched: R + B'PB is not positive definite for instance " + std::to_string(i));
    }
    ALMPC_TRY(upload_input_box(h, umin, umax));   // (no umin <= umax check on this route)
    h->P.assign(Pall.begin(), Pall.begin() + (size_t)n * n); h->H.clear(); h->F.clear(); h->d.clear();
    keep_weights(h, nullptr, nullptr, useS ? Sm : hm::mat((size_t)m * m, 0.0), R[0] != 0.0, useS);
    h->has_box = box.min ? 1 : 0;
    h->designed = true;
    return set_zero_reference(h);
}

// ALMPC_DESIGN_TRACE=1: host-side time between the marks of a per-instance design on stderr (where the call spends its wall clock)
struct DesignTrace {
    bool on = false;
    std::chrono::steady_clock::time_point mark = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[almpc design] %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(now - mark).count());
        mark = now;
    }
};

// What the front of a condensed per-instance design leaves its caller: the weights, symmetrised; one terminal weight per instance?
// (dQ, dR, dS: the weights the design kernels read, the handle's shared set or -- ds.Q, ds.R, ds.S -- its per-instance buffers)
struct BatchedDesign {
    hm::mat Qm, Rm, Sm; bool p_inst = true; int useR = 0, useS = 0; DesignStrides ds; DesignTrace tr;
    const double *dQ = nullptr, *dR = nullptr, *dS = nullptr;
};

// almpc_design_batched_weighted: every instance's weights, [batch] matrices each, symmetrised one by one as almpc_design_batched
// symmetrises its single set (S null: no S_batch), in the handle's pinned buffers.  The front's Q, R, S are then instance 0's: the
// branch is the whole batch's.
struct InstanceWeights { const double* Q; const double* R; const double* S; };

// The front of the condensed per-instance designs (almpc_design_batched, almpc_design_ltv): argument checks, weights, terminal weights,
// state rows, the per-instance operands, then models and weights on the device -- continuous-time models discretised in place (k_c2d).
// (What a time-varying design cannot have -- P null, continuous-time models -- its entry point has refused already.)
int batched_design_front(almpc_handle* h, const double* A_batch, const double* B_batch, const double* Q, const double* R, const double* S,
                         const double* P, int P_per_instance, const double* umin, const double* umax, double rho, double sigma, BatchedDesign& d,
                         const InstanceWeights* wi = nullptr) {
    if (!A_batch || !B_batch || !Q || !R || !umin || !umax) return fail(h, ALMPC_ERR_INVALID, "design_batched: null matrix pointer");
    if (!(rho > 0.0) || !(sigma >= 0.0)) return fail(h, ALMPC_ERR_INVALID, "design_batched: rho must be > 0 and sigma >= 0");
    DesignTrace& tr = d.tr;
    tr.on = h->sw.design_trace;
    ALMPC_TRY(begin_redesign(h, DROP_SQP | DROP_RELIN));
    const int n = h->n, m = h->m;
    const size_t b = (size_t)h->batch;
    ALMPC_TRY(check_input_box(h, umin, umax, "design_batched"));
    d.Qm = hm::symmetrised(Q, n); d.Rm = hm::symmetrised(R, m); d.Sm = hm::symmetrised(S, m);
    const hm::mat &Qm = d.Qm, &Rm = d.Rm, &Sm = d.Sm;
    const bool p_inst = d.p_inst = P ? (P_per_instance != 0) : true;
    // (almpc_set_terminal_weight: k_dare on the uploaded models instead of the host loop, behind the uploads below; its P_i are symmetric)
    const bool dev_dare = !P && h->terminal_mode == ALMPC_TERMINAL_DARE_DEVICE;
    h->t_step = false; h->c_step = false;
    const bool cont = model_continuous(h);   // (almpc_set_model_time: k_c2d in place on the uploaded models, below)
    if (cont) ALMPC_TRY(c2d_shape_check(h, "design_batched"));
    hm::mat Pall;
    ALMPC_TRY(terminal_weights(h, A_batch, B_batch, Qm, Rm, P, p_inst, dev_dare, "design_batched", Pall, wi ? wi->Q : nullptr, wi ? wi->R : nullptr));
    for (size_t i = 0; i < (dev_dare ? 0 : p_inst ? b : 1); ++i) {
        const hm::mat Pm = hm::symmetrised(Pall.data() + i * n * n, n);
        std::copy(Pm.begin(), Pm.end(), Pall.begin() + i * n * n);
    }
    if (!dev_dare) h->P.assign(Pall.begin(), Pall.begin() + (size_t)n * n);
    h->rho = rho; h->sigma = sigma;
    d.useR = Rm[0] != 0.0; d.useS = d.useR && Sm[0] != 0.0;
    keep_weights(h, &Qm, &Rm, Sm, d.useR, d.useS);
    tr("host preparation");
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    tr("stream idle");
    // state rows (almpc_set_state_box, almpc_set_terminal_equality): one constraint-space matrix per instance
    ALMPC_TRY(setup_state_rows(h, state_box(h).min, state_box(h).max, true));
    ALMPC_TRY(ensure_batched_alloc(h));
    hipStream_t st = h->stream;
    tr("state rows + allocation");
    if (!wi) {
        HIP_TRY(h, h->wQ.once((size_t)n * n));
        HIP_TRY(h, h->wR.once((size_t)m * m));
        HIP_TRY(h, h->wS.once((size_t)m * m));
    } else {   // one set per instance: buffers of their own, made here and nowhere else
        HIP_TRY(h, h->wiQ.grow(b * n * n));
        HIP_TRY(h, h->wiR.grow(b * m * m));
        if (wi->S) HIP_TRY(h, h->wiS.grow(b * m * m));
    }
    const bool s_given = !wi || wi->S;
    double *dQ = wi ? h->wiQ.get() : h->wQ.get(), *dR = wi ? h->wiR.get() : h->wR.get();   // (kept with the handle: three hipMalloc + hipFree per design cost 0.15 ms)
    double* dS = !wi ? h->wS.get() : s_given ? h->wiS.get() : nullptr;
    const double *Qup = wi ? wi->Q : Qm.data(), *Rup = wi ? wi->R : Rm.data(), *Sup = wi ? wi->S : Sm.data();
    const size_t qn = wi ? b * n * n : Qm.size(), rn = wi ? b * m * m : Rm.size(), sn = wi ? b * m * m : Sm.size();
    HIP_TRY(h, hipMemcpyAsync(h->bA, A_batch, b * n * n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->bB, B_batch, b * n * m * sizeof(double), hipMemcpyHostToDevice, st));
    if (!dev_dare) HIP_TRY(h, hipMemcpyAsync(h->bP, Pall.data(), Pall.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(dQ, Qup, qn * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(dR, Rup, rn * sizeof(double), hipMemcpyHostToDevice, st));
    if (s_given) HIP_TRY(h, hipMemcpyAsync(dS, Sup, sn * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemsetAsync(h->bFlag, 0, b * sizeof(int), st));
    tr("weights alloc + copies queued");
    h->bP_stride = p_inst ? (long)n * n : 0;
    if (cont) {
        ALMPC_TRY(design_c2d_device(h));
        tr("k_c2d");
    }
    if (dev_dare) {
        ALMPC_TRY(design_dare_device(h, dQ, dR, Rm, h->P, wi ? (long)n * n : 0, wi ? (long)m * m : 0));
        tr("k_dare");
    }
    d.ds = batched_strides(h, p_inst);
    if (wi) { d.ds.Q = (long)n * n; d.ds.R = (long)m * m; d.ds.S = s_given ? (long)m * m : 0; }
    d.dQ = dQ; d.dR = dR; d.dS = dS;
    return ALMPC_OK;
}

// ... and behind their kernels: the flags and the host copies of instance 0 (almpc_get_design; every instance:
// almpc_get_design_instance) read back, a flagged instance reported, the input box uploaded
int batched_design_readback(almpc_handle* h, BatchedDesign& d, const double* umin, const double* umax) {
    const int n = h->n, nz = h->nz, nzs = h->nzs;
    const size_t b = (size_t)h->batch;
    hipStream_t st = h->stream;
    d.tr("kernels queued");
    std::vector<int> flags(b, 0);
    HIP_TRY(h, hipMemcpyAsync(flags.data(), h->bFlag, b * sizeof(int), hipMemcpyDeviceToHost, st));
    h->H.assign((size_t)nz * nz, 0.0); h->F.assign((size_t)nz * n, 0.0); h->d.assign((size_t)nzs, 0.0);
    HIP_TRY(h, hipMemcpyAsync(h->H.data(), h->bH, h->H.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(h->F.data(), h->bF, h->F.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(h->d.data(), h->bD, h->d.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    d.tr("device done");
    for (size_t i = 0; i < b; ++i)
        if (flags[i] != 0)
            return fail(h, ALMPC_ERR_NUMERIC, "design_batched: instance " + std::to_string(i) +
                        (flags[i] == 1 ? ": condensed Hessian has a non-positive diagonal" : ": Cholesky pivot not positive"));
    return upload_input_box(h, umin, umax);
}

// almpc_design_batched on a condensed handle: every instance gets its own condensed QP from (A_i, B_i).  The design kernels of
// almpc_design.hip.h run with blockIdx.y = instance; the per-step path is k_admm_inst + k_polish<false> with strides.
int design_batched_condensed(almpc_handle* h, const double* A_batch, const double* B_batch, const double* Q, const double* R, const double* S,
                             const double* P, int P_per_instance, const double* umin, const double* umax, double rho, double sigma,
                             const InstanceWeights* wi = nullptr) {
    BatchedDesign d;
    ALMPC_TRY(batched_design_front(h, A_batch, B_batch, Q, R, S, P, P_per_instance, umin, umax, rho, sigma, d, wi));
    const DesignStrides& ds = d.ds;
    const int n = h->n, useR = d.useR, useS = d.useS;
    HIP_TRY(h, launch_batched_design(h, ds, useR, useS, d.dQ, d.dR, d.dS, rho, sigma, false));
    if (h->mc > 0) HIP_TRY(h, launch_ghat_inst(h, nullptr, nullptr));
    ALMPC_TRY(batched_design_readback(h, d, umin, umax));
    h->sd.ready = false;
    // (per-instance weights: the stage-wise solvers take shared weights, so no redo covers this design -- run_step, step_redo)
    h->weighted = wi != nullptr; h->wiS_given = wi && wi->S;
    if (h->fallback && !wi) {
        h->r_batched_P = true; h->rP_stride = d.p_inst ? (long)n * n : 0;
        // (one stage of records per instance when the terminal weight is the instance's own DARE solution; the stage records are
        // computed when a step leaves instances to redo, for those instances only: nothing here)
        ALMPC_TRY(setup_redo_solvers(h, nullptr, P == nullptr && !useS, d.Qm, d.Rm, useS ? &d.Sm : nullptr, state_box(h), h->fallback == 1,
                                     "structured fallback: state rows / input-rate weight need n + m <= 48 and (N + 1)(n + m) <= 4096"));
    }
    h->designed = true; h->batched = true; h->ltv = false;
    const int rc = set_zero_reference(h);
    d.tr("flags + set_reference");
    return rc;
}

// almpc_design_ltv (a condensed handle): the per-instance design from stage models.  The QP variable is v = u - ubar, so ubar takes
// the place of the input reference (bounds umin - ubar <= v, u = v + ubar); the gradient is the explicit vector q_i (F'_i = V_i = 0:
// the step kernels add nothing for e0).  No redo by the stage-wise solvers.
int design_ltv_condensed(almpc_handle* h, const double* A_batch, const double* B_batch, const double* Q, const double* R, const double* S,
                         const double* P, int P_per_instance, const double* umin, const double* umax, double rho, double sigma,
                         const LtvInputs& ltv) {
    BatchedDesign d;
    ALMPC_TRY(batched_design_front(h, A_batch, B_batch, Q, R, S, P, P_per_instance, umin, umax, rho, sigma, d));
    const DesignStrides& ds = d.ds;
    const int n = h->n, m = h->m, N = h->N, nz = h->nz, nzs = h->nzs;
    const size_t b = (size_t)h->batch;
    hipStream_t st = h->stream;
    double *dQ = h->wQ, *dR = h->wR, *dS = h->wS;
    hipError_t e;
    {
        DevBuf<double> dAll, dBll, dC, dE, dQa;  // LTV staging (released at the end of this block)
        e = dAll.upload_async(ltv.A_all, b * N * n * n, st);
        if (e == hipSuccess) e = dBll.upload_async(ltv.B_all, b * N * n * m, st);
        if (e == hipSuccess && ltv.c_all) e = dC.upload_async(ltv.c_all, b * N * n, st);
        if (e == hipSuccess) e = dE.upload_async(ltv.ebar, b * N * n, st);
        if (e == hipSuccess) e = dQa.upload_async(ltv.qadd, b * nz, st);
        if (e == hipSuccess) e = h->bQ.once(b * nz);
        if (e == hipSuccess) e = hipMemsetAsync(h->bF, 0, b * nz * n * sizeof(double), st);
        if (e == hipSuccess) {
            DesignLtvParams lp;
            lp.n = n; lp.m = m; lp.N = N; lp.nz = nz; lp.useR = d.useR; lp.useS = d.useS;
            lp.A = dAll; lp.B = dBll; lp.c = dC; lp.ebar = dE; lp.P = h->bP; lp.sP = ds.P; lp.Q = dQ; lp.R = dR; lp.S = dS;
            lp.qadd = dQa; lp.H = h->bH; lp.q = h->bQ;
            e = launch_design_ltv(h, lp, st);
        }
        if (e == hipSuccess && h->mc > 0) {   // (needs G_i, d_i: the factor step comes first when there are state rows)
            launch_batched_factor(h, ds, rho, sigma, st, false);
            e = launch_ghat_inst(h, dAll, dBll);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);  // the staging buffers are released right away
        h->lA.reset(); h->lB.reset(); h->lC.reset(); h->lE.reset();
        if (e == hipSuccess && h->mc > 0) {   // ... except with state rows: the step rolls the stage models out
            h->lA = std::move(dAll); h->lB = std::move(dBll); h->lC = std::move(dC); h->lE = std::move(dE);
        } else if (e == hipSuccess && h->cert.keep) {   // ... or for almpc_certificate_ltv (almpc_set_keep_stage_models)
            h->lA = std::move(dAll); h->lB = std::move(dBll); h->lC = std::move(dC);
        }
    }
    if (e != hipSuccess) return fail(h, ALMPC_ERR_HIP, std::string("design_ltv: ") + hipGetErrorString(e));
    if (h->mc == 0) launch_batched_factor(h, ds, rho, sigma, st, false);
    launch_neg_gm_batched(st, (unsigned)b, nz, nzs, n, h->bG, h->bFs, h->bVs, ds.G, ds.Fs);
    HIP_TRY(h, hipGetLastError());
    ALMPC_TRY(batched_design_readback(h, d, umin, umax));
    h->sd.ready = false;
    h->designed = true; h->batched = true; h->ltv = false;
    const int rc = almpc_set_reference(h, ltv.xbar, ltv.ubar, 1);
    if (rc != ALMPC_OK) { h->designed = false; return rc; }
    h->designed = false;  // until the explicit gradient below is in place
    hipLaunchKernelGGL(k_fs_scale, dim3(256), dim3(256), 0, h->stream, h->batch, nz, nzs, h->bQ, (long)nz, h->bD, h->dFS);
    hipLaunchKernelGGL(k_neg_gm, dim3(1, (unsigned)h->batch), dim3(256), 0, h->stream, nz, nzs, 1, nz, h->bG, h->dFS, h->dV0S,
                       (long)nz * nzs, (long)nz);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->cert.keep) {   // the shared references beside the kept stage models (xbar, ubar are the reference buffers already)
        std::vector<double> xr((size_t)n * (N + 1), 0.0), ur((size_t)nz, 0.0);
        if (ltv.xref) xr.assign(ltv.xref, ltv.xref + xr.size());
        if (ltv.uref) ur.assign(ltv.uref, ltv.uref + ur.size());
        HIP_TRY(h, h->cert.xref.upload(xr.data(), xr.size()));
        HIP_TRY(h, h->cert.uref.upload(ur.data(), ur.size()));
        h->cert.kept = true; h->cert.kept_c = ltv.c_all != nullptr;
    }
    h->ltv = true;
    h->designed = true;
    return ALMPC_OK;
}

// ---- the step (almpc_calculate_async, and the SQP loop / re-linearisation pipeline on their own designs) -------------------------

// Where the working-set guess of a per-instance step comes from: the ADMM phase, or -- no ADMM phase, no KKT inverse in the design --
// the SQP loop's iterate, or the previous step's inputs shifted by one stage (warm steps of the re-linearisation pipeline)
enum class Guess { Admm, FromIterate, ShiftInputs };
struct StepMode {
    Guess guess = Guess::Admm;
    bool fold_flag = false;        // (re-linearisation step) the finish turns a flagged design into ALMPC_NON_FINITE itself
    RowMultOut rows;               // (SQP loop with almpc_sqp_fnn_set_row_multipliers) the state-row finish hands its multipliers out
};

// Timing events of a step (ALMPC_FLAG_TIMING): 0 start, 1 end of the ADMM phase, 2 end of the finish, 3 end.  Event 0 is recorded in
// front of the step's first launch -- unless the step turns out to be ONE kernel: then only the pair around that kernel is recorded
// (an event record costs ~3.5 us of stream time: four of them are 5 % of such a step)
struct StepTimer {
    hipEvent_t* ev = nullptr;   // null: this step is not timed
    hipStream_t st = nullptr;
    bool started = false;
    hipError_t open(almpc_handle* h) {
        st = h->stream;
        if (!(h->flags & ALMPC_FLAG_TIMING) || (h->step_count++ % (size_t)h->timing_stride) != 0) return hipSuccess;
        if (h->ev.size() < 4 * (h->ev_used + 1)) {
            const size_t old = h->ev.size();
            h->ev.resize(old + 4 * 64, nullptr);
            for (size_t i = old; i < h->ev.size(); ++i) {
                const hipError_t e = hipEventCreate(&h->ev[i]);
                if (e != hipSuccess) return e;
            }
        }
        ev = &h->ev[4 * h->ev_used];
        if (h->ev_two.size() < h->ev_used + 1) h->ev_two.resize(h->ev_used + 64, 0);
        return hipSuccess;
    }
    hipError_t start() {
        if (!ev || started) return hipSuccess;
        started = true;
        return hipEventRecord(ev[0], st);
    }
    hipError_t mark(int i) const { return ev ? hipEventRecord(ev[i], st) : hipSuccess; }
    hipError_t close(almpc_handle* h) const {
        if (!ev) return hipSuccess;
        if (started) {
            const hipError_t e = hipEventRecord(ev[3], st);
            if (e != hipSuccess) return e;
        }
        h->ev_two[h->ev_used] = started ? 0 : 1;
        h->ev_used += 1;
        return hipSuccess;
    }
};

// What every route of one condensed step shares
struct Step {
    almpc_handle* h;
    almpc_opts o;
    StepMode mode;
    bool keep_state, lazy_redo;
    StepTimer t;
    RollGeom roll;
    RolloutParams rp;
};

// Operands of the per-instance ADMM (k_admm_inst, k_step_inst_wave, the guess kernels): the handle's per-instance models, or with
// `shared` the dense shared design [Minv | H' | F' | V] that every instance reads (operand strides 0)
AdmmInstParams admm_inst_params(const almpc_handle* h, const almpc_opts& o, bool shared) {
    AdmmInstParams ip;
    ip.nz = h->nz; ip.n = h->n; ip.m = h->m; ip.batch = h->batch; ip.nzs = h->nzs;
    if (shared) {
        const size_t mm = (size_t)h->nz * h->nzs, fv = (size_t)h->n * h->nzs;
        ip.Minv = h->dPlain; ip.Hs = h->dPlain + mm; ip.Fs = h->dPlain + 2 * mm; ip.Vs = h->dPlain + 2 * mm + fv;
        ip.dvec = h->dD; ip.rhovec = h->dRho;
        ip.mat_stride = 0; ip.fv_stride = 0; ip.vec_stride = 0; ip.fs_stride = h->fS_stride;
    } else {
        ip.Minv = h->bMinv; ip.Hs = h->bHs; ip.Fs = h->bFs; ip.Vs = h->bVs; ip.dvec = h->bD; ip.rhovec = h->bRho;
        ip.mat_stride = (long)h->nz * h->nzs; ip.fv_stride = (long)h->n * h->nzs; ip.vec_stride = h->nzs; ip.fs_stride = h->nz;
    }
    ip.fS = h->dFS; ip.v0S = h->dV0S; ip.umin = h->dUmin; ip.umax = h->dUmax;
    ip.uref = h->dUref; ip.uref_stride = h->uref_stride; ip.xref = h->dXref; ip.xref_stride = h->xref_stride; ip.x0 = h->dX0;
    ip.xs = h->dXs; ip.zs = h->dZs; ip.ys = h->dYs; ip.v0 = h->dV0; ip.status = h->dStatus; ip.iters = h->dIters;
    ip.piters = h->dPiters; ip.perm = h->dPerm;
    ip.sigma = o.sigma; ip.alpha = o.alpha; ip.eps_abs = o.eps_abs; ip.eps_rel = o.eps_rel;
    ip.max_iter = o.max_iter; ip.check_every = o.check_every; ip.warm = o.warm_start ? 1 : 0;
    return ip;
}

// Operands of the shared model's ADMM tile kernel (k_admm, the ADMM phase of k_step_fused)
AdmmParams admm_params(const almpc_handle* h, const almpc_opts& o, bool keep_state) {
    AdmmParams ap;
    ap.nz = h->nz; ap.n = h->n; ap.m = h->m; ap.batch = h->batch; ap.nzs = h->nzs;
    ap.MinvFrag = h->dMinvFrag; ap.VFrag = h->dVFrag; ap.v0S = h->dV0S; ap.v0S_stride = h->fS_stride; ap.HFrag = h->dHFrag; ap.FFrag = h->dFFrag; ap.ksf = h->ksf;
    ap.dvec = h->dD; ap.rhovec = h->dRho; ap.umin = h->dUmin; ap.umax = h->dUmax;
    ap.uref = h->dUref; ap.uref_stride = h->uref_stride; ap.xref = h->dXref; ap.xref_stride = h->xref_stride;
    ap.fS = h->dFS; ap.fS_stride = h->fS_stride; ap.x0 = h->dX0;
    if (h->dCold && h->cold_ref && h->uref_stride == 0 && h->fS_stride == 0) {
        const size_t w = (size_t)h->n * h->nzs;
        ap.rowc = h->dCold + w + h->nzs;
        if (!(o.reserved[0] & ALMPC_OPT_FULL_FIRST_PRODUCT)) ap.Wp = h->dCold;
    }
    ap.xs = h->dXs; ap.zs = h->dZs; ap.ys = h->dYs; ap.v0 = h->dV0; ap.status = h->dStatus; ap.iters = h->dIters;
    ap.piters = h->dPiters;
    ap.perm = h->dPerm;
    ap.rho = o.rho; ap.sigma = o.sigma; ap.alpha = o.alpha; ap.eps_abs = o.eps_abs; ap.eps_rel = o.eps_rel;
    ap.max_iter = o.max_iter; ap.check_every = o.check_every; ap.warm = o.warm_start ? 1 : 0;
    ap.keep_state = keep_state ? 1 : 0; ap.yflags = h->dYflags;
    return ap;
}

size_t admm_lds_bytes(const almpc_handle* h) {
    return ((size_t)2 * h->nzs * TILE + (size_t)h->nrb * 8 * TILE + (size_t)4 * h->ksf * TILE) * sizeof(double);
}

// The rollout of every instance from its inputs rp.w: x, e_x, u, e_u
RolloutParams rollout_params(const almpc_handle* h) {
    RolloutParams rp;
    rp.n = h->n; rp.m = h->m; rp.N = h->N; rp.batch = h->batch; rp.nzs = h->nzs; rp.A = h->batched ? h->bA : h->dA; rp.B = h->batched ? h->bB : h->dB;
    rp.dvec = h->dD; rp.w = h->dZs; rp.x0 = h->dX0; rp.xref = h->dXref; rp.xref_stride = h->xref_stride;
    rp.uref = h->dUref; rp.uref_stride = h->uref_stride; rp.umin = h->dUmin; rp.umax = h->dUmax; rp.x = h->dX; rp.ex = h->dEx; rp.u = h->dU; rp.eu = h->dEu;
    return rp;
}

// LDS layout of the input-box finish (k_polish*, k_step_*)
struct PolishLayout {
    PolishShared SL;                 // workgroup-shared part
    bool fused = false;              // the rollout runs in the finish's tail
    int fuse_rollout = 0;            // PolishParams::fuse_rollout
    int per_wave = 0;                // doubles per wave
    int wave_const_off = -1;         // per-instance models: the wave's copy of d_i | [A_i B_i] behind its buffers
    int sg_shared_off = -1;          // the workgroup-shared second-tier slot, or -1
    size_t g_lds = 0;                // doubles of G in LDS (rows packed to an even stride)
    size_t l_glds = 0, l_step = 0;   // bytes of k_polish<true> (G in LDS), of k_step_fused
};

PolishLayout polish_layout(const almpc_handle* h, const RollGeom& roll) {
    PolishLayout L;
    const bool blocked = !h->batched && h->roll_s > 0;   // shared model: blocked rollout, no trajectory buffer
    L.fused = roll.fits || blocked;   // (rollout fused into the tail of the finish when its trajectory buffer fits the wave's LDS slot)
    L.fuse_rollout = L.fused ? (h->ltv ? 2 : (blocked ? 3 : 1)) : 0;
    int per_wave = POLISH_LDS_MIN_PER_WAVE;
    if (L.fused && !blocked && (h->N + 1) * (h->n + h->m) > per_wave) per_wave = (h->N + 1) * (h->n + h->m);
    per_wave = (per_wave + 1) & ~1;
    if (h->batched) {
        L.wave_const_off = per_wave;
        per_wave += (h->nzs + h->n * (h->n + h->m) + 1) & ~1;
    }
    L.per_wave = per_wave;
    // G in LDS when it fits beside the buffers of 8 waves (gfx950: 160 KB per workgroup)
    L.SL = polish_shared_layout(h->n, h->m, h->N, h->nz, h->nzs, L.fuse_rollout);
    L.g_lds = (size_t)h->nz * ((h->nz + 1) & ~1);
    L.l_glds = (L.g_lds + L.SL.total + (size_t)POLISH_WAVES_GLDS * per_wave + 2) * sizeof(double);
    // workgroup-shared second-tier slot (working sets beyond 32 rows) behind the queue words, if the 160 KB allow it
    const size_t slot = (size_t)POLISH_SG_SHARED_CAP * 64 * sizeof(double);
    if (L.l_glds + slot <= 160 * 1024 && !h->batched && !h->sw.polish_sg_global) {
        L.sg_shared_off = (int)(L.SL.total + (size_t)POLISH_WAVES_GLDS * per_wave + 2);
        L.l_glds += slot;
    }
    // one kernel for the whole step: [G | union(ADMM buffers, finish buffers)]
    L.l_step = L.l_glds - L.g_lds * sizeof(double);
    if (admm_lds_bytes(h) > L.l_step) L.l_step = admm_lds_bytes(h);
    L.l_step += L.g_lds * sizeof(double);
    return L;
}

// The finish's parameters on the standard layout (the routes adjust the LDS offsets of their kernel)
PolishParams polish_params(const Step& s, const PolishLayout& L) {
    const almpc_handle* h = s.h;
    PolishParams pp;
    pp.nz = h->nz; pp.m = h->m; pp.batch = h->batch; pp.nzs = h->nzs;
    pp.G = h->batched ? h->bG : h->dG; pp.dvec = h->batched ? h->bD : h->dD;
    pp.G_stride = h->batched ? (long)h->nz * h->nzs : 0; pp.d_stride = h->batched ? (long)h->nzs : 0;
    pp.A_stride = h->batched ? (long)h->n * h->n : 0; pp.B_stride = h->batched ? (long)h->n * h->m : 0;
    pp.wave_const_off = L.wave_const_off; pp.sg_off = 0; pp.g_off = 0; pp.sg_shared_off = L.sg_shared_off;
    pp.umin = h->dUmin; pp.umax = h->dUmax; pp.uref = h->dUref; pp.uref_stride = h->uref_stride;
    pp.zs = h->dZs; pp.ys = h->dYs; pp.v0 = h->dV0; pp.w = h->dW; pp.status = h->dStatus; pp.piters = h->dPiters;
    pp.yflags = s.keep_state ? nullptr : h->dYflags; pp.yflag_words = h->nrb;
    pp.sglobal = h->dSglobal; pp.perm = h->dPerm; pp.ntiles = (h->batch + 15) / 16;
    pp.max_iter = s.o.polish_max_iter > 0 ? s.o.polish_max_iter : 2 * h->nz + 50;
    pp.dflag = s.mode.fold_flag ? h->bFlag : nullptr;
    if (s.lazy_redo) { pp.unsolved = h->redo.dUnsolved; pp.redo_gate = h->redo.dGate; pp.step_serial = h->redo.step_serial; }
    pp.fuse_rollout = L.fuse_rollout; pp.roll_g = s.roll.g; pp.roll_cpl = s.roll.cpl; pp.roll = s.rp;
    pp.rollM = h->dRollM; pp.roll_s = h->roll_s; pp.roll_nb = h->roll_nb;
    pp.lds_per_wave = L.per_wave;
    return pp;
}

enum class Route { StateRows, FusedShared, WaveShared, WaveInst, TwoLaunch, NoPolish };

Route pick_route(const Step& s, const PolishLayout& L) {
    const almpc_handle* h = s.h;
    if (h->mc > 0) return Route::StateRows;
    if (!s.o.polish) return Route::NoPolish;
    if (!h->batched && h->fuse_step && POLISH_WAVES_GLDS == 8 && !h->sw.polish_no_glds && h->nrb == 8 && (h->ks == 30 || h->ks == 32) && L.fused &&
        L.l_step <= 160 * 1024)
        return Route::FusedShared;
    // small SHARED problems in small batches (configs[0], the reference's own test sizes: one instance, N 5 - 15, m 2 -> nz 10 - 30;
    // round 5): the two-launch path gives them a 16-instance MFMA tile they cannot fill and two launch ramps.  ONE kernel, one wave per
    // instance -- k_step_inst_wave with operand strides of zero: every wave reads the same dense Minv / F' / V (a few KB, L1 / L2
    // resident), runs the ADMM iterations from registers and then the single-wave finish (G through L1: 13 KB at nz 40).  Measured
    // (tools/time_small_shared.py, QTP fixture, N 5 / N 20, us per step): batch 1 16.9 / 21.8 against 29.7 / 33.1, batch 64 20 / 45
    // against 43 / 56, batch 512 30 / 58 against 44 / 58; from 2048 instances on a wave per 10 - 40-row problem wastes the machine
    // (63 / 113 against 45 / 70 us; 65,536: 1.8 / 2.3 ms against 0.32 / 0.68 ms): up to two instances per CU take this path, larger
    // batches the tile path.
    if (!h->batched && h->nzs <= 64 && L.fused && h->dPlain && !h->ltv && !h->sw.no_shared_wave &&
        (long)h->batch <= h->sw.shared_wave_max_batch.value_or((long)2 * h->num_cus) && ((size_t)L.SL.total + (size_t)L.per_wave) * sizeof(double) <= 64 * 1024)
        return Route::WaveShared;
    // small per-instance problems (BASELINE configs[3]): ONE wave per instance for the whole step -- ADMM with the KKT inverse in
    // registers, then the single-wave finish with G_i in the wave's LDS (the second-tier Sinv, rarely needed at these sizes, stays in the
    // global scratch: with its 32 KB per wave only three waves would fit a CU)
    if (h->batched && s.mode.guess == Guess::Admm && h->nzs <= 64 && L.fused && !h->sw.no_inst_wave &&
        ((size_t)L.SL.total + (size_t)L.per_wave + (size_t)h->nz * h->nzs) * sizeof(double) <= 64 * 1024)
        return Route::WaveInst;
    return Route::TwoLaunch;
}

template <bool PACKED>
hipError_t launch_admm_inst(const AdmmInstParams& ip, int wgs, size_t lds, hipStream_t st) {
    if (lds > 64 * 1024) {
        const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(k_admm_inst<PACKED>), lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_admm_inst<PACKED>), dim3(wgs), dim3(ADMM_INST_THREADS), lds, st, ip);
    return hipGetLastError();
}

// The ADMM phase (the shared model's tile kernel, or k_admm_inst on per-instance models) or the per-instance guess that replaces it
// (StepMode::guess), between timing events 0 and 1.  *guess_ws: k_guess_iterate_ws also left the inverse of the guessed working set
// (installed by k_polish_sgl<1>)
int step_admm_or_guess(Step& s, bool* guess_ws = nullptr) {
    almpc_handle* h = s.h;
    hipStream_t st = h->stream;
    HIP_TRY(h, s.t.start());
    if (!h->batched) {
        HIP_TRY(h, launch_admm(h->nrb, h->ks, admm_params(h, s.o, s.keep_state), (h->batch + TILE - 1) / TILE, admm_lds_bytes(h), st));
        HIP_TRY(h, s.t.mark(1));
        return ALMPC_OK;
    }
    AdmmInstParams ip = admm_inst_params(h, s.o, false);
    if (s.mode.guess == Guess::ShiftInputs) {
        hipLaunchKernelGGL(k_guess_shift, dim3((h->batch + 3) / 4), dim3(256), 0, st, ip, (const double*)h->dU, h->N);
    } else if (s.mode.guess == Guess::FromIterate && h->nzs <= 128 && h->nzs > 64 && h->batch <= 2 * h->num_cus && h->dSglobal && h->bG &&
               !h->sw.no_guess_ws) {
        // the guess of an SQP iteration AND the inverse of its working set (33..64 of the inputs on a bound), four waves per instance
        HIP_TRY(h, h->dStartRows.once((size_t)h->batch * 65));
        GuessWsParams gw;
        gw.G = h->bG; gw.G_stride = (long)h->nz * h->nzs; gw.sinv = h->dSglobal; gw.rows = h->dStartRows;
        hipLaunchKernelGGL(k_guess_iterate_ws, dim3((unsigned)h->batch), dim3(256), 0, st, ip, gw);
        if (guess_ws) *guess_ws = true;
    } else if (s.mode.guess == Guess::FromIterate) {
        hipLaunchKernelGGL(k_guess_iterate, dim3((h->batch + 3) / 4), dim3(256), 0, st, ip);
    } else {
        // KKT inverse in LDS; persistent grid: as many workgroups as fit the CUs at once -- register bound: 2 x 256 threads at up to 256
        // VGPRs each fill the CU's register file
        const bool packed = h->minv_packed;
        const size_t l = admm_inst_lds_doubles(h->nz, h->nzs, h->m, packed) * sizeof(double);
        const int wgs = h->num_cus * 2 > h->batch ? h->batch : h->num_cus * 2;
        ip.minv_stride = packed ? packed_tri_doubles(h->nz) : 0;
        HIP_TRY(h, packed ? launch_admm_inst<true>(ip, wgs, l, st) : launch_admm_inst<false>(ip, wgs, l, st));
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, s.t.mark(1));
    return ALMPC_OK;
}

// The rollout on its own, behind a finish that did not run it in its tail
int step_rollout(Step& s) {
    almpc_handle* h = s.h;
    RolloutParams& rp = s.rp;
    const size_t per_wave = (size_t)h->n * (h->N + 1) + h->nz, shared = (size_t)h->n * h->n + (size_t)h->n * h->m;
    if (h->batched) { rp.A_stride = (long)h->n * h->n; rp.B_stride = (long)h->n * h->m; rp.d_stride = h->nzs; rp.dvec = h->bD; }
    if (!h->batched && (shared + 4 * per_wave) * sizeof(double) <= 60 * 1024) {
        const size_t l = (shared + 4 * per_wave) * sizeof(double);
        hipLaunchKernelGGL((k_rollout<4>), dim3((h->batch + 3) / 4), dim3(256), l, h->stream, rp);
    } else {  // long horizons with many states: one instance per workgroup, LDS beyond the 64 KiB default
        const size_t l = (shared + per_wave) * sizeof(double);
        HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_rollout<1>), l));
        hipLaunchKernelGGL((k_rollout<1>), dim3(h->batch), dim3(64), l, h->stream, rp);
    }
    HIP_TRY(h, hipGetLastError());
    return ALMPC_OK;
}

template <int NP>
hipError_t launch_polish_gen(const almpc_handle* h, const PolishGenParams& gp) {
    // first launch: working sets up to 32 rows, every instance; second launch: the instances the first one flagged, up to 64 rows
    const size_t l32 = (size_t)PGEN_WAVES * pgen_lds_per_wave(32) * sizeof(double);
    const size_t l64 = (size_t)pgen_coop_lds_doubles() * sizeof(double);   // (wave 0's buffers + job word + three partial sums)
    hipLaunchKernelGGL((k_polish_gen<NP>), dim3((h->batch + PGEN_WAVES - 1) / PGEN_WAVES), dim3(64 * PGEN_WAVES), l32, h->stream, gp);
    const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(k_polish_gen64<NP>), l64);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_polish_gen64<NP>), dim3(3 * h->num_cus < h->batch ? 3 * h->num_cus : h->batch), dim3(64 * (PGEN_HELPERS + 1)), l64,
                       h->stream, gp);
    return hipGetLastError();
}

// State rows (state box / terminal equality): the ADMM phase or a guess, then the state-row finish k_polish_gen + k_polish_gen64 with
// the rollout in its tail
int step_state_rows(Step& s) {
    almpc_handle* h = s.h;
    const almpc_opts& o = s.o;
    if (!s.roll.fits) return fail(h, ALMPC_ERR_UNSUPPORTED, "calculate: state rows need the fused rollout (n + m <= 8 * lanes-per-row)");
    if (h->batched && !h->ghat_inst) return fail(h, ALMPC_ERR_NOT_DESIGNED, "calculate: state rows without their per-instance matrices");
    const bool sq = h->sqp.ready;
    if (h->ltv && !(sq ? h->sqp.A && h->sqp.B : h->lA && h->lB))
        return fail(h, ALMPC_ERR_NOT_DESIGNED, "calculate: state rows of a time-varying design without its stage models");
    { const int rc = step_admm_or_guess(s); if (rc != ALMPC_OK) return rc; }
    PolishGenParams gp;
    gp.nz = h->nz; gp.mc = h->mc; gp.R = h->R; gp.Rs = h->Rs; gp.m = h->m; gp.n = h->n; gp.N = h->N; gp.batch = h->batch; gp.nzs = h->nzs;
    if (h->ltv) {
        gp.ltv = 1;
        gp.ltvA = sq ? h->sqp.A : h->lA; gp.ltvB = sq ? h->sqp.B : h->lB; gp.ltvC = sq ? h->sqp.c : h->lC;
        if (h->terminal_eq) { gp.eq_off = (sq ? h->sqp.ebar : h->lE) + (size_t)(h->N - 1) * h->n; gp.eq_stride = (long)h->N * h->n; }
    }
    if (h->batched) {
        gp.Ghat_stride = (long)h->R * h->Rs; gp.gnorm_stride = h->Rs; gp.d_stride = h->nzs;
        gp.A_stride = (long)h->n * h->n; gp.B_stride = (long)h->n * h->m;
    }
    if (!h->batched && h->roll_s > 0) { gp.rollM = h->dRollM; gp.roll_s = h->roll_s; gp.roll_nb = h->roll_nb; }
    if (h->eq_proj && !h->batched) { gp.eq_proj = 1; gp.eq0 = h->R - h->n; gp.ne = h->n; gp.GhatE = h->dGhatE; gp.WinvE = h->dWinvE; }
    gp.Ghat = h->dGhat; gp.gnorm = h->dGnorm; gp.row_traj = h->dRowTraj; gp.row_eq = h->dRowEq; gp.row_xidx = h->dRowXidx;
    gp.row_state = h->dRowState; gp.xmin = h->dXmin; gp.xmax = h->dXmax; gp.has_box = h->has_box;
    gp.dvec = h->batched ? h->bD : h->dD; gp.umin = h->dUmin; gp.umax = h->dUmax; gp.uref = h->dUref; gp.uref_stride = h->uref_stride;
    gp.zs = h->dZs; gp.ys = h->dYs; gp.v0 = h->dV0; gp.status = h->dStatus; gp.piters = h->dPiters;
    gp.max_iter = o.polish_max_iter > 0 ? o.polish_max_iter : 20 * h->R + 50;
    gp.roll_g = s.roll.g; gp.roll_cpl = s.roll.cpl; gp.roll = s.rp;
    HIP_TRY(h, h->dOverflow.once((size_t)h->batch * 33 + 2));   // list, then [batch][32] working sets
    HIP_TRY(h, hipMemsetAsync(h->dOverflow, 0, 2 * sizeof(int32_t), h->stream));
    HIP_TRY(h, h->dOvfSinv.once((size_t)h->batch * (32 * 32 + 32)));
    gp.ovf = h->dOverflow; gp.ovf_ws = h->dOverflow + 2 + h->batch; gp.ovf_sinv = h->dOvfSinv;
    if (s.lazy_redo) { gp.unsolved = h->redo.dUnsolved; gp.redo_gate = h->redo.dGate; gp.step_serial = h->redo.step_serial; }
    if (h->fallback && !h->ltv && h->sd.ready && !h->sd.sqp && !h->sw.no_redo_start) {   // a stage-wise redo may follow: it starts from what this finish gives up with
        HIP_TRY(h, h->sd.start_ws.once((size_t)h->batch * 64));
        gp.redo_ws = h->sd.start_ws; gp.redo_sp = h->sd.NT + h->sd.MC; gp.redo_nt = h->sd.NT;
        h->sd.start_ws_fresh = true;
    }
    if (h->s0_basis_ok && !h->batched && !h->ltv && h->fS_stride == 0) gp.s0_basis = h->dS0Basis;   // (shared model, shared references)
    if (s.mode.rows.mu && sq) { gp.rows = s.mode.rows; gp.rows_map = h->dRowMap; }
    switch (h->np_pairs) {
        case 1: HIP_TRY(h, launch_polish_gen<1>(h, gp)); break;
        case 2: HIP_TRY(h, launch_polish_gen<2>(h, gp)); break;
        case 3: HIP_TRY(h, launch_polish_gen<3>(h, gp)); break;
        default: HIP_TRY(h, launch_polish_gen<4>(h, gp)); break;
    }
    HIP_TRY(h, s.t.mark(2));
    return ALMPC_OK;
}

template <int KS>
hipError_t launch_step_fused(const AdmmParams& ap, const PolishParams& pp, size_t lds, hipStream_t st) {
    const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(k_step_fused<8, KS>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_step_fused<8, KS>), dim3(pp.ntiles), dim3(512), lds, st, ap, pp);
    return hipGetLastError();
}

// Shared model, ONE kernel for the whole step (k_step_fused): the tile is 8 waves and [G | union(ADMM buffers, finish buffers)] fits LDS
int step_fused_shared(Step& s, const PolishLayout& L) {
    almpc_handle* h = s.h;
    const AdmmParams ap = admm_params(h, s.o, s.keep_state);
    PolishParams pp = polish_params(s, L);
    // a step that keeps no warm state hands z, v0 and the signs of y to the finish through LDS (records in the finish's idle wave
    // buffers and second-tier slot) instead of dZs / dV0 / dYflags; ALMPC_OPT_HBM_HANDOFF keeps the global round trip (A/B control)
    pp.handoff = (!s.keep_state && L.sg_shared_off >= 0 && !(s.o.reserved[0] & ALMPC_OPT_HBM_HANDOFF)) ? 1 : 0;
    HIP_TRY(h, s.t.mark(1));   // (no boundary between the phases to time: admm_ms reads 0)
    HIP_TRY(h, h->ks == 30 ? launch_step_fused<30>(ap, pp, L.l_step, h->stream) : launch_step_fused<32>(ap, pp, L.l_step, h->stream));
    HIP_TRY(h, s.t.mark(2));
    return ALMPC_OK;
}

template <int NZC>
hipError_t launch_step_inst_wave_t(const almpc_handle* h, const AdmmInstParams& ip, const PolishParams& pp, size_t lds) {
    const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(k_step_inst_wave<NZC>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_step_inst_wave<NZC>), dim3((unsigned)h->batch), dim3(64), lds, h->stream, ip, pp);
    return hipGetLastError();
}

// ONE wave per instance for the whole step (k_step_inst_wave): the ADMM iterations from registers, then the single-wave finish.  shared:
// every wave reads the shared model's dense operands; else the wave's own per-instance model, with G_i in the wave's LDS
int step_wave(Step& s, const PolishLayout& L, bool shared) {
    almpc_handle* h = s.h;
    if (shared) HIP_TRY(h, s.t.start());
    const AdmmInstParams ip = admm_inst_params(h, s.o, shared);
    PolishParams pp = polish_params(s, L);
    if (shared) { pp.yflags = nullptr; pp.yflag_words = 0; }   // (this ADMM phase hands over y itself)
    const size_t wave = (size_t)L.per_wave + (shared ? 0 : (size_t)h->nz * h->nzs);
    const size_t lds = ((size_t)L.SL.total + wave) * sizeof(double);
    pp.sg_off = -1; pp.g_off = shared ? 0 : L.per_wave;
    pp.lds_per_wave = (int)wave;
    pp.direct = 1;
    HIP_TRY(h, s.t.mark(1));   // (a one-kernel step on per-instance models: no boundary between the phases to time, admm_ms reads 0)
    if (h->nzs <= 16) HIP_TRY(h, launch_step_inst_wave_t<16>(h, ip, pp, lds));
    else if (h->nzs <= 32) HIP_TRY(h, launch_step_inst_wave_t<32>(h, ip, pp, lds));
    else if (h->nzs <= 48) HIP_TRY(h, launch_step_inst_wave_t<48>(h, ip, pp, lds));
    else HIP_TRY(h, launch_step_inst_wave_t<64>(h, ip, pp, lds));
    HIP_TRY(h, s.t.mark(2));
    return ALMPC_OK;
}

template <int START>
hipError_t launch_polish_sgl(const PolishParams& pp, size_t lds, hipStream_t st) {
    const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(k_polish_sgl<START>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_polish_sgl<START>), dim3(pp.ntiles * 16), dim3(64), lds, st, pp);
    return hipGetLastError();
}

// Two launches: the ADMM phase or a guess, then the finish -- k_polish<true> (shared model, G in LDS), k_polish_sgl<0|1> (small batches of
// per-instance models: single-wave workgroups with G_i and the second-tier Sinv in LDS; <1>: from the guess's working set and inverse)
// or k_polish<false> (G through L2); the rollout in the finish's tail where it fits, else behind it
int step_two_launch(Step& s, const PolishLayout& L) {
    almpc_handle* h = s.h;
    hipStream_t st = h->stream;
    if (h->batched && !L.fused) return fail(h, ALMPC_ERR_UNSUPPORTED, "calculate: per-instance models need the fused rollout (n + m <= 8 * lanes-per-row)");
    bool guess_ws = false;
    { const int rc = step_admm_or_guess(s, &guess_ws); if (rc != ALMPC_OK) return rc; }
    PolishParams pp = polish_params(s, L);
    const size_t sgl_wave = (size_t)L.per_wave + POLISH_GLB_PER_INST + (size_t)h->nz * h->nzs;
    const size_t l_sgl = ((size_t)L.SL.total + sgl_wave) * sizeof(double);
    if (L.l_glds <= 160 * 1024 && !h->sw.polish_no_glds && !h->batched) {
        HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_polish<true>), L.l_glds));
        const int wgs = pp.ntiles > h->num_cus ? h->num_cus : pp.ntiles;   // one ADMM tile (16 instances) per workgroup and round
        hipLaunchKernelGGL((k_polish<true>), dim3(wgs), dim3(64 * POLISH_WAVES_GLDS), L.l_glds, st, pp);
    } else if (h->batched && h->batch <= 2 * h->num_cus && l_sgl <= 160 * 1024 && !h->sw.polish_sg_global) {
        pp.sg_off = L.per_wave;
        pp.g_off = L.per_wave + POLISH_GLB_PER_INST;
        pp.lds_per_wave = (int)sgl_wave;
        if (guess_ws) pp.start_rows = h->dStartRows;
        HIP_TRY(h, guess_ws ? launch_polish_sgl<1>(pp, l_sgl, st) : launch_polish_sgl<0>(pp, l_sgl, st));
    } else {
        const size_t l = ((size_t)L.SL.total + (size_t)POLISH_WAVES * L.per_wave) * sizeof(double);
        HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_polish<false>), l));
        hipLaunchKernelGGL((k_polish<false>), dim3((pp.ntiles * 16 + POLISH_WAVES - 1) / POLISH_WAVES), dim3(64 * POLISH_WAVES), l, st, pp);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, s.t.mark(2));
    if (L.fused) return ALMPC_OK;
    s.rp.w = h->dW;
    return step_rollout(s);
}

// No polish: the ADMM phase, then the rollout of its iterate
int step_no_polish(Step& s) {
    { const int rc = step_admm_or_guess(s); if (rc != ALMPC_OK) return rc; }
    HIP_TRY(s.h, s.t.mark(2));
    return step_rollout(s);
}

// Structured handle: the stage-wise active-set solve is the whole step (polish_max_iter caps its working-set changes)
int step_structured(almpc_handle* h, const almpc_opts& o) {
    const double* guess = nullptr;
    if (h->guess_ready) { guess = h->rGuess; h->guess_ready = false; }   // almpc_set_start_from: consumed by this step
    else if (o.warm_start && h->r_has_step) {   // receding horizon: the previous step's inputs shifted by one stage (the last stage repeated)
        HIP_TRY(h, h->rGuess.once((size_t)h->batch * h->nz));
        const long cnt = (long)h->batch * h->nz;
        hipLaunchKernelGGL(k_guess_from_inputs, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, h->batch, h->m, h->N, h->N, 1,
                           (const double*)h->dU, (const double*)h->dUref, h->uref_stride, h->rGuess);
        HIP_TRY(h, hipGetLastError());
        guess = h->rGuess;
    }
    SolveCall solve, net;
    solve.guess = guess; solve.max_iter = o.polish_max_iter;
    net.filter = FILTER_UNSOLVED; net.guess = h->dU;
    if (h->sd.ready) {
        HIP_TRY(h, launch_sdual(h, solve));
        // safety net (input box only, S = 0): what the dual method left without a certificate goes to the primal Riccati active set
        if (!h->sd.has_box && !h->sd.has_eq && !h->sd.useS && h->rKst) HIP_TRY(h, launch_riccati(h, net));
    } else
        HIP_TRY(h, launch_riccati(h, solve));
    h->r_has_step = true;
    return ALMPC_OK;
}

// k_ltv_stage_prepare on the handle's stream: (xb, ub) -> the iterate buffers, ebar, qadd, the terminal-equality target.  Launch only.
hipError_t launch_ltv_stage_prepare(almpc_handle* h, const double* xb, const double* ub) {
    const almpc_handle::Lsw& l = h->lsw;
    LtvStageParams p;
    p.n = h->n; p.m = h->m; p.N = h->N; p.batch = h->batch; p.useR = h->kept.useR; p.useS = h->kept.useS;
    p.xbar = xb; p.ubar = ub; p.xref = h->cert.xref; p.uref = h->cert.uref; p.R = h->wR; p.S = h->wS;
    p.xbar_out = h->dXref; p.ubar_out = h->dUref; p.ebar = l.ebar; p.qadd = l.qadd; p.eqt = l.eqt;
    const int waves = LTV_STAGE_THREADS / 64, wgs = capped_grid(h->batch, waves, 8 * h->num_cus);
    hipLaunchKernelGGL(k_ltv_stage_prepare, dim3((unsigned)wgs), dim3(LTV_STAGE_THREADS), 0, h->stream, p);
    return hipGetLastError();
}

// The step of an almpc_design_ltv_stagewise design, by sqp_qp_stagewise's rule: an input box alone without S goes to the primal Riccati
// active set on the stage models, everything else to k_sgains + k_sdual; start v = 0 (the guess is ubar itself: its inputs on a bound
// seed the working set).  Behind the solve k_ltv_stage_finish: u = ubar + e_u, x = xbar + e_x.  opts.warm_start is ignored.
int step_ltv_stagewise(almpc_handle* h, const almpc_opts& o) {
    SolveCall qp;
    qp.guess = h->dUref; qp.max_iter = o.polish_max_iter;
    if (!h->sd.ready) {
        HIP_TRY(h, launch_riccati(h, qp));
    } else {
        qp.first_tier = h->nz > 48 ? 1 : 0;
        HIP_TRY(h, launch_sgains(h));
        HIP_TRY(h, launch_sdual(h, qp));
    }
    LtvStageFinishParams f;
    f.n = h->n; f.m = h->m; f.N = h->N; f.batch = h->batch;
    f.xbar = h->dXref; f.ubar = h->dUref; f.ex = h->dEx; f.eu = h->dEu; f.x = h->dX; f.u = h->dU;
    const int waves = LTV_STAGE_THREADS / 64, wgs = capped_grid(h->batch, waves, 8 * h->num_cus);
    hipLaunchKernelGGL(k_ltv_stage_finish, dim3((unsigned)wgs), dim3(LTV_STAGE_THREADS), 0, h->stream, f);
    HIP_TRY(h, hipGetLastError());
    h->r_has_step = true;
    return ALMPC_OK;
}

// Structured fallback: instances the condensed path left without a certificate (status != 0: an active-set finish that ran into its cap,
// a non-finite or indefinite condensed problem) are redone in the multiple-shooting form, from the step's own result -- deferred
// (almpc_handle::Redo) or right behind the step
int step_redo(Step& s) {
    almpc_handle* h = s.h;
    if (s.lazy_redo) {
        h->redo.lazy_pending = true;   // (resolve_lazy_redo at the next host sync point)
        return ALMPC_OK;
    }
    if (!h->fallback || h->ltv || h->weighted || !s.o.polish) return ALMPC_OK;
    return launch_redo(h, SolveCall(), !h->sw.dbg_no_sdual_fb, !h->sw.dbg_no_primal_net);   // (right behind the step: its x0 is still the handle's)
}

// The pinned count and the gate word of the redo (almpc_handle::Redo): at the first step that defers its redo
hipError_t ensure_unsolved_word(almpc_handle* h) {
    almpc_handle::Redo& r = h->redo;
    if (r.hUnsolved) return hipSuccess;
    hipError_t e = r.hUnsolved.alloc(1);
    if (e != hipSuccess) return e;
    *r.hUnsolved = 0; r.unsolved_seen = 0;
    if ((e = r.dGate.alloc(1)) != hipSuccess) return e;
    if ((e = hipMemset(r.dGate, 0, sizeof(int))) != hipSuccess) return e;   // (step numbers start at 1)
    return hipHostGetDevicePointer(reinterpret_cast<void**>(&r.dUnsolved), r.hUnsolved, 0);
}

// One step on checked options: the route is picked here, on every call (it depends on almpc_set_step_fusion, the reference strides,
// the options and the handle's switches)
int run_step(almpc_handle* h, const almpc_opts& o, StepMode mode) {
    // ALMPC_OPT_NO_WARM_STATE: shared-model steps with the polish on (the polish needs only the signs of y); ignored elsewhere
    const bool keep_state = !((o.reserved[0] & ALMPC_OPT_NO_WARM_STATE) && !h->batched && o.polish && h->mc == 0);
    if (o.warm_start && !h->state_valid)
        return fail(h, ALMPC_ERR_INVALID, "calculate: warm_start = 1, but the previous step ran with ALMPC_OPT_NO_WARM_STATE (no ADMM state was kept)");
    // default redo of unsolved instances on the shared-model / input-box-only path: lazily, at the next host sync (almpc_handle::Redo)
    // (every condensed path that is not the SQP loop ends in a finish that does the counting -- polish_body for an input box,
    // polish_gen_body with state rows --: shared model, per-instance models, re-linearisation pipeline.  Infeasible instances keep
    // their verdict and are not counted; what is counted is rare -- a handful of edge-of-feasibility instances in 4096 -- and a
    // stage-wise solve of one of them takes about a millisecond, which an eager redo would put behind every step)
    const bool lazy_redo = h->fallback == 2 && !h->structured && !h->ltv && !h->weighted && o.polish != 0 &&
                           (h->sd.ready || (h->mc == 0 && h->rKst)) && !h->sw.eager_redo;
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->io.big_copy_pending) {   // an asynchronous read-back straight from the result buffers: this step overwrites them
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->io.ev_big, 0));
        h->io.big_copy_pending = false;
    }
    h->redo.step_serial += 1;
    h->sd.start_ws_fresh = false;
    int rc = ALMPC_OK;
    if (h->lsw.ready) {
        rc = step_ltv_stagewise(h, o);
    } else if (h->structured) {
        rc = step_structured(h, o);
    } else {
        Step s{h, o, mode, keep_state, lazy_redo, StepTimer(), roll_geom(h), rollout_params(h)};
        HIP_TRY(h, s.t.open(h));
        if (h->batched && mode.guess != Guess::Admm && !o.polish) return fail(h, ALMPC_ERR_INVALID, "calculate: the SQP loop needs opts.polish = 1");
        if (h->mc > 0 && !o.polish)
            return fail(h, ALMPC_ERR_UNSUPPORTED, "calculate: problems with state rows (state box / terminal equality) need opts.polish = 1");
        if (lazy_redo) HIP_TRY(h, ensure_unsolved_word(h));
        const PolishLayout L = polish_layout(h, s.roll);
        switch (pick_route(s, L)) {
            case Route::StateRows: rc = step_state_rows(s); break;
            case Route::FusedShared: rc = step_fused_shared(s, L); break;
            case Route::WaveShared: rc = step_wave(s, L, true); break;
            case Route::WaveInst: rc = step_wave(s, L, false); break;
            case Route::TwoLaunch: rc = step_two_launch(s, L); break;
            case Route::NoPolish: rc = step_no_polish(s); break;
        }
        if (rc == ALMPC_OK) rc = step_redo(s);
        if (rc == ALMPC_OK) HIP_TRY(h, s.t.close(h));
    }
    if (rc != ALMPC_OK) return rc;
    h->state_valid = keep_state;   // (recorded only here: every launch of the step went out)
    h->sens.stepped = true; h->sens.have = 0;
    h->cert.have = 0;
    if (h->io.x0_slot >= 0) {      // the x0 slot of an asynchronous update is free again once this step has finished
        HIP_TRY(h, hipEventRecord(h->io.ev_used[h->io.x0_slot], h->stream));
        h->io.used_pending[h->io.x0_slot] = true;
    }
    return ALMPC_OK;
}

// almpc_calculate_async in the given mode: the options checked against the design, then the step
int calculate_checked(almpc_handle* h, const almpc_opts* user, StepMode mode) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, "calculate before design");
    almpc_opts o;
    almpc_default_opts(&o);
    if (user) o = *user;
    if (o.rho == 0.0) o.rho = h->rho;
    if (o.sigma == 0.0) o.sigma = h->sigma;
    if (o.rho != h->rho || o.sigma != h->sigma)
        return fail(h, ALMPC_ERR_INVALID, "calculate: rho/sigma differ from the design values (the shared KKT inverse is built for them)");
    if (o.max_iter < 1 || o.check_every < 1 || !(o.alpha > 0.0 && o.alpha < 2.0) || !(o.eps_abs >= 0.0) || !(o.eps_rel >= 0.0))
        return fail(h, ALMPC_ERR_INVALID, "calculate: bad options");
    return run_step(h, o, mode);
}
}  // namespace

extern "C" {

int almpc_design_batched(almpc_handle* h, const double* A_batch, const double* B_batch, const double* Q, const double* R,
                         const double* S, const double* P, int P_per_instance, const double* umin, const double* umax,
                         double rho, double sigma) {
    if (!h) return ALMPC_ERR_INVALID;
    drop_lazy_redo(h);
    return h->structured ? design_batched_structured(h, A_batch, B_batch, Q, R, S, P, P_per_instance, umin, umax)
                         : design_batched_condensed(h, A_batch, B_batch, Q, R, S, P, P_per_instance, umin, umax, rho, sigma);
}

// One weight set per instance: see include/almpc.h.  The checks that are this call's own, every set symmetrised, then the condensed
// per-instance design with strides on its weights.
int almpc_design_batched_weighted(almpc_handle* h, const double* A_batch, const double* B_batch, const double* Q_batch, const double* R_batch,
                                  const double* S_batch, const double* P, int P_per_instance, const double* umin, const double* umax,
                                  double rho, double sigma) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!A_batch || !B_batch || !Q_batch || !R_batch || !umin || !umax) return fail(h, ALMPC_ERR_INVALID, "design_batched_weighted: null matrix pointer");
    if (h->structured)
        return fail(h, ALMPC_ERR_UNSUPPORTED, "design_batched_weighted: an ALMPC_FLAG_STRUCTURED handle's solvers (k_sgains, k_riccati, k_sdual) take shared weights");
    if (h->fallback == 1)
        return fail(h, ALMPC_ERR_UNSUPPORTED, "design_batched_weighted: almpc_set_structured_fallback(h, 1) asks for a stage-wise redo, whose solvers take shared weights");
    const int n = h->n, m = h->m;
    const size_t b = (size_t)h->batch, nn = (size_t)n * n, mm = (size_t)m * m;
    // the branch rule (src/sub/design_mpc.jl:423-456) is one choice per launch: every instance has to take instance 0's
    for (size_t i = 1; i < b; ++i) {
        if ((R_batch[i * mm] != 0.0) != (R_batch[0] != 0.0))
            return fail(h, ALMPC_ERR_INVALID, "design_batched_weighted: R[1,1] == 0 for some instances and not for others (the branch is one for the batch): instance " + std::to_string(i));
        if (S_batch && (S_batch[i * mm] != 0.0) != (S_batch[0] != 0.0))
            return fail(h, ALMPC_ERR_INVALID, "design_batched_weighted: S[1,1] == 0 for some instances and not for others (the branch is one for the batch): instance " + std::to_string(i));
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (nothing of an earlier design still reads the staging buffers)
    HIP_TRY(h, h->hQi.grow(b * nn));
    HIP_TRY(h, h->hRi.grow(b * mm));
    if (S_batch) HIP_TRY(h, h->hSi.grow(b * mm));
    const InstanceWeights wi{h->hQi, h->hRi, S_batch ? h->hSi.get() : nullptr};
    // (hm::symmetrised's arithmetic, written into place: no vector per matrix)
    const auto sym_into = [](const double* M, int k, double* o) {
        for (int j = 0; j < k; ++j) {
            o[(size_t)j * k + j] = M[(size_t)j * k + j];
            for (int i = 0; i < j; ++i) o[(size_t)j * k + i] = o[(size_t)i * k + j] = 0.5 * (M[(size_t)j * k + i] + M[(size_t)i * k + j]);
        }
    };
    for (size_t i = 0; i < b; ++i) {
        sym_into(Q_batch + i * nn, n, h->hQi + i * nn);
        sym_into(R_batch + i * mm, m, h->hRi + i * mm);
        if (S_batch) sym_into(S_batch + i * mm, m, h->hSi + i * mm);
    }
    drop_lazy_redo(h);
    return design_batched_condensed(h, A_batch, B_batch, Q_batch, R_batch, S_batch, P, P_per_instance, umin, umax, rho, sigma, &wi);
}

// parity hook: the weights instance i is designed on, as the design kernels read them (symmetrised); the shared set for every i
// unless the design is almpc_design_batched_weighted's
int almpc_get_weights_instance(almpc_handle* h, int instance, double* Q, double* R, double* S) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, "get_weights_instance before design");
    if (instance < 0 || instance >= h->batch) return fail(h, ALMPC_ERR_INVALID, "get_weights_instance: instance out of range");
    const size_t nn = (size_t)h->n * h->n, mm = (size_t)h->m * h->m, i = (size_t)instance;
    if (!h->weighted) {
        const almpc_handle::Kept& k = h->kept;
        if (k.Q.size() != nn || k.R.size() != mm || k.S.size() != mm || h->relin.ready)   // (the pipeline's Q and R are kept for its certificate)
            return fail(h, ALMPC_ERR_UNSUPPORTED, "get_weights_instance: this design keeps no host copy of its weights (condensed almpc_design_shared / _batched do)");
        if (Q) std::copy(k.Q.begin(), k.Q.end(), Q);
        if (R) std::copy(k.R.begin(), k.R.end(), R);
        if (S) std::copy(k.S.begin(), k.S.end(), S);
        return ALMPC_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (Q) HIP_TRY(h, hipMemcpy(Q, h->wiQ + i * nn, nn * sizeof(double), hipMemcpyDeviceToHost));
    if (R) HIP_TRY(h, hipMemcpy(R, h->wiR + i * mm, mm * sizeof(double), hipMemcpyDeviceToHost));
    if (S) {
        if (!h->wiS_given) std::fill(S, S + mm, 0.0);   // (no S_batch: S = 0 everywhere)
        else HIP_TRY(h, hipMemcpy(S, h->wiS + i * mm, mm * sizeof(double), hipMemcpyDeviceToHost));
    }
    return ALMPC_OK;
}

// Time-varying models: see include/almpc.h.  The host prepares ebar = xbar - x_ref (stages 1..N), the input part of the
// gradient 2 Rbar (ubar - u_ref) + 2 D'Sbar D ubar, and hands stage 0's (A, B) to the time-invariant slots (they only feed
// the rollout outputs x / e_x, which are not defined for an LTV design).
int almpc_design_ltv(almpc_handle* h, const double* A_all, const double* B_all, const double* c_all, const double* xbar,
                     const double* ubar, const double* xref, const double* uref, const double* Q, const double* R, const double* S,
                     const double* P, int P_per_instance, const double* umin, const double* umax, double rho, double sigma) {
    if (!h) return ALMPC_ERR_INVALID;
    if (model_continuous(h)) return fail(h, ALMPC_ERR_UNSUPPORTED, "design_ltv: continuous-time models (almpc_set_model_time) are not discretised stage by stage; give discrete stage models");
    drop_lazy_redo(h);
    if (!A_all || !B_all || !xbar || !ubar || !Q || !R || !P || !umin || !umax)
        return fail(h, ALMPC_ERR_INVALID, "design_ltv: null pointer (P must be given: there is no single model to take a DARE of)");
    const int n = h->n, m = h->m, N = h->N, nz = h->nz;
    const size_t b = (size_t)h->batch;
    if (!ltv_supported(h))
        return fail(h, ALMPC_ERR_UNSUPPORTED, "design_ltv: nz <= 128, or nz^2 + 3 n nz doubles must fit the 160 KB of LDS");
    std::vector<double> A0(b * n * n), B0(b * n * m), ebar(b * N * n), qadd(b * nz, 0.0);
    for (size_t i = 0; i < b; ++i) {
        std::copy(A_all + i * N * n * n, A_all + i * N * n * n + (size_t)n * n, A0.begin() + i * n * n);
        std::copy(B_all + i * N * n * m, B_all + i * N * n * m + (size_t)n * m, B0.begin() + i * n * m);
        for (int k = 0; k < N; ++k)
            for (int j = 0; j < n; ++j)
                ebar[(i * N + k) * n + j] = xbar[i * (size_t)(N + 1) * n + (size_t)(k + 1) * n + j] - (xref ? xref[(size_t)(k + 1) * n + j] : 0.0);
    }
    const bool useR = R[0] != 0.0, useS = useR && S && S[0] != 0.0;
    for (size_t i = 0; i < b; ++i) {
        const double* ub = ubar + i * nz;
        double* qa = qadd.data() + i * nz;
        if (useR)
            for (int k = 0; k < N; ++k)
                for (int a = 0; a < m; ++a) {
                    double sr = 0.0;
                    for (int c2 = 0; c2 < m; ++c2) sr += 0.5 * (R[(size_t)c2 * m + a] + R[(size_t)a * m + c2]) * (ub[k * m + c2] - (uref ? uref[k * m + c2] : 0.0));
                    qa[k * m + a] += 2.0 * sr;
                }
        if (useS)  // the input-rate cost is on u itself (src/sub/design_mpc.jl:423-446): 2 D'Sbar D ubar
            for (int k = 0; k + 1 < N; ++k)
                for (int a = 0; a < m; ++a) {
                    double sd = 0.0;
                    for (int c2 = 0; c2 < m; ++c2) sd += 0.5 * (S[(size_t)c2 * m + a] + S[(size_t)a * m + c2]) * (ub[k * m + c2] - ub[(k + 1) * m + c2]);
                    qa[k * m + a] += 2.0 * sd;
                    qa[(k + 1) * m + a] -= 2.0 * sd;
                }
    }
    LtvInputs in{A_all, B_all, c_all, ebar.data(), qadd.data(), ubar, xbar, xref, uref};
    if (h->structured) return fail(h, ALMPC_ERR_UNSUPPORTED, "structured solve: time-varying designs go through almpc_sqp_fnn_* (stage models on the device)");
    return design_ltv_condensed(h, A0.data(), B0.data(), Q, R, S, P, P_per_instance, umin, umax, rho, sigma, in);
}

// ---- time-varying designs on the stage-wise solvers (almpc_design_ltv_stagewise, almpc_ltv_stagewise_update; include/almpc.h) ----

// The one path both forms of both calls take: the five trajectory arrays into the handle's buffers (stage models and defects by copy,
// host to device or device to device; a host trajectory through the staging pair), then k_ltv_stage_prepare.  Enqueues; the host form
// waits for its uploads, the device form for nothing.
static int ltv_stagewise_load(almpc_handle* h, const double* A_all, const double* B_all, const double* c_all, const double* xbar,
                              const double* ubar, int on_device) {
    almpc_handle::Lsw& l = h->lsw;
    const size_t n = (size_t)h->n, m = (size_t)h->m, N = (size_t)h->N, b = (size_t)h->batch;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->lA, A_all, b * N * n * n * sizeof(double), kind, st));
    HIP_TRY(h, hipMemcpyAsync(h->lB, B_all, b * N * n * m * sizeof(double), kind, st));
    if (l.has_c) HIP_TRY(h, hipMemcpyAsync(h->lC, c_all, b * N * n * sizeof(double), kind, st));
    const double *xb = xbar, *ub = ubar;
    if (!on_device) {
        HIP_TRY(h, hipMemcpyAsync(l.xst, xbar, b * (N + 1) * n * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(l.ust, ubar, b * N * m * sizeof(double), hipMemcpyHostToDevice, st));
        xb = l.xst; ub = l.ust;
    }
    HIP_TRY(h, launch_ltv_stage_prepare(h, xb, ub));
    if (!on_device) HIP_TRY(h, hipStreamSynchronize(st));   // (the caller's host arrays are free when the call returns)
    h->sens.stepped = false; h->sens.have = 0; h->cert.have = 0;   // (the last step belongs to the data replaced here)
    h->r_has_step = false;
    return ALMPC_OK;
}

int almpc_design_ltv_stagewise(almpc_handle* h, const double* A_all, const double* B_all, const double* c_all, const double* xbar,
                               const double* ubar, const double* xref, const double* uref, const double* Q, const double* R,
                               const double* S, const double* P, int P_per_instance, const double* umin, const double* umax,
                               int on_device) {
    if (!h) return ALMPC_ERR_INVALID;
    const char* who = "design_ltv_stagewise";
    const std::string w(who);
    if (!h->structured)
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": an ALMPC_FLAG_STRUCTURED handle's call (a condensed handle: almpc_design_ltv)");
    if (model_continuous(h))
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": continuous-time models (almpc_set_model_time) are not discretised stage by stage; give discrete stage models");
    drop_lazy_redo(h);
    if (!A_all || !B_all || !xbar || !ubar || !Q || !R || !P || !umin || !umax)
        return fail(h, ALMPC_ERR_INVALID, w + ": null pointer (P must be given: there is no single model to take a DARE of)");
    const int n = h->n, m = h->m, N = h->N, nz = h->nz;
    const size_t b = (size_t)h->batch;
    ALMPC_TRY(check_input_box(h, umin, umax, who));
    // the route and its shape, before anything is touched: input box alone without S -> k_riccati_t, else k_sgains + k_sdual
    const StateBox box = state_box(h);
    const bool useR = R[0] != 0.0, useS = useR && S && S[0] != 0.0, rows = box.min || h->terminal_eq;
    if (!rows && !useS) {
        if (!riccati_shape_ok(h)) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the shape is outside k_riccati (n <= 32, m <= 16, m N <= 1024, its stage buffers in LDS)");
    } else {
        int NT = 0, MC = 0;
        const int nt = useS ? n + m : n;
        if (!sdual_shape_ok(n, m, N, useS) || !sdual_pick_shape(nt, m, &NT, &MC))
            return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": state rows / input-rate weight need the stage-wise dual solve (n + m <= 48, (N + 1)(n + m) <= 4096)");
        if (NT > 16)
            return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": state rows / input-rate weight need n (+ m with S) <= 16 and m <= 8 here: the table-less G = 1 builds of "
                                                      "k_sdual ((32, 16), (48, 16): a per-instance design has no cached responses) are not launched");
        if ((size_t)sgains_lds_doubles(nt, m) * sizeof(double) > LDS_BUDGET) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the gain recursion does not fit LDS");
    }
    ALMPC_TRY(begin_redesign(h, DROP_SQP | DROP_RELIN | WAIT_STREAM));
    const hm::mat Qm = hm::symmetrised(Q, n), Rm = hm::symmetrised(R, m), Sm = hm::symmetrised(S, m);
    const bool p_inst = P_per_instance != 0;
    hm::mat Pall((p_inst ? b : 1) * (size_t)n * n);
    for (size_t i = 0; i < (p_inst ? b : 1); ++i) {
        const hm::mat Pm = hm::symmetrised(P + i * n * n, n);
        std::copy(Pm.begin(), Pm.end(), Pall.begin() + i * n * n);
    }
    almpc_handle::Lsw& l = h->lsw;
    l.has_c = c_all != nullptr; l.sP = p_inst ? (long)n * n : 0;
    // buffers: stage models and defects, the iterate, the prepared vectors, the host form's staging pair
    const size_t xs = (size_t)n * (N + 1);
    HIP_TRY(h, h->lA.grow(b * N * n * n)); HIP_TRY(h, h->lB.grow(b * N * n * m));
    if (l.has_c) HIP_TRY(h, h->lC.grow(b * N * n)); else h->lC.reset();
    h->lE.reset();
    HIP_TRY(h, h->dXref.alloc(b * xs)); HIP_TRY(h, h->dUref.alloc(b * nz));
    h->dFS.reset(); h->dV0S.reset(); h->ref_keep = false;
    HIP_TRY(h, l.ebar.grow(b * N * n)); HIP_TRY(h, l.qadd.grow(b * nz));
    HIP_TRY(h, l.xst.grow(b * xs)); HIP_TRY(h, l.ust.grow(b * nz));
    if (h->terminal_eq) HIP_TRY(h, l.eqt.grow((size_t)n)); else l.eqt.reset();
    // weights, terminal weights and the shared references on the device
    HIP_TRY(h, h->wQ.once((size_t)n * n)); HIP_TRY(h, h->wR.once((size_t)m * m)); HIP_TRY(h, h->wS.once((size_t)m * m));
    HIP_TRY(h, hipMemcpy(h->wQ, Qm.data(), Qm.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->wR, Rm.data(), Rm.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->wS, Sm.data(), Sm.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, h->bP.grow(b * n * n));
    HIP_TRY(h, hipMemcpy(h->bP, Pall.data(), Pall.size() * sizeof(double), hipMemcpyHostToDevice));
    std::vector<double> xr(xs, 0.0), ur((size_t)nz, 0.0);
    if (xref) xr.assign(xref, xref + xr.size());
    if (uref) ur.assign(uref, uref + ur.size());
    HIP_TRY(h, h->cert.xref.upload(xr.data(), xr.size()));
    HIP_TRY(h, h->cert.uref.upload(ur.data(), ur.size()));
    ALMPC_TRY(upload_input_box(h, umin, umax));
    h->P.assign(Pall.begin(), Pall.begin() + (size_t)n * n); h->H.clear(); h->F.clear(); h->d.clear();
    keep_weights(h, &Qm, &Rm, Sm, useR, useS);
    h->t_step = false; h->c_step = false; h->weighted = false;
    // state rows as the SQP loop's stage-wise route has them: coordinates of the stage-wise trajectory, no constraint-space matrix
    ALMPC_TRY(setup_state_rows(h, nullptr, nullptr, true));
    h->has_box = box.min ? 1 : 0;
    h->mc = box.min ? N * n : (h->terminal_eq ? n : 0);
    h->xref_stride = (long)xs; h->uref_stride = nz; h->fS_stride = nz;
    h->batched = true; h->r_batched_P = true; h->rP_stride = l.sP; h->bP_stride = l.sP;
    h->sd.ready = false;
    if (!rows && !useS)
        ALMPC_TRY(riccati_weights(h, Qm, Rm, nullptr));
    else {   // per-instance records (k_sgains, every stage), cost terms and defects' value-function terms per instance, no cached responses
        ALMPC_TRY(sdual_setup_batched(h, Qm, Rm, useS ? &Sm : nullptr, false, box.min, box.max, h->terminal_eq != 0));
        almpc_handle::Sd& sd = h->sd;
        const size_t TP = (size_t)sdual_tp(sd.NT, sd.MC, N);
        HIP_TRY(h, sd.base.grow(b * TP));
        sd.has_base = true; sd.base_stride = (long)TP;
        HIP_TRY(h, sd.pc.grow(b * N * sd.NT)); HIP_TRY(h, sd.ct.grow(b * N * sd.NT));
    }
    l.ready = true;
    const int rc = ltv_stagewise_load(h, A_all, B_all, c_all, xbar, ubar, on_device);
    if (rc != ALMPC_OK) { l.ready = false; return rc; }
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (a design call returns with its work done; the update call is the one that does not wait)
    h->cert.kept = true; h->cert.kept_c = l.has_c;
    h->ltv = true;
    h->designed = true;
    return ALMPC_OK;
}

int almpc_ltv_stagewise_update(almpc_handle* h, const double* A_all, const double* B_all, const double* c_all, const double* xbar,
                               const double* ubar, int on_device) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->designed || !h->lsw.ready) return fail(h, ALMPC_ERR_NOT_DESIGNED, "ltv_stagewise_update before almpc_design_ltv_stagewise");
    if (!A_all || !B_all || !xbar || !ubar) return fail(h, ALMPC_ERR_INVALID, "ltv_stagewise_update: null pointer");
    if ((c_all != nullptr) != h->lsw.has_c)
        return fail(h, ALMPC_ERR_INVALID, h->lsw.has_c ? "ltv_stagewise_update: c_all is NULL, but the design was given defects"
                                                       : "ltv_stagewise_update: c_all is given, but the design had none (NULL)");
    HIP_TRY(h, hipSetDevice(h->device));
    return ltv_stagewise_load(h, A_all, B_all, c_all, xbar, ubar, on_device);
}

// The vectors k_ltv_stage_prepare left for the current data, read back (any pointer may be null): ebar [batch][N][n], qadd [batch][N][m],
// the terminal-equality target [n]
int almpc_get_ltv_stagewise_prepared(almpc_handle* h, double* ebar, double* qadd, double* eq_target) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->designed || !h->lsw.ready) return fail(h, ALMPC_ERR_NOT_DESIGNED, "get_ltv_stagewise_prepared before almpc_design_ltv_stagewise");
    if (eq_target && !h->lsw.eqt) return fail(h, ALMPC_ERR_INVALID, "get_ltv_stagewise_prepared: the design has no terminal equality");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t b = (size_t)h->batch, N = (size_t)h->N;
    if (ebar) HIP_TRY(h, hipMemcpy(ebar, h->lsw.ebar, b * N * h->n * sizeof(double), hipMemcpyDeviceToHost));
    if (qadd) HIP_TRY(h, hipMemcpy(qadd, h->lsw.qadd, b * N * h->m * sizeof(double), hipMemcpyDeviceToHost));
    if (eq_target) HIP_TRY(h, hipMemcpy(eq_target, h->lsw.eqt, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

int almpc_get_gradient_instance(almpc_handle* h, int instance, double* q) {
    if (!h || !q) return ALMPC_ERR_INVALID;
    if (!h->designed || !h->ltv) return fail(h, ALMPC_ERR_NOT_DESIGNED, "get_gradient_instance needs almpc_design_ltv");
    if (instance < 0 || instance >= h->batch) return fail(h, ALMPC_ERR_INVALID, "get_gradient_instance: instance out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpy(q, h->bQ + (size_t)instance * h->nz, (size_t)h->nz * sizeof(double), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

// The network arguments of a setup call that are there and have a shape
static bool net_args_ok(int H, int L, const double* W_in, const double* W_h, const double* b_h, const double* W_out) {
    return H >= 1 && L >= 0 && W_in && W_out && (L == 0 || (W_h && b_h));
}
// ... and its kind and activation (setup_net); who: "relin" or "sqp", the call's name in the message
static int decode_setup_net(almpc_handle* h, bool dense, const char* who, int* activation, int* net) {
    if (setup_net(dense, *activation, net, activation)) return ALMPC_OK;
    return fail(h, ALMPC_ERR_UNSUPPORTED, std::string(who) + (dense ? "_densenet_setup: activation must be 0..4"
                                                                    : "_fnn_setup: activation must be ALMPC_NET_CODE(kind 0..2, activation 0..4)"));
}
// The network of a pipeline or loop as the kernels take it: shape, weights and the batch; points and outputs are the caller's
static FnnParams fnn_params(const almpc_handle* h, const almpc_handle::Net& q) {
    FnnParams fp;
    fp.n = h->n; fp.m = h->m; fp.H = q.H; fp.L = q.L; fp.act = q.act; fp.batch = h->batch;
    fp.W_in = q.W_in; fp.W_h = q.W_h; fp.b_h = q.b_h; fp.W_out = q.W_out;
    return fp;
}
// ... at its points (ppi per group, the strides between groups), with where the Jacobians and the outputs (null: none) go
static FnnParams fnn_points(FnnParams fp, const double* x, const double* u, int ppi, long xs_group, long us_group, double* A, double* B, double* f) {
    fp.x = x; fp.u = u; fp.ppi = ppi; fp.xs_group = xs_group; fp.us_group = us_group; fp.A = A; fp.B = B; fp.f = f;
    return fp;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Per-step re-linearisation of a black-box Fnn model, resident on the device (BASELINE configs[3]; include/almpc.h).

// Host side of a setup: the weights, symmetrised, and the references
struct RelinSetup { hm::mat Qm, Rm, Sm, Pm; std::vector<double> xr, ur; };

// The front of almpc_relin_*_setup on either kind of handle: the checks that are left, the previous design gone, then the network and
// every instance's linearisation input on the device, the timing events, the buffers of almpc_relin_fnn_advance
static int relin_setup_common(almpc_handle* h, int H, int L, int net, int activation, const double* W_in, const double* W_h, const double* b_h,
                              const double* W_out, const double* xref, const double* uref, const double* Q, const double* R, const double* S,
                              const double* P, const double* umin, const double* umax, RelinSetup& s) {
    const int n = h->n, m = h->m, N = h->N;
    const size_t b = (size_t)h->batch;
    if (fnn_wave_scratch_doubles(n, m, H, L, net) * sizeof(double) > 160 * 1024)
        return fail(h, ALMPC_ERR_UNSUPPORTED, "relin_fnn_setup: the network's forward-mode Jacobian must fit the 160 KB of LDS");
    ALMPC_TRY(check_input_box(h, umin, umax, "relin_fnn_setup"));
    ALMPC_TRY(begin_redesign(h, DROP_SQP | DROP_RELIN | WAIT_STREAM));
    s.Qm = hm::symmetrised(Q, n); s.Rm = hm::symmetrised(R, m); s.Sm = hm::symmetrised(S, m); s.Pm = hm::symmetrised(P, n);
    almpc_handle::Relin& q = h->relin;
    q.useR = s.Rm[0] != 0.0; q.useS = q.useR && s.Sm[0] != 0.0;
    keep_weights(h, &s.Qm, &s.Rm, s.Sm, q.useR != 0, q.useS != 0);
    if (h->structured && !sdual_shape_ok(n, m, N, q.useS != 0))
        return fail(h, ALMPC_ERR_UNSUPPORTED, "relin_fnn_setup (structured): n (+ m with an input-rate weight) <= 48, m <= 16 and (N + 1)(n + m) <= 4096");
    q.Q.reset(); q.R.reset(); q.S.reset(); q.gS.reset();   // (the network and ulin are replaced by their uploads below)
    s.xr.assign((size_t)n * (N + 1), 0.0); s.ur.assign((size_t)h->nz, 0.0);
    if (xref) s.xr.assign(xref, xref + s.xr.size());
    if (uref) s.ur.assign(uref, uref + s.ur.size());
    std::vector<double> ul(b * m);
    for (size_t i = 0; i < b; ++i)
        for (int a = 0; a < m; ++a) ul[i * m + a] = s.ur[a];  // every instance linearises at the first input reference
    HIP_TRY(h, upload_net(q, n, m, H, L, activation, net, W_in, W_h, b_h, W_out)); HIP_TRY(h, q.ulin.upload(ul.data(), ul.size()));
    for (auto& e : q.ev)
        if (!e) HIP_TRY(h, hipEventCreate(&e));
    q.have_prev = false;
    HIP_TRY(h, q.u0.once(b * m));
    HIP_TRY(h, q.xnext.once(b * n));
    return ALMPC_OK;
}

// ... on an ALMPC_FLAG_STRUCTURED handle: the per-instance model and terminal-weight slots, and the stage-wise solver's per-instance
// set-up (records per stage: the terminal weight is the caller's P)
static int relin_setup_structured(almpc_handle* h, const RelinSetup& s, const double* umin, const double* umax) {
    const int n = h->n, m = h->m;
    const size_t b = (size_t)h->batch;
    const hm::mat &Qm = s.Qm, &Rm = s.Rm, &Sm = s.Sm, &Pm = s.Pm;
    almpc_handle::Relin& q = h->relin;
    HIP_TRY(h, h->bA.once(b * n * n));
    HIP_TRY(h, h->bB.once(b * n * m));
    HIP_TRY(h, h->bP.once(b * n * n));
    HIP_TRY(h, hipMemset(h->bA, 0, b * n * n * sizeof(double)));
    HIP_TRY(h, hipMemset(h->bB, 0, b * n * m * sizeof(double)));
    HIP_TRY(h, hipMemcpy(h->bP, Pm.data(), Pm.size() * sizeof(double), hipMemcpyHostToDevice));
    ALMPC_TRY(relin_terminal_setup(h, Rm, Pm));
    ALMPC_TRY(relin_c2d_setup(h));
    h->batched = true; h->ltv = false; h->r_batched_P = true; h->rP_stride = h->t_step ? (long)n * n : 0;   // (t_step: one P_i per step, k_dare)
    h->bP_stride = h->rP_stride;
    const StateBox box = state_box(h);
    h->sd.ready = false;   // (k_sdual whatever ALMPC_STRUCTURED_PRIMAL says: the step's k_sgains has no other reader)
    ALMPC_TRY(sdual_setup_batched(h, Qm, Rm, q.useS ? &Sm : nullptr, false, box.min, box.max, h->terminal_eq != 0));
    if (riccati_shape_ok(h)) ALMPC_TRY(riccati_weights(h, Qm, Rm, nullptr));
    ALMPC_TRY(upload_input_box(h, umin, umax));
    h->P = Pm; h->H.clear(); h->F.clear(); h->d.clear();
    h->has_box = box.min ? 1 : 0;
    h->r_has_step = false;
    h->designed = true;
    const int rc_ref = almpc_set_reference(h, s.xr.data(), s.ur.data(), 0);   // (also the input-rate terms of a horizon-varying u_ref: sdual_update_base)
    if (rc_ref != ALMPC_OK) { h->designed = false; return rc_ref; }
    q.ready = true;
    return ALMPC_OK;
}

// ... on a condensed handle: weights and references on the device (shared; the scaled input-rate gradient fS_i = d_i .* gS and
// v0S_i = -G_i fS_i are per instance, re-made every step), the per-instance operands and state rows, the redo's solvers
static int relin_setup_condensed(almpc_handle* h, const RelinSetup& s, const double* umin, const double* umax, double rho, double sigma) {
    const int n = h->n, m = h->m, N = h->N, nz = h->nz;
    const size_t b = (size_t)h->batch;
    const hm::mat &Qm = s.Qm, &Rm = s.Rm, &Sm = s.Sm, &Pm = s.Pm;
    const std::vector<double>&xr = s.xr, &ur = s.ur;
    almpc_handle::Relin& q = h->relin;
    ALMPC_TRY(ensure_batched_alloc(h));
    // unscaled input-rate gradient of the shared reference: 2 D'Sbar D u_ref (the rate cost is on u itself, src/sub/design_mpc.jl:423-446)
    std::vector<double> gS((size_t)nz, 0.0);
    if (q.useS)
        for (int i = 0; i + 1 < N; ++i)
            for (int a = 0; a < m; ++a) {
                double sd = 0.0;
                for (int c2 = 0; c2 < m; ++c2) sd += Sm[(size_t)c2 * m + a] * (ur[i * m + c2] - ur[(i + 1) * m + c2]);
                gS[i * m + a] += 2.0 * sd;
                gS[(i + 1) * m + a] -= 2.0 * sd;
            }
    HIP_TRY(h, q.Q.upload(Qm.data(), Qm.size())); HIP_TRY(h, q.R.upload(Rm.data(), Rm.size())); HIP_TRY(h, q.S.upload(Sm.data(), Sm.size()));
    HIP_TRY(h, q.gS.upload(gS.data(), gS.size()));
    HIP_TRY(h, hipMemcpy(h->bP, Pm.data(), Pm.size() * sizeof(double), hipMemcpyHostToDevice));
    ALMPC_TRY(relin_terminal_setup(h, Rm, Pm));
    ALMPC_TRY(relin_c2d_setup(h));
    h->bP_stride = h->t_step ? (long)n * n : 0;   // (t_step: one P_i per step, k_dare)
    ALMPC_TRY(upload_input_box(h, umin, umax));
    h->ref_keep = false;
    HIP_TRY(h, h->dXref.upload(xr.data(), xr.size())); HIP_TRY(h, h->dUref.upload(ur.data(), ur.size()));
    HIP_TRY(h, h->dFS.alloc(b * nz)); HIP_TRY(h, h->dV0S.alloc(b * nz)); h->dCold.reset(); h->cold_ref = false;
    HIP_TRY(h, hipMemset(h->dFS, 0, b * nz * sizeof(double))); HIP_TRY(h, hipMemset(h->dV0S, 0, b * nz * sizeof(double)));
    h->xref_stride = 0; h->uref_stride = 0; h->fS_stride = nz;
    h->P = Pm;
    h->rho = rho; h->sigma = sigma;
    const StateBox box = state_box(h);
    ALMPC_TRY(setup_state_rows(h, box.min, box.max, true));
    h->batched = true; h->ltv = false;
    h->state_valid = true;
    h->sd.ready = false;
    if (h->fallback) {
        h->r_batched_P = true; h->rP_stride = h->bP_stride;
        // (the models change with every step: the records of the instances a step leaves unsolved are computed in that step)
        ALMPC_TRY(setup_redo_solvers(h, nullptr, false, Qm, Rm, q.useS ? &Sm : nullptr, box, h->fallback == 1,
                                     "structured fallback: state rows / input-rate weight need n + m <= 48 and (N + 1)(n + m) <= 4096"));
        // the references were uploaded above, not through almpc_set_reference (which this pipeline refuses): the input-rate terms
        // of a horizon-varying u_ref (+-S (u_ref[k-1] - u_ref[k])) have to reach the stage-wise redo from here
        if (h->sd.ready) ALMPC_TRY(sdual_update_base(h, ur.data(), 1));
    }
    q.ready = true;
    return ALMPC_OK;
}

// (dense: almpc_relin_densenet_setup, activation a bare code; else almpc_relin_fnn_setup, activation an ALMPC_NET_CODE)
static int relin_net_setup(almpc_handle* h, bool dense, int H, int L, int activation, const double* W_in, const double* W_h,
                           const double* b_h, const double* W_out, const double* xref, const double* uref, const double* Q,
                           const double* R, const double* S, const double* P, const double* umin, const double* umax, double rho,
                           double sigma) {
    if (!h) return ALMPC_ERR_INVALID;
    drop_lazy_redo(h);
    if (!net_args_ok(H, L, W_in, W_h, b_h, W_out) || !Q || !R || !P || !umin || !umax)
        return fail(h, ALMPC_ERR_INVALID, "relin_fnn_setup: null pointer or bad network shape (P must be given: the terminal weight "
                                          "comes from the linearisation at the last reference, src/sub/design_mpc.jl:312-327)");
    int net = NET_FNN;
    ALMPC_TRY(decode_setup_net(h, dense, "relin", &activation, &net));
    if (!h->structured && (!(rho > 0.0) || !(sigma >= 0.0))) return fail(h, ALMPC_ERR_INVALID, "relin_fnn_setup: rho must be > 0 and sigma >= 0");
    RelinSetup s;
    ALMPC_TRY(relin_setup_common(h, H, L, net, activation, W_in, W_h, b_h, W_out, xref, uref, Q, R, S, P, umin, umax, s));
    return h->structured ? relin_setup_structured(h, s, umin, umax) : relin_setup_condensed(h, s, umin, umax, rho, sigma);
}
int almpc_relin_fnn_setup(almpc_handle* h, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                          const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                          const double* S, const double* P, const double* umin, const double* umax, double rho, double sigma) {
    return relin_net_setup(h, false, H, L, activation, W_in, W_h, b_h, W_out, xref, uref, Q, R, S, P, umin, umax, rho, sigma);
}
int almpc_relin_densenet_setup(almpc_handle* h, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                               const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                               const double* S, const double* P, const double* umin, const double* umax, double rho, double sigma) {
    return relin_net_setup(h, true, H, L, activation, W_in, W_h, b_h, W_out, xref, uref, Q, R, S, P, umin, umax, rho, sigma);
}

// Structured handle (m N beyond the condensed limit, round 5): Jacobians -> the stage records of every instance's own
// unconstrained problem (k_sgains) -> the stage-wise dual active set (k_sdual), warm-started from the previous step's inputs
// shifted by one stage when opts->warm_start is set.  No Hessian is formed: the reference's Fnn-LP delegation has no horizon
// limit (.../fnn/mpc_modeler_implementation_fnn.jl:23-58) and neither has this route.
static int relin_step_structured(almpc_handle* h, almpc_opts o2) {
    almpc_handle::Relin& q = h->relin;
    HIP_TRY(h, launch_sgains(h));   // (every instance)
    if (h->flags & ALMPC_FLAG_TIMING) HIP_TRY(h, hipEventRecord(q.ev[2], h->stream));
    h->designed = true;
    if (!q.have_prev) o2.warm_start = 0;   // (a warm start needs a solved step behind it)
    const int rc = almpc_calculate_async(h, &o2);
    if (rc != ALMPC_OK) h->designed = false;
    return rc;
}

// Condensed handle (fused: the network's points when the design kernel linearises; design_flags: the flag words the finish left to the caller)
static int relin_step_condensed(almpc_handle* h, almpc_opts o2, const FnnParams* fused, const int** design_flags) {
    almpc_handle::Relin& q = h->relin;
    const int nz = h->nz, nzs = h->nzs;
    hipStream_t st = h->stream;
    // 2. the reference's QP for every (A_i, B_i): H_i, F_i, scaling, inverses, V_i; reference-dependent vectors.  A warm step
    // (opts.warm_start = 1 after a solved step) takes its working-set guess from the previous step's inputs shifted by one stage
    // instead of an ADMM phase, and the design then needs one inverse (G_i) instead of two
    const bool warm = o2.warm_start && q.have_prev && o2.polish;
    const DesignStrides ds = batched_strides(h, h->t_step);
    const hipError_t e_ = launch_batched_design(h, ds, q.useR, q.useS, q.Q, q.R, q.S, h->rho, h->sigma, warm, fused);
    if (e_ != hipSuccess) return fail(h, ALMPC_ERR_HIP, std::string("relin design: ") + hipGetErrorString(e_));
    if (h->mc > 0) HIP_TRY(h, launch_ghat_inst(h, nullptr, nullptr));
    if (q.useS) {
        hipLaunchKernelGGL(k_fs_scale, dim3(256), dim3(256), 0, st, h->batch, nz, nzs, q.gS, 0L, h->bD, h->dFS);
        hipLaunchKernelGGL(k_neg_gm, dim3(1, (unsigned)h->batch), dim3(256), 0, st, nz, nzs, 1, nz, h->bG, h->dFS, h->dV0S, (long)nz * nzs, (long)nz);
        HIP_TRY(h, hipGetLastError());
    }
    if (h->flags & ALMPC_FLAG_TIMING) HIP_TRY(h, hipEventRecord(q.ev[2], st));
    // 3. the step itself
    h->designed = true;
    o2.warm_start = 0;   // (the per-instance ADMM's own warm start is not what a warm step of this pipeline means)
    // an instance whose design was flagged gets ALMPC_NON_FINITE: by the finish itself when it is polish_body (input box only), else by
    // a launch of its own behind the step
    StepMode mode;
    mode.guess = warm ? Guess::ShiftInputs : Guess::Admm; mode.fold_flag = h->mc == 0 && o2.polish != 0;
    const int rc = calculate_checked(h, &o2, mode);
    if (rc != ALMPC_OK) h->designed = false;   // (no step ran on this step's designs: the handle is not left "designed")
    if (!mode.fold_flag) *design_flags = h->bFlag;
    return rc;
}

int almpc_relin_fnn_step_async(almpc_handle* h, const almpc_opts* opts) {
    if (!h) return ALMPC_ERR_INVALID;
    almpc_handle::Relin& q = h->relin;
    if (!q.ready) return fail(h, ALMPC_ERR_NOT_DESIGNED, "relin_fnn_step before relin_fnn_setup");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const bool timing = (h->flags & ALMPC_FLAG_TIMING) != 0;
    if (timing) HIP_TRY(h, hipEventRecord(q.ev[0], st));
    // 1. Jacobians at (x0_i, u_ref[:,1]) straight into the handle's per-instance model slots
    const FnnParams fp = fnn_points(fnn_params(h, q), h->dX0, q.ulin, 1, h->n, h->m, h->bA, h->bB, nullptr);
    // (the condensed design kernel's workgroups linearise their own instance -- unless every instance's terminal weight is the DARE solution
    // of its Jacobians, almpc_set_terminal_weight: P_i has to be there before the design, so the Jacobians get their own launch in front;
    // the same when the Jacobians are continuous-time and k_c2d stands between them and the design, almpc_set_model_time)
    const bool fuse_jac = !h->structured && design_fuses_fnn(h, q.H, q.L, q.net) && !h->t_step && !h->c_step;
    if (!fuse_jac) HIP_TRY(h, launch_fnn_jacobian(h->sw, fp, q.net, h->num_cus, st));
    if (timing) HIP_TRY(h, hipEventRecord(q.ev[1], st));
    if (h->c_step) HIP_TRY(h, launch_model_c2d(h, true));   // the network is x' = net(x, u): its Jacobians are continuous-time
    if (h->t_step) HIP_TRY(h, launch_relin_dare(h, h->structured ? h->sd.dQ : q.Q, h->structured ? h->sd.dR : q.R));   // every instance's own P_i, from the route's Q and R
    almpc_opts o2; almpc_default_opts(&o2);   // the options of the step inside: the caller's; each route sets the solver's own warm start by its rule
    if (opts) o2 = *opts;
    const int* design_flags = nullptr;
    ALMPC_TRY(h->structured ? relin_step_structured(h, o2) : relin_step_condensed(h, o2, fuse_jac ? &fp : nullptr, &design_flags));
    // solved; the instances of design_flags and those whose discretisation failed (their model slots hold NaN) leave with ALMPC_NON_FINITE
    q.have_prev = true;
    for (const int* flags : {design_flags, h->c_step ? (const int*)h->cStat.get() : nullptr}) {
        if (!flags) continue;
        hipLaunchKernelGGL(k_flag_to_status, dim3((h->batch + 255) / 256), dim3(256), 0, st, h->batch, flags, h->dStatus);
        HIP_TRY(h, hipGetLastError());
    }
    if (timing) HIP_TRY(h, hipEventRecord(q.ev[3], st));
    return ALMPC_OK;
}

int almpc_relin_fnn_step(almpc_handle* h, const almpc_opts* opts) {
    ALMPC_TRY(almpc_relin_fnn_step_async(h, opts));
    return almpc_synchronize(h);
}

// x0 <- fnn(x0, u[:,1]) on the device: the closed loop of the black-box model itself (the plant a simulation study drives), no host
// round trip.  Follow with almpc_relin_fnn_step(_async) -- typically with opts.warm_start = 1.
int almpc_relin_fnn_advance(almpc_handle* h) {
    if (!h) return ALMPC_ERR_INVALID;
    almpc_handle::Relin& q = h->relin;
    if (!q.ready || !q.have_prev) return fail(h, ALMPC_ERR_NOT_DESIGNED, "relin_fnn_advance needs a solved almpc_relin_fnn_step");
    if (h->c_step)
        return fail(h, ALMPC_ERR_UNSUPPORTED, "relin_fnn_advance: the network is continuous-time (almpc_set_model_time); its plant is an integrator, which is the caller's");
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(enqueue_gated_redo(h));   // (the network is driven by decided instances' inputs only)
    const int n = h->n, m = h->m;
    hipStream_t st = h->stream;
    const size_t cnt = (size_t)h->batch * m;
    hipLaunchKernelGGL(k_pack_first_input, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, h->batch, m, h->N, h->dU, q.u0);
    // (the Jacobians of the forward pass go to a scratch of their own: the model slots keep the last step's linearisations, which a
    // lazily deferred redo of that step still needs)
    HIP_TRY(h, q.Ascr.once((size_t)h->batch * n * n)); HIP_TRY(h, q.Bscr.once((size_t)h->batch * n * m));
    const FnnParams fp = fnn_points(fnn_params(h, q), h->dX0, q.u0, 1, n, m, q.Ascr, q.Bscr, q.xnext);
    HIP_TRY(h, launch_fnn_jacobian(h->sw, fp, q.net, h->num_cus, st));
    if (h->io.x0_slot >= 0) {   // a pinned x0 slot was read once more by the forward pass: free for the host only after it
        HIP_TRY(h, hipEventRecord(h->io.ev_used[h->io.x0_slot], st));
        h->io.used_pending[h->io.x0_slot] = true;
    }
    io_release_x0(h);
    HIP_TRY(h, hipMemcpyAsync(h->dX0, q.xnext, (size_t)h->batch * n * sizeof(double), hipMemcpyDeviceToDevice, st));
    return ALMPC_OK;
}

int almpc_relin_fnn_timing(almpc_handle* h, float* ms_jacobian, float* ms_design, float* ms_step) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!(h->flags & ALMPC_FLAG_TIMING) || !h->relin.ready) return fail(h, ALMPC_ERR_INVALID, "relin_fnn_timing: needs ALMPC_FLAG_TIMING and a step");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipEventSynchronize(h->relin.ev[3]));
    float a = 0, d = 0, s2 = 0;
    HIP_TRY(h, hipEventElapsedTime(&a, h->relin.ev[0], h->relin.ev[1]));
    HIP_TRY(h, hipEventElapsedTime(&d, h->relin.ev[1], h->relin.ev[2]));
    HIP_TRY(h, hipEventElapsedTime(&s2, h->relin.ev[2], h->relin.ev[3]));
    if (ms_jacobian) *ms_jacobian = a;
    if (ms_design) *ms_design = d;
    if (ms_step) *ms_step = s2;
    return ALMPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// SQP outer loop for a black-box Fnn model, resident on the device (see almpc_sqp.hip.h and include/almpc.h).
// (dense: almpc_sqp_densenet_setup, activation a bare code; else almpc_sqp_fnn_setup, activation an ALMPC_NET_CODE)
static int sqp_net_setup(almpc_handle* h, bool dense, int H, int L, int activation, const double* W_in, const double* W_h,
                         const double* b_h, const double* W_out, const double* xref, const double* uref, const double* Q,
                         const double* R, const double* S, const double* P, int P_per_instance, const double* umin, const double* umax,
                         double rho, double sigma) {
    if (!h) return ALMPC_ERR_INVALID;
    if (model_continuous(h))
        return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp_fnn_setup: continuous-time models (almpc_set_model_time) are outside the SQP loop");
    drop_lazy_redo(h);
    if (!net_args_ok(H, L, W_in, W_h, b_h, W_out) || !Q || !R || !P || !umin || !umax)
        return fail(h, ALMPC_ERR_INVALID, "sqp_fnn_setup: null pointer or bad network shape (P must be given)");
    int net = NET_FNN;
    ALMPC_TRY(decode_setup_net(h, dense, "sqp", &activation, &net));
    if (!(rho > 0.0) || !(sigma >= 0.0)) return fail(h, ALMPC_ERR_INVALID, "sqp_fnn_setup: rho must be > 0 and sigma >= 0");
    const int n = h->n, m = h->m, N = h->N, nz = h->nz, nzs = h->nzs;
    const size_t b = (size_t)h->batch, nin = (size_t)n + m;
    if (n > 64 || sqp_step_lds_doubles(n, m, N) * sizeof(double) > 160 * 1024)
        return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp_fnn_setup: n <= 64 (one lane per state in the update kernel) and its stage buffers must fit LDS");
    if (h->structured) {   // a structured handle has no condensed path: every QP of the loop goes to k_riccati (any m N <= 1024)
        if (!riccati_shape_ok(h) && !sdual_shape_ok(h->n, h->m, h->N, false))
            return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp_fnn_setup: the shape is outside both stage-wise QP solvers");
        h->sqp.structured_qp = 1;
    }
    const bool sq_struct = h->sqp.structured_qp != 0;
    if (!sq_struct && !ltv_supported(h))
        return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp_fnn_setup: nz <= 128, or nz^2 + 3 n nz doubles must fit the 160 KB of LDS");
    if ((net == NET_DENSENET ? fnn_wave_scratch_doubles(n, m, H, L, net) : 2 * (size_t)H + 2 * (size_t)H * nin + nin) * sizeof(double) > 160 * 1024)
        return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp_fnn_setup: the network's forward-mode Jacobian must fit the 160 KB of LDS");
    ALMPC_TRY(check_input_box(h, umin, umax, "sqp_fnn_setup"));
    // (any earlier design of the handle is replaced: its reference buffers are released below)
    ALMPC_TRY(begin_redesign(h, DROP_SQP | DROP_RELIN | WAIT_STREAM));
    const hm::mat Qm = hm::symmetrised(Q, n), Rm = hm::symmetrised(R, m), Sm = hm::symmetrised(S, m);
    const bool p_inst = P_per_instance != 0;
    hm::mat Pall((p_inst ? b : 1) * (size_t)n * n);
    for (size_t i = 0; i < (p_inst ? b : 1); ++i) {
        const hm::mat Pm = hm::symmetrised(P + i * n * n, n);
        std::copy(Pm.begin(), Pm.end(), Pall.begin() + i * n * n);
    }
    if (sq_struct && !h->batched_alloc) {   // the stage-wise QP needs no condensed operand: terminal weights and the flag words only
        HIP_TRY(h, h->bP.once(b * n * n));
        HIP_TRY(h, h->bFlag.once(b));
    } else
        ALMPC_TRY(ensure_batched_alloc(h));
    almpc_handle::Sqp& q = h->sqp;
    q.reset_keeping_switches();
    h->dXref.reset(); h->dUref.reset(); h->dFS.reset(); h->dV0S.reset(); h->dCold.reset(); h->cold_ref = false;
    h->ref_keep = false;
    std::vector<double> xr((size_t)n * (N + 1), 0.0), ur((size_t)nz, 0.0);
    if (xref) xr.assign(xref, xref + xr.size());
    if (uref) ur.assign(uref, uref + ur.size());
    HIP_TRY(h, upload_net(q, n, m, H, L, activation, net, W_in, W_h, b_h, W_out));
    HIP_TRY(h, q.A.alloc(b * N * n * n)); HIP_TRY(h, q.B.alloc(b * N * n * m)); HIP_TRY(h, q.c.alloc(b * N * n));
    HIP_TRY(h, q.fval.alloc(b * N * n)); HIP_TRY(h, q.ebar.alloc(b * N * n)); HIP_TRY(h, q.qadd.alloc(b * nz));
    HIP_TRY(h, q.xref.upload(xr.data(), xr.size())); HIP_TRY(h, q.uref.upload(ur.data(), ur.size()));
    HIP_TRY(h, q.Q.upload(Qm.data(), Qm.size())); HIP_TRY(h, q.R.upload(Rm.data(), Rm.size())); HIP_TRY(h, q.S.upload(Sm.data(), Sm.size()));
    HIP_TRY(h, q.bad.alloc(b));
    HIP_TRY(h, q.mer.alloc(4 * b));
    HIP_TRY(h, q.xback.alloc(b * (size_t)n * (N + 1))); HIP_TRY(h, q.dxback.alloc(b * (size_t)n * (N + 1)));
    HIP_TRY(h, q.uback.alloc(b * nz)); HIP_TRY(h, q.vback.alloc(b * nz));
    {
        double pm = 0.0;
        for (double v : Pall) pm = std::max(pm, std::fabs(v));
        for (double v : Qm) pm = std::max(pm, std::fabs(v));
        q.mu = 2.0 * pm;  // the multipliers of the dynamics are ~ 2 |P e|: exact for errors up to order one.  Measured on the benchmark
                          // set: 0.2 |P| rejects good steps near the solution, 10 |P| rejects every full step of some instances
    }
    HIP_TRY(h, hipMemset(q.bad, 0, b * sizeof(int)));
    HIP_TRY(h, h->dXref.alloc(b * (size_t)n * (N + 1))); HIP_TRY(h, h->dUref.alloc(b * nz));
    HIP_TRY(h, hipMemcpy(h->bP, Pall.data(), Pall.size() * sizeof(double), hipMemcpyHostToDevice));
    ALMPC_TRY(upload_input_box(h, umin, umax));
    if (h->batched_alloc) {   // the condensed route (also kept ready when a condensed handle sends its QPs to k_riccati after an earlier design)
        HIP_TRY(h, h->bQ.once(b * nz));
        HIP_TRY(h, h->dFS.alloc(b * nz)); HIP_TRY(h, h->dV0S.alloc(b * nz)); h->dCold.reset(); h->cold_ref = false;
        // F_i = 0 for an LTV design (the gradient is explicit), so F'_i and V_i stay zero; stage-0 model slots are unused but read
        HIP_TRY(h, hipMemset(h->bF, 0, b * nz * n * sizeof(double)));
        HIP_TRY(h, hipMemset(h->bFs, 0, b * n * nzs * sizeof(double)));
        HIP_TRY(h, hipMemset(h->bVs, 0, b * n * nzs * sizeof(double)));
        HIP_TRY(h, hipMemset(h->bA, 0, b * n * n * sizeof(double)));
        HIP_TRY(h, hipMemset(h->bB, 0, b * n * m * sizeof(double)));
    }
    q.useR = Rm[0] != 0.0; q.useS = q.useR && Sm[0] != 0.0; q.sP = p_inst ? (long)n * n : 0;
    h->P.assign(Pall.begin(), Pall.begin() + (size_t)n * n);
    keep_weights(h, nullptr, nullptr, Sm, q.useR != 0, q.useS != 0);
    h->rho = rho; h->sigma = sigma;
    // state rows (almpc_set_state_box: the box of .../fnn/mpc_modeler_implementation_fnn.jl:146-153; terminal equality): one
    // constraint-space matrix per instance, rebuilt with every iteration's linearisation
    const StateBox box = state_box(h);
    if (q.structured_qp) {   // no constraint-space matrix: the state rows are coordinates of the stage-wise trajectory (k_sdual)
        ALMPC_TRY(setup_state_rows(h, nullptr, nullptr, true));
        h->has_box = box.min ? 1 : 0;
        h->mc = box.min ? N * n : (h->terminal_eq ? n : 0);
    } else
        ALMPC_TRY(setup_state_rows(h, box.min, box.max, true));
    h->xref_stride = (long)n * (N + 1); h->uref_stride = nz; h->fS_stride = nz;
    h->designed = false;  // becomes true with the first iteration's design
    h->batched = true; h->ltv = true;
    h->r_batched_P = true; h->rP_stride = q.sP; h->bP_stride = q.sP; h->t_step = false;
    h->sd.ready = false;
    if (h->fallback || q.structured_qp) {
        // stage-wise QP of an iteration: k_sgains (stage records, defects' value-function terms, cost terms) + k_sdual; behind it, for
        // an input box without S, the primal Riccati active set
        ALMPC_TRY(setup_redo_solvers(h, nullptr, false, Qm, Rm, q.useS ? &Sm : nullptr, box, h->fallback == 1 || q.structured_qp,
                                     "sqp_fnn_setup: state rows / input-rate weight in the stage-wise QP need n + m <= 48 and (N + 1)(n + m) <= 4096"));
        if (h->sd.ready) {
            almpc_handle::Sd& sd = h->sd;
            const size_t TP = (size_t)sdual_tp(sd.NT, sd.MC, N);
            HIP_TRY(h, sd.base.grow(b * TP));
            sd.has_base = true; sd.base_stride = (long)TP;
            HIP_TRY(h, sd.pc.alloc(b * N * sd.NT)); HIP_TRY(h, sd.ct.alloc(b * N * sd.NT));
            sd.sqp = true;
        } else if (q.structured_qp && !primal_redo_covers(h, h->mc > 0, q.useS != 0))
            return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp_fnn_setup: the shape is outside both stage-wise QP solvers");
    }
    q.ready = true; q.started = false;
    return ALMPC_OK;
}
int almpc_sqp_fnn_setup(almpc_handle* h, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                        const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                        const double* S, const double* P, int P_per_instance, const double* umin, const double* umax, double rho,
                        double sigma) {
    return sqp_net_setup(h, false, H, L, activation, W_in, W_h, b_h, W_out, xref, uref, Q, R, S, P, P_per_instance, umin, umax, rho, sigma);
}
int almpc_sqp_densenet_setup(almpc_handle* h, int H, int L, int activation, const double* W_in, const double* W_h, const double* b_h,
                             const double* W_out, const double* xref, const double* uref, const double* Q, const double* R,
                             const double* S, const double* P, int P_per_instance, const double* umin, const double* umax, double rho,
                             double sigma) {
    return sqp_net_setup(h, true, H, L, activation, W_in, W_h, b_h, W_out, xref, uref, Q, R, S, P, P_per_instance, umin, umax, rho, sigma);
}

// The row multipliers' buffer, once the switch is on and the handle has state rows (zero: no QP solved yet)
static int sqp_rows_buffer(almpc_handle* h) {
    almpc_handle::Sqp& q = h->sqp;
    if (!q.row_mult || h->mc == 0 || q.smu) return ALMPC_OK;
    const size_t cnt = (size_t)h->batch * h->N * h->n;
    HIP_TRY(h, q.smu.alloc(cnt));
    HIP_TRY(h, hipMemset(q.smu, 0, cnt * sizeof(double)));
    return ALMPC_OK;
}

int almpc_sqp_fnn_start(almpc_handle* h, const double* x0, const double* u_guess) {
    if (!h || !x0) return h ? fail(h, ALMPC_ERR_INVALID, "sqp_fnn_start: null x0") : ALMPC_ERR_INVALID;
    almpc_handle::Sqp& q = h->sqp;
    if (!q.ready) return fail(h, ALMPC_ERR_NOT_DESIGNED, "sqp_fnn_start before sqp_fnn_setup");
    HIP_TRY(h, hipSetDevice(h->device));
    const int n = h->n, m = h->m, N = h->N, nz = h->nz;
    const size_t b = (size_t)h->batch;
    hipStream_t st = h->stream;
    HIP_TRY(h, hipStreamSynchronize(st));
    io_release_x0(h);
    HIP_TRY(h, hipMemcpy(h->dX0, x0, b * n * sizeof(double), hipMemcpyHostToDevice));
    // the start: the caller's guess or the input reference, clipped to the box
    std::vector<double> ug(b * nz), lo(m), hi(m);
    if (u_guess) ug.assign(u_guess, u_guess + b * nz);
    else {
        std::vector<double> ur(nz);
        HIP_TRY(h, hipMemcpy(ur.data(), q.uref, nz * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t t = 0; t < ug.size(); ++t) ug[t] = ur[t % nz];
    }
    HIP_TRY(h, hipMemcpy(lo.data(), h->dUmin, m * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(hi.data(), h->dUmax, m * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < ug.size(); ++t) ug[t] = std::min(std::max(ug[t], lo[t % m]), hi[t % m]);
    HIP_TRY(h, hipMemcpy(h->dUref, ug.data(), ug.size() * sizeof(double), hipMemcpyHostToDevice));
    FnnRolloutParams rp;
    rp.n = n; rp.m = m; rp.H = q.H; rp.L = q.L; rp.act = q.act; rp.N = N;
    rp.W_in = q.W_in; rp.W_h = q.W_h; rp.b_h = q.b_h; rp.W_out = q.W_out; rp.x0 = h->dX0; rp.ubar = h->dUref; rp.xbar = h->dXref;
    const size_t l = fnn_rollout_lds_doubles(n, m, q.H, q.L, q.net) * sizeof(double);
    void (*roll)(FnnRolloutParams) = with_net(q.net, [](auto k) { return k_fnn_rollout<k>; });
    if (l > 64 * 1024) HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(roll), (size_t)(l)));
    hipLaunchKernelGGL(roll, dim3((unsigned)b), dim3(256), l, st, rp);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemsetAsync(q.bad, 0, b * sizeof(int), st));
    ALMPC_TRY(sqp_rows_buffer(h));
    if (q.smu) HIP_TRY(h, hipMemsetAsync(q.smu, 0, b * N * (size_t)n * sizeof(double), st));   // (no QP solved yet)
    std::vector<double> d0(4 * b, 0.0);
    for (size_t i = 0; i < b; ++i) { d0[4 * i] = 1.0; d0[4 * i + 1] = std::numeric_limits<double>::infinity(); }
    HIP_TRY(h, hipMemcpyAsync(q.mer, d0.data(), d0.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    q.started = true; q.since_start = 0;
    return ALMPC_OK;
}

// almpc_sqp_fnn_solve's part of the loop (null for almpc_sqp_fnn_iterate): the stopping test and the frozen instances
struct SqpSolveCtl {
    double tol;
    int *done, *iters, *verdict, *live;   // device, see almpc_handle::Sqp::sv
    double* kkt;
    int* live_pin;                        // pinned [4]
    hipEvent_t ev[4];
};

// what the exact-Hessian mode covers: the condensed route, smooth activations, nz <= 128, the per-wave LDS scratch of k_fnn_lag_hessian
// within 64 KB for four waves; state rows only with their multipliers handed out (almpc_sqp_fnn_set_row_multipliers) and the stage-wise
// solvers behind the loop (an iteration whose shifted exact Hessian is indefinite takes the Gauss-Newton QP through k_sgains + k_sdual)
static int sqp_exact_check(almpc_handle* h) {
    const almpc_handle::Sqp& q = h->sqp;
    if (q.structured_qp || h->structured) return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp exact Hessian: the condensed QP route only");
    if (h->mc > 0 && !q.row_mult) return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp exact Hessian: no state rows (their multipliers would enter the adjoint)");
    if (h->mc > 0 && !(h->fallback && h->sd.ready && h->sd.sqp))
        return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp exact Hessian with state rows: needs the stage-wise fallback (k_sgains + k_sdual) for the "
                                              "iterations whose exact Hessian is indefinite; it is off or the shape is outside it");
    if (q.act == 1) return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp exact Hessian: relu makes the NLP non-smooth");
    if (h->nz > 128) return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp exact Hessian: nz <= 128");
    if (4 * fnn_hess_wave_doubles(h->n, h->m, q.H, q.L, q.net) * sizeof(double) > 64 * 1024)
        return fail(h, ALMPC_ERR_UNSUPPORTED, std::string("sqp exact Hessian: the ") + net_name(q.net) +
                                                  " network's per-wave scratch (its activation sites' Jacobians) must fit 16 KB of LDS");
    if (sqp_exact_lds_doubles(h->n, h->m, h->nz) * sizeof(double) > 64 * 1024)
        return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp exact Hessian: the network / stage scratch must fit 64 KB of LDS");
    return ALMPC_OK;
}

// k_sqp_prepare's and k_sqp_step's
static SqpParams sqp_step_params(const almpc_handle* h, double step_scale, const SqpSolveCtl* sv) {
    const almpc_handle::Sqp& q = h->sqp;
    SqpParams sp;
    sp.n = h->n; sp.m = h->m; sp.N = h->N; sp.nz = h->nz; sp.batch = h->batch; sp.useR = q.useR; sp.useS = q.useS;
    sp.xref = q.xref; sp.uref = q.uref; sp.R = q.R; sp.S = q.S; sp.umin = h->dUmin; sp.umax = h->dUmax;
    sp.xbar = h->dXref; sp.ubar = h->dUref; sp.fval = q.fval; sp.A = q.A; sp.B = q.B; sp.c = q.c; sp.ebar = q.ebar; sp.qadd = q.qadd;
    sp.v = h->dEu; sp.flag = h->bFlag; sp.status = h->dStatus; sp.bad = q.bad; sp.stats = q.stats; sp.step_scale = step_scale;
    sp.x = h->dX; sp.ex = h->dEx; sp.u = h->dU; sp.eu = h->dEu; sp.adaptive = q.step_rule; sp.mu = q.mu; sp.Q = q.Q; sp.P = h->bP; sp.sP = q.sP; sp.mer = q.mer;
    sp.xback = q.xback; sp.uback = q.uback; sp.dxback = q.dxback; sp.vback = q.vback;
    if (sv) { sp.done = sv->done; sp.verdict = sv->verdict; }
    return sp;
}
// What the iterations of one call launch with, made once by sqp_plan: the route decisions, the LDS sizes and every kernel's parameters
struct SqpCall {
    const almpc_opts* opts; const SqpSolveCtl* sv;
    bool exact = false, ltv_scales = false, prep_in_design = false; size_t step_lds = 0, hess_lds = 0, exact_lds = 0;
    RowMultOut rows; DesignStrides ds; FnnParams fp; SqpParams sp; SqpKktParams kp; DesignLtvParams lp; FnnHessParams hp; SqpExactParams xp;
};
static int sqp_plan(almpc_handle* h, double step_scale, SqpCall& c) {
    almpc_handle::Sqp& q = h->sqp;
    const SqpSolveCtl* sv = c.sv;
    const int n = h->n, m = h->m, N = h->N, nz = h->nz;
    const size_t b = (size_t)h->batch;
    c.ds = batched_strides(h, q.sP != 0);
    c.step_lds = sqp_step_lds_doubles(n, m, N) * sizeof(double);
    if (c.step_lds > 64 * 1024) HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_sqp_step), (size_t)(c.step_lds)));
    c.fp = fnn_points(fnn_params(h, q), h->dXref, h->dUref, N, (long)n * (N + 1), nz, q.A, q.B, q.fval);
    c.fp.batch = (int)(b * N);   // (every stage of every instance is a point)
    c.sp = sqp_step_params(h, step_scale, sv);
    if (sv && c.step_lds > 64 * 1024) HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_sqp_kkt), (size_t)(c.step_lds)));
    // state rows with almpc_sqp_fnn_set_row_multipliers: whichever finish decides an instance's QP hands its row multipliers out, and the
    // adjoint walk of k_sqp_kkt (the stopping test, the multipliers of the exact Hessian) takes them in
    if (q.row_mult && h->mc > 0) {
        if (q.structured_qp)
            return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp row multipliers: the condensed QP route only (the stage-wise route of "
                                                  "almpc_sqp_fnn_set_structured / ALMPC_FLAG_STRUCTURED does not hand them out)");
        ALMPC_TRY(sqp_rows_buffer(h));
        c.rows.mu = q.smu; c.rows.done = sv ? sv->done : nullptr; c.rows.mer = q.step_rule ? q.mer : nullptr;
    }
    DesignLtvParams& lp = c.lp;
    lp.n = n; lp.m = m; lp.N = N; lp.nz = nz; lp.useR = q.useR; lp.useS = q.useS;
    lp.A = q.A; lp.B = q.B; lp.c = q.c; lp.ebar = q.ebar; lp.P = h->bP; lp.sP = q.sP; lp.Q = q.Q; lp.R = q.R; lp.S = q.S;
    lp.qadd = q.qadd; lp.H = h->bH; lp.q = h->bQ;
    c.exact = q.hessian == 1;
    if (c.exact) {
        ALMPC_TRY(sqp_exact_check(h));
        HIP_TRY(h, q.lam.once(b * N * (size_t)n)); HIP_TRY(h, q.Wlag.once(b * N * (size_t)(n + m) * (n + m)));
        if (!sv && c.step_lds > 64 * 1024) HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_sqp_kkt), (size_t)(c.step_lds)));
        FnnHessParams& hp = c.hp; SqpExactParams& xp = c.xp;
        hp.n = n; hp.m = m; hp.H = q.H; hp.L = q.L; hp.act = q.act; hp.N = N; hp.batch = h->batch;
        hp.W_in = q.W_in; hp.W_h = q.W_h; hp.b_h = q.b_h; hp.W_out = q.W_out; hp.xbar = h->dXref; hp.ubar = h->dUref; hp.lam = q.lam;
        hp.done = sv ? sv->done : nullptr; hp.W = q.Wlag;
        xp.n = n; xp.m = m; xp.N = N; xp.nz = nz; xp.A = q.A; xp.B = q.B; xp.c = q.c; xp.W = q.Wlag; xp.ubar = h->dUref;
        xp.umin = h->dUmin; xp.umax = h->dUmax; xp.done = sv ? sv->done : nullptr; xp.H = h->bH; xp.q = h->bQ;
        c.hess_lds = 4 * fnn_hess_wave_doubles(n, m, q.H, q.L, q.net) * sizeof(double); c.exact_lds = sqp_exact_lds_doubles(n, m, nz) * sizeof(double);
    }
    if (sv || c.exact) {   // k_sqp_kkt: the stopping test of almpc_sqp_fnn_solve, or (sv null) the multipliers only: its adjoint walk without the test
        SqpKktParams& kp = c.kp;
        kp.n = n; kp.m = m; kp.N = N; kp.nz = nz; kp.useS = q.useS;
        kp.xref = q.xref; kp.uref = q.uref; kp.Q = q.Q; kp.R = q.R; kp.S = q.S; kp.P = h->bP; kp.sP = q.sP;
        kp.umin = h->dUmin; kp.umax = h->dUmax; kp.xbar = h->dXref; kp.ubar = h->dUref; kp.fval = q.fval; kp.A = q.A; kp.B = q.B;
        kp.tol = sv ? sv->tol : 0.0; kp.it = 0;
        kp.done = sv ? sv->done : nullptr; kp.iters = sv ? sv->iters : nullptr; kp.kkt = sv ? sv->kkt : nullptr; kp.live = sv ? sv->live : nullptr;
        if (c.exact) kp.lam = q.lam;
        if (c.rows.mu) { kp.mu = q.smu; kp.term_eq = h->terminal_eq ? 1 : 0; }
        if (c.rows.mu && h->has_box) { kp.xmin = h->dXmin; kp.xmax = h->dXmax; }
    }
    // register-tile design kernel: scaling, scaled gradient and the flag reset ride along as its tail (three launches less per iteration)
    // (not in exact mode: k_sqp_exact_qp changes H and q after the design, the factor then scales them)
    c.ltv_scales = !c.exact && ltv_reg_path(h) && nz <= 128 && !q.structured_qp && !h->sw.dbg_split_scale;
    if (c.ltv_scales) { lp.sc_d = h->bD; lp.sc_Hs = h->bHs; lp.sc_fS = h->dFS; lp.sc_flag = h->bFlag; lp.nzs = h->nzs; }
    // ... and k_sqp_prepare as its head (its outputs are that kernel's inputs): a fourth launch less
    c.prep_in_design = c.ltv_scales && !h->sw.dbg_split_prepare;
    if (c.prep_in_design) { lp.prep_on = 1; lp.prep = c.sp; }
    return ALMPC_OK;
}

// Jacobians and network outputs at the iterate (into q.A, q.B, q.fval); the stopping test at the top of iteration `it`, its live count into
// the pinned ring; unless `last`: the exact mode's multipliers (from the test, or the walk alone) and Hessians, the stage data, the flag reset
static int sqp_linearise(almpc_handle* h, const SqpCall& c, int it, bool last) {
    const almpc_handle::Sqp& q = h->sqp;
    const size_t b = (size_t)h->batch;
    hipStream_t st = h->stream;
    HIP_TRY(h, launch_fnn_jacobian(h->sw, c.fp, q.net, h->num_cus, st));
    if (c.sv || (c.exact && !last)) {
        SqpKktParams kp = c.kp; kp.it = c.sv ? it : 0;
        hipLaunchKernelGGL(k_sqp_kkt, dim3((unsigned)b), dim3(256), c.step_lds, st, kp);
    }
    if (c.sv) {
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(c.sv->live_pin + (it & 3), c.sv->live, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipEventRecord(c.sv->ev[it & 3], st));
    }
    if (last) return ALMPC_OK;
    if (c.exact) {
        void (*hk)(FnnHessParams) = with_net(q.net, [](auto k) { return k_fnn_lag_hessian<k>; });
        hipLaunchKernelGGL(hk, dim3((unsigned)((b * h->N + 3) / 4)), dim3(256), c.hess_lds, st, c.hp);
        HIP_TRY(h, hipGetLastError());
    }
    if (!c.prep_in_design) hipLaunchKernelGGL(k_sqp_prepare, dim3((unsigned)b), dim3(256), 0, st, c.sp);
    if (!c.ltv_scales) HIP_TRY(h, hipMemsetAsync(h->bFlag, 0, b * sizeof(int), st));
    return ALMPC_OK;
}

// The QP in its stage-wise form for every instance; start: v = 0 (working set = the iterate's inputs on a bound)
static int sqp_qp_stagewise(almpc_handle* h, const SqpCall& c) {
    const almpc_handle::Sqp& q = h->sqp;
    h->designed = true;
    // input box without S: the primal Riccati active set (an iterate of this loop has about half of its inputs on a bound: rows a
    // primal method holds at no cost, while the dual one pays a sweep per row of its start -- measured 0.56 against 3.1 ms per
    // iteration at the configs[4] shape); with state rows / S: k_sgains + k_sdual
    SolveCall qp;
    qp.guess = h->dUref; qp.max_iter = c.opts ? c.opts->polish_max_iter : 0;
    if (h->mc == 0 && !q.useS && h->rKst) {
        qp.filter = FILTER_SQP_ALL;
        HIP_TRY(h, launch_riccati(h, qp));
    } else if (h->sd.ready) {
        qp.first_tier = h->nz > 48 ? 1 : 0;
        HIP_TRY(h, launch_sgains(h));
        HIP_TRY(h, launch_sdual(h, qp));
    } else
        return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp_fnn_iterate: no stage-wise QP solver for this design");
    return ALMPC_OK;
}

// The condensed QP: design, exact H and q, factor, constraint-space matrix, scaled gradient, v0, step; behind it the redo of the flagged
static int sqp_qp_condensed(almpc_handle* h, const SqpCall& c) {
    const almpc_handle::Sqp& q = h->sqp;
    const int nz = h->nz, nzs = h->nzs;
    const size_t b = (size_t)h->batch;
    hipStream_t st = h->stream;
    HIP_TRY(h, launch_design_ltv(h, c.lp, st));
    if (c.exact) {   // H, q of the exact QP (an instance whose result is not positive definite is flagged by the factor and, with the
                     // structured fallback on, takes the Gauss-Newton QP in its stage-wise form)
        hipLaunchKernelGGL(k_sqp_exact_qp, dim3((unsigned)b), dim3(256), c.exact_lds, st, c.xp);
        HIP_TRY(h, hipGetLastError());
    }
    StepMode mode;
    mode.guess = (!h->sw.sqp_admm_always && q.since_start > 0) ? Guess::FromIterate : Guess::Admm; mode.rows = c.rows;
    // (with the scaling in the design kernel's tail fS_i exists before the inverse: v0S_i = -G_i fS_i comes out of the inverse's launch)
    const bool v0_in_inverse = c.ltv_scales && design_inverse_makes_v(h->sw, nz);
    launch_batched_factor(h, c.ds, h->rho, h->sigma, st, mode.guess != Guess::Admm, c.ltv_scales, false, v0_in_inverse ? h->dFS : nullptr, h->dV0S);
    if (h->mc > 0) HIP_TRY(h, launch_ghat_inst(h, q.A, q.B));
    if (!c.ltv_scales) hipLaunchKernelGGL(k_fs_scale, dim3(256), dim3(256), 0, st, h->batch, nz, nzs, h->bQ, (long)nz, h->bD, h->dFS);
    if (!v0_in_inverse) hipLaunchKernelGGL(k_neg_gm, dim3(1, (unsigned)b), dim3(256), 0, st, nz, nzs, 1, nz, h->bG, h->dFS, h->dV0S, (long)nz * nzs, (long)nz);
    HIP_TRY(h, hipGetLastError());
    h->designed = true;
    ALMPC_TRY(calculate_checked(h, c.opts, mode));
    // structured fallback: an instance whose condensed Hessian came out indefinite to working precision (open-loop unstable
    // linearisation over the horizon) or whose QP was left unsolved gets this iteration's QP solved in its stage-wise form
    if (!h->fallback) return ALMPC_OK;
    // input box without S: the primal Riccati active set alone -- the solver this loop's stage-wise QP route uses for such problems
    // (an iterate holds half of its inputs on bounds; a saturated unstable linearisation is where the dual method has no
    // certificate) --, ONE idle launch per iteration instead of three; with state rows / S: k_sgains + k_sdual
    const bool primal_only = h->mc == 0 && !q.useS && h->rKst && !h->sw.sqp_redo_dual_first;
    SolveCall flagged;
    flagged.filter = FILTER_SQP_FLAGGED; flagged.single_launch = true; flagged.rows = c.rows;   // (the last two: k_sdual's)
    if (h->sd.ready && !primal_only) { HIP_TRY(h, launch_sgains(h, flagged)); HIP_TRY(h, launch_sdual(h, flagged)); }
    if (h->mc == 0 && !q.useS && h->rKst) HIP_TRY(h, launch_riccati(h, flagged));
    return ALMPC_OK;
}

static int sqp_loop(almpc_handle* h, int iters, double step_scale, const almpc_opts* opts, double* step_inf, double* defect_inf,
                    const SqpSolveCtl* sv) {
    almpc_handle::Sqp& q = h->sqp;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    if (q.stats && q.stats.size() < (size_t)2 * iters) HIP_TRY(h, hipStreamSynchronize(st));   // (the buffer is replaced: its last reader first)
    HIP_TRY(h, q.stats.grow((size_t)2 * std::max(iters, 1)));
    HIP_TRY(h, hipMemsetAsync(q.stats, 0, (size_t)2 * iters * sizeof(unsigned long long), st));
    SqpCall c; c.opts = opts; c.sv = sv;
    ALMPC_TRY(sqp_plan(h, step_scale, c));
    bool all_done = false;
    for (int it = 0; it < iters; ++it) {
        if (sv && it >= 2) {   // every live instance had converged at the top of iteration it - 2: the rest is frozen work
            HIP_TRY(h, hipEventSynchronize(sv->ev[(it - 2) & 3]));
            if (sv->live_pin[(it - 2) & 3] == 0) { all_done = true; break; }
        }
        ALMPC_TRY(sqp_linearise(h, c, it, false));
        ALMPC_TRY(q.structured_qp ? sqp_qp_stagewise(h, c) : sqp_qp_condensed(h, c));
        q.since_start += 1;   // the update behind either QP route; its step and defect norms go to the iteration's slot of the histories
        c.sp.stats = q.stats + 2 * it;
        hipLaunchKernelGGL(k_sqp_step, dim3((unsigned)h->batch), dim3(256), c.step_lds, st, c.sp);
        HIP_TRY(h, hipGetLastError());
    }
    if (sv && !all_done) ALMPC_TRY(sqp_linearise(h, c, iters, true));   // the last test, at the final iterate
    if (sv) return almpc_synchronize(h);   // (per-instance verdicts instead of ALMPC_ERR_NUMERIC; no histories)
    // the histories of almpc_sqp_fnn_iterate and its verdict: ALMPC_ERR_NUMERIC names the first instance that skipped an iteration
    const size_t b = (size_t)h->batch;
    std::vector<unsigned long long> stats((size_t)2 * iters);
    std::vector<int> bad(b);
    HIP_TRY(h, hipMemcpyAsync(stats.data(), q.stats, stats.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(bad.data(), q.bad, b * sizeof(int), hipMemcpyDeviceToHost, st));
    ALMPC_TRY(almpc_synchronize(h));
    for (int it = 0; it < iters; ++it) {
        if (step_inf) std::memcpy(&step_inf[it], &stats[2 * it], 8);
        if (defect_inf) std::memcpy(&defect_inf[it], &stats[2 * it + 1], 8);
    }
    for (size_t i = 0; i < b; ++i)
        if (bad[i])
            return fail(h, ALMPC_ERR_NUMERIC, "sqp_fnn_iterate: instance " + std::to_string(i) +
                        ": an iteration was skipped (condensed Hessian not positive definite to working precision, a non-finite QP "
                        "solution, or -- with state rows -- an infeasible QP); its iterate is the last good one, the other instances are unaffected");
    return ALMPC_OK;
}

int almpc_sqp_fnn_set_hessian(almpc_handle* h, int mode) {
    if (!h) return ALMPC_ERR_INVALID;
    if (mode != 0 && mode != 1) return fail(h, ALMPC_ERR_INVALID, "sqp_fnn_set_hessian: 0 (Gauss-Newton) or 1 (exact)");
    if (mode == 1 && h->sqp.ready) { const int rc = sqp_exact_check(h); if (rc != ALMPC_OK) return rc; }
    h->sqp.hessian = mode;
    return ALMPC_OK;
}

int almpc_sqp_fnn_iterate(almpc_handle* h, int iters, double step_scale, const almpc_opts* opts, double* step_inf, double* defect_inf) {
    if (!h) return ALMPC_ERR_INVALID;
    almpc_handle::Sqp& q = h->sqp;
    if (!q.ready || !q.started) return fail(h, ALMPC_ERR_NOT_DESIGNED, "sqp_fnn_iterate needs sqp_fnn_setup and sqp_fnn_start");
    if (iters < 1 || !(step_scale > 0.0 && step_scale <= 1.0)) return fail(h, ALMPC_ERR_INVALID, "sqp_fnn_iterate: iters >= 1, 0 < step_scale <= 1");
    return sqp_loop(h, iters, step_scale, opts, step_inf, defect_inf, nullptr);
}

// Solve to a tolerance: at the top of every iteration k_sqp_kkt tests each live instance at its iterate (after the linearisation, which
// computes the network outputs and Jacobians there anyway) and freezes those that pass; k_sqp_prepare and k_sqp_step leave a frozen
// instance alone, so its iterate and results stay bit-identical from then on.  The live count is copied into a pinned ring after
// every test and read by the host two iterations later (the device has more than an iteration queued by then: no bubble); the loop
// ends when it reaches 0 or after max_iters iterations, followed by one last test at the final iterate.
int almpc_sqp_fnn_solve(almpc_handle* h, int max_iters, double tol, const almpc_opts* opts, int32_t* status, int32_t* iters, double* kkt) {
    if (!h) return ALMPC_ERR_INVALID;
    almpc_handle::Sqp& q = h->sqp;
    if (!q.ready || !q.started) return fail(h, ALMPC_ERR_NOT_DESIGNED, "sqp_fnn_solve needs sqp_fnn_setup and sqp_fnn_start");
    if (max_iters < 1 || !(tol > 0.0)) return fail(h, ALMPC_ERR_INVALID, "sqp_fnn_solve: max_iters >= 1, tol > 0");
    if (!q.useR) return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp_fnn_solve: the stopping test scales the gradient by 1 / (2 R_aa): R[0,0] must not be 0");
    if (h->m > 64) return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp_fnn_solve: m <= 64 (one lane per input in the adjoint walk)");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t b = (size_t)h->batch;
    hipStream_t st = h->stream;
    HIP_TRY(h, hipStreamSynchronize(st));
    HIP_TRY(h, q.sv.once(3 * b + 1)); HIP_TRY(h, q.kkt.once(b));
    HIP_TRY(h, q.live_pin.once(4));
    SqpSolveCtl sv;
    sv.tol = tol; sv.done = q.sv; sv.iters = q.sv + b; sv.verdict = q.sv + 2 * b; sv.live = q.sv + 3 * b; sv.kkt = q.kkt;
    sv.live_pin = q.live_pin;
    {
        std::vector<int> init(3 * b + 1, 0);
        for (size_t i = 0; i < b; ++i) init[2 * b + i] = 1;   // verdict: iteration limit unless converged / skipped
        init[3 * b] = (int)b;
        HIP_TRY(h, hipMemcpy(q.sv, init.data(), init.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    for (auto& e : sv.ev) e = nullptr;
    int rc = ALMPC_OK;
    for (auto& e : sv.ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { rc = fail(h, ALMPC_ERR_HIP, "sqp_fnn_solve: hipEventCreate"); break; }
    if (rc == ALMPC_OK) rc = sqp_loop(h, max_iters, 1.0, opts, nullptr, nullptr, &sv);
    for (auto& e : sv.ev)
        if (e) (void)hipEventDestroy(e);
    if (rc != ALMPC_OK) return rc;
    std::vector<int> w(3 * b);
    std::vector<double> r(b);
    HIP_TRY(h, hipMemcpy(w.data(), q.sv, w.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(r.data(), q.kkt, b * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < b; ++i) {
        if (status) status[i] = w[i] ? 0 : w[2 * b + i];
        if (iters) iters[i] = w[b + i];
        if (kkt) kkt[i] = r[i];
    }
    return ALMPC_OK;
}

int almpc_sqp_fnn_set_structured(almpc_handle* h, int on) {
    if (!h) return ALMPC_ERR_INVALID;
    if (on && !riccati_shape_ok(h) && !sdual_shape_ok(h->n, h->m, h->N, false))
        return fail(h, ALMPC_ERR_UNSUPPORTED, "sqp_fnn_set_structured: the shape is outside both stage-wise QP solvers");
    h->sqp.structured_qp = on ? 1 : 0;
    h->designed = false;   // takes effect at the next almpc_sqp_fnn_setup
    h->sqp.ready = h->sqp.started = false;
    return ALMPC_OK;
}

int almpc_sqp_fnn_set_step_rule(almpc_handle* h, int rule) {
    if (!h) return ALMPC_ERR_INVALID;
    if (rule != 0 && rule != 1) return fail(h, ALMPC_ERR_INVALID, "sqp_fnn_set_step_rule: 0 (fixed step) or 1 (merit-function safeguard)");
    h->sqp.step_rule = rule;
    return ALMPC_OK;
}

int almpc_sqp_fnn_set_row_multipliers(almpc_handle* h, int on) {
    if (!h) return ALMPC_ERR_INVALID;
    h->sqp.row_mult = on ? 1 : 0;
    return ALMPC_OK;
}

int almpc_sqp_fnn_state_multipliers(almpc_handle* h, double* mu) {
    if (!h || !mu) return ALMPC_ERR_INVALID;
    if (!h->sqp.ready) return fail(h, ALMPC_ERR_NOT_DESIGNED, "sqp_fnn_state_multipliers before sqp_fnn_setup");
    const size_t cnt = (size_t)h->batch * h->N * h->n;
    if (!h->sqp.smu) {   // switch off, no state rows, or nothing started yet: no row has a multiplier
        std::fill(mu, mu + cnt, 0.0);
        return ALMPC_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(mu, h->sqp.smu, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

int almpc_sqp_fnn_skipped(almpc_handle* h, int32_t* skipped) {
    if (!h || !skipped) return ALMPC_ERR_INVALID;
    if (!h->sqp.ready) return fail(h, ALMPC_ERR_NOT_DESIGNED, "sqp_fnn_skipped before sqp_fnn_setup");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(skipped, h->sqp.bad, (size_t)h->batch * sizeof(int), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

int almpc_get_design_instance(almpc_handle* h, int instance, double* H, double* F, double* d) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->designed || !h->batched) return fail(h, ALMPC_ERR_NOT_DESIGNED, "get_design_instance needs almpc_design_batched");
    if (instance < 0 || instance >= h->batch) return fail(h, ALMPC_ERR_INVALID, "get_design_instance: instance out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t nz = h->nz, n = h->n, i = (size_t)instance;
    if (H) HIP_TRY(h, hipMemcpy(H, h->bH + i * nz * nz, nz * nz * sizeof(double), hipMemcpyDeviceToHost));
    if (F) HIP_TRY(h, hipMemcpy(F, h->bF + i * nz * n, nz * n * sizeof(double), hipMemcpyDeviceToHost));
    if (d) HIP_TRY(h, hipMemcpy(d, h->bD + i * h->nzs, nz * sizeof(double), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

int almpc_set_terminal_weight(almpc_handle* h, int mode) {
    if (!h) return ALMPC_ERR_INVALID;
    if (mode != ALMPC_TERMINAL_GIVEN && mode != ALMPC_TERMINAL_DARE_DEVICE) return fail(h, ALMPC_ERR_INVALID, "set_terminal_weight: mode must be 0 or 1");
    h->terminal_mode = mode;   // (read by the next almpc_design_batched / almpc_relin_fnn_setup)
    return ALMPC_OK;
}

int almpc_set_model_time(almpc_handle* h, int mode, double Ts) {
    if (!h) return ALMPC_ERR_INVALID;
    if (mode != ALMPC_MODEL_DISCRETE && mode != ALMPC_MODEL_CONTINUOUS_ZOH) return fail(h, ALMPC_ERR_INVALID, "set_model_time: mode must be 0 or 1");
    if (mode == ALMPC_MODEL_CONTINUOUS_ZOH && !(Ts > 0.0 && std::isfinite(Ts))) return fail(h, ALMPC_ERR_INVALID, "set_model_time: the sample time must be positive and finite");
    h->model_mode = mode;   // (read by the next design / almpc_relin_*_setup)
    h->model_Ts = mode == ALMPC_MODEL_CONTINUOUS_ZOH ? Ts : 0.0;
    return ALMPC_OK;
}

int almpc_get_model_instance(almpc_handle* h, int instance, double* A, double* B) {
    if (!h || (!A && !B)) return ALMPC_ERR_INVALID;
    if (!h->designed && !h->relin.ready) return fail(h, ALMPC_ERR_NOT_DESIGNED, "get_model_instance before a design");
    if (instance < 0 || instance >= h->batch) return fail(h, ALMPC_ERR_INVALID, "get_model_instance: instance out of range");
    if (h->ltv) return fail(h, ALMPC_ERR_UNSUPPORTED, "get_model_instance: a time-varying design has no single model per instance");
    const size_t nn = (size_t)h->n * h->n, nm = (size_t)h->n * h->m;
    const bool pi = h->batched && h->bA && h->bB;   // one model per instance, else the shared one
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (A) HIP_TRY(h, hipMemcpy(A, pi ? h->bA + (size_t)instance * nn : h->dA.get(), nn * sizeof(double), hipMemcpyDeviceToHost));
    if (B) HIP_TRY(h, hipMemcpy(B, pi ? h->bB + (size_t)instance * nm : h->dB.get(), nm * sizeof(double), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

int almpc_relin_fnn_terminal_status(almpc_handle* h, int32_t* st) {
    if (!h || !st) return ALMPC_ERR_INVALID;
    if (!h->relin.ready || !h->t_step)
        return fail(h, ALMPC_ERR_NOT_DESIGNED, "relin_fnn_terminal_status needs almpc_set_terminal_weight(ALMPC_TERMINAL_DARE_DEVICE) before almpc_relin_fnn_setup");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(st, h->tStat, (size_t)h->batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < h->batch; ++i) st[i] = st[i] != 0 ? 1 : 0;
    return ALMPC_OK;
}

int almpc_get_terminal_weight_instance(almpc_handle* h, int instance, double* P) {
    if (!h || !P) return ALMPC_ERR_INVALID;
    if (!h->designed && !h->relin.ready) return fail(h, ALMPC_ERR_NOT_DESIGNED, "get_terminal_weight_instance before a design");
    if (instance < 0 || instance >= h->batch) return fail(h, ALMPC_ERR_INVALID, "get_terminal_weight_instance: instance out of range");
    const size_t nn = (size_t)h->n * h->n;
    if (!h->batched || !h->bP) {   // shared model: one weight
        if (h->P.size() != nn) return fail(h, ALMPC_ERR_NOT_DESIGNED, "get_terminal_weight_instance before a design");
        std::memcpy(P, h->P.data(), nn * sizeof(double));
        return ALMPC_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(P, h->bP + (size_t)instance * (size_t)h->bP_stride, nn * sizeof(double), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

int almpc_set_reference(almpc_handle* h, const double* xref, const double* uref, int per_instance) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, "set_reference before design");
    if (h->ltv) return fail(h, ALMPC_ERR_INVALID, "set_reference: the references of an LTV design are arguments of almpc_design_ltv");
    if (h->relin.ready)
        return fail(h, ALMPC_ERR_INVALID, "set_reference: the references of the re-linearisation pipeline are arguments of almpc_relin_fnn_setup");
    if (!xref || !uref) return fail(h, ALMPC_ERR_INVALID, "set_reference: null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    const int n = h->n, m = h->m, N = h->N, nz = h->nz;
    const size_t cnt = per_instance ? (size_t)h->batch : 1;
    const size_t xs = (size_t)n * (N + 1), us = (size_t)nz;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->structured) {
        h->designed = false;
        HIP_TRY(h, h->dXref.alloc(cnt * xs));
        HIP_TRY(h, h->dUref.alloc(cnt * us));
        HIP_TRY(h, hipMemcpy(h->dXref, xref, cnt * xs * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->dUref, uref, cnt * us * sizeof(double), hipMemcpyHostToDevice));
        h->xref_stride = per_instance ? (long)xs : 0;
        h->uref_stride = per_instance ? (long)us : 0;
        ALMPC_TRY(sdual_update_base(h, uref, cnt));
        h->designed = true;
        return ALMPC_OK;
    }
    h->sqp.ready = h->sqp.started = false;  // the SQP iterate lived in the reference buffers released here
    h->relin.ready = false;                 // ... and so did the re-linearisation pipeline's references
    h->designed = false;                    // the reference buffers are replaced below: designed again on success only
    const size_t fcnt = h->batched ? (size_t)h->batch : cnt;  // per-instance models: fS depends on d_i
    // (a re-design or a new reference of the same shape keeps the four buffers: hipFree + hipMalloc cost ~0.1 ms each)
    // the exact policy, over the four together: buffers another entry point made, or one size that moved, replace them all
    if (!(h->ref_keep && h->dXref.size() == cnt * xs && h->dUref.size() == cnt * us && h->dFS.size() == fcnt * us && h->dV0S.size() == fcnt * us)) {
        h->dXref.reset(); h->dUref.reset(); h->dFS.reset(); h->dV0S.reset();
    }
    h->cold_ref = false;
    HIP_TRY(h, h->dXref.once(cnt * xs));
    HIP_TRY(h, h->dUref.once(cnt * us));
    HIP_TRY(h, h->dFS.once(fcnt * us));
    HIP_TRY(h, h->dV0S.once(fcnt * us));
    h->ref_keep = true;
    HIP_TRY(h, hipMemcpy(h->dXref, xref, cnt * xs * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->dUref, uref, cnt * us * sizeof(double), hipMemcpyHostToDevice));
    // fS = d .* (2 D'Sbar D u_ref): the input-rate cost is on u, not e_u (src/sub/design_mpc.jl:423-446)
    // (per-instance weights with an input-rate term: one vector per instance, from S_i, whatever the reference's form)
    const bool s_inst = h->weighted && h->kept.useS && h->wiS_given;
    const size_t gcnt = s_inst ? (size_t)h->batch : cnt;
    std::vector<double> fS(gcnt * us, 0.0);
    if (h->kept.useS) {  // S counts only together with R (the reference's branch rule, src/sub/design_mpc.jl:423-466), as in the design kernels
        for (size_t c = 0; c < gcnt; ++c) {
            const double* ur = uref + (per_instance ? c : 0) * us;
            const double* Sw = s_inst ? h->hSi + c * m * m : h->kept.S.data();
            double* f = fS.data() + c * us;
            for (int i = 0; i + 1 < N; ++i)
                for (int a = 0; a < m; ++a) {
                    double sd = 0.0;  // (S (u_i - u_{i+1}))_a
                    for (int b2 = 0; b2 < m; ++b2) sd += Sw[(size_t)b2 * m + a] * (ur[i * m + b2] - ur[(i + 1) * m + b2]);
                    f[i * m + a] += 2.0 * sd;
                    f[(i + 1) * m + a] -= 2.0 * sd;
                }
            if (!h->batched)
                for (int r = 0; r < nz; ++r) f[r] *= h->d[r];
        }
    }
    if (h->batched && !h->kept.useS) {   // no input-rate weight: fS_i = 0 and v0S_i = -G_i fS_i = 0 (no pass over the 0.5 GB of G_i)
        HIP_TRY(h, hipMemsetAsync(h->dFS, 0, fcnt * us * sizeof(double), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->dV0S, 0, fcnt * us * sizeof(double), h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else if (h->batched) {  // fS_i = d_i .* g and v0S_i = -G_i fS_i on the device, one vector per instance
        DevBuf<double> dGs;
        HIP_TRY(h, dGs.alloc(gcnt * us));
        hipError_t e = hipMemcpy(dGs, fS.data(), gcnt * us * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_fs_scale, dim3(256), dim3(256), 0, h->stream, h->batch, nz, h->nzs, dGs, (per_instance || s_inst) ? (long)us : 0L,
                               h->bD, h->dFS);
            hipLaunchKernelGGL(k_neg_gm, dim3(1, (unsigned)h->batch), dim3(256), 0, h->stream, nz, h->nzs, 1, (int)us, h->bG, h->dFS,
                               h->dV0S, (long)nz * h->nzs, (long)us);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        }
        if (e != hipSuccess) return fail(h, ALMPC_ERR_HIP, std::string("set_reference (batched): ") + hipGetErrorString(e));
    } else {
    HIP_TRY(h, hipMemcpy(h->dFS, fS.data(), cnt * us * sizeof(double), hipMemcpyHostToDevice));
    // v0S = -G fS: constant part of the polish's unconstrained minimiser (k_admm adds the part linear in e0)
    {
        const size_t blocks = (cnt * us + 255) / 256;
        // shared reference: the same launch makes wS = -Minv fS (constant part of the cold start's first ADMM iterate) and the
        // prologue's row-constant table, behind W in the workspace the design left
        NegGmExtra cold;
        const size_t w = (size_t)n * h->nzs;
        if (!per_instance && h->dCold && h->dMinv && h->dCold.size() >= w + 9 * (size_t)h->nzs) {
            cold.G2 = h->dMinv; cold.Out2 = h->dCold + w; cold.tab = h->dCold + w + h->nzs;
            cold.m = m; cold.dvec = h->dD; cold.rhovec = h->dRho; cold.umin = h->dUmin; cold.umax = h->dUmax; cold.uref = h->dUref;
            h->cold_ref = true;
        }
        hipLaunchKernelGGL(k_neg_gm, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, h->stream, nz, h->nzs,
                           (int)cnt, (int)us, h->dG, h->dFS, h->dV0S, 0L, 0L, cold);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    }
    h->xref_stride = per_instance ? (long)xs : 0;
    h->uref_stride = per_instance ? (long)us : 0;
    h->fS_stride = (per_instance || h->batched) ? (long)us : 0;
    ALMPC_TRY(sdual_update_base(h, uref, cnt));
    ALMPC_TRY(build_s0_basis(h));   // (v0S has changed)
    h->designed = true;
    return ALMPC_OK;
}

int almpc_update_initialization(almpc_handle* h, const double* x0) {
    if (!h || !x0) return h ? fail(h, ALMPC_ERR_INVALID, "update_initialization: null x0") : ALMPC_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    io_release_x0(h);
    HIP_TRY(h, hipMemcpyAsync(h->dX0, x0, (size_t)h->batch * h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return ALMPC_OK;
}

int almpc_update_initialization_device(almpc_handle* h, const double* d_x0) {
    if (!h || !d_x0) return h ? fail(h, ALMPC_ERR_INVALID, "update_initialization_device: null x0") : ALMPC_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    io_release_x0(h);
    HIP_TRY(h, hipMemcpyAsync(h->dX0, d_x0, (size_t)h->batch * h->n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return ALMPC_OK;
}

int almpc_calculate_async(almpc_handle* h, const almpc_opts* user) { return calculate_checked(h, user, StepMode()); }

int almpc_synchronize(almpc_handle* h) {
    if (!h) return ALMPC_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    // A step is tens of microseconds: the wait polls the stream for a while before falling back to the blocking wait, whose wake-up
    // (interrupt + scheduler) was seen to cost up to ~15 ms on this pool -- 200 steps' worth (stream_wait_polling).
    return wait_and_settle(h);
}

int almpc_calculate(almpc_handle* h, const almpc_opts* opts) {
    int rc = almpc_calculate_async(h, opts);
    if (rc != ALMPC_OK) return rc;
    return almpc_synchronize(h);
}

int almpc_get_results(almpc_handle* h, double* x, double* e_x, double* u, double* e_u, int32_t* status,
                      int32_t* iters, int32_t* polish_iters) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, "get_results before design");
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(wait_and_settle(h, true));
    const size_t b = (size_t)h->batch, xs = (size_t)h->n * (h->N + 1), us = (size_t)h->nz;
    if (x) HIP_TRY(h, hipMemcpy(x, h->dX, b * xs * sizeof(double), hipMemcpyDeviceToHost));
    if (e_x) HIP_TRY(h, hipMemcpy(e_x, h->dEx, b * xs * sizeof(double), hipMemcpyDeviceToHost));
    if (u) HIP_TRY(h, hipMemcpy(u, h->dU, b * us * sizeof(double), hipMemcpyDeviceToHost));
    if (e_u) HIP_TRY(h, hipMemcpy(e_u, h->dEu, b * us * sizeof(double), hipMemcpyDeviceToHost));
    if (status) HIP_TRY(h, hipMemcpy(status, h->dStatus, b * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (iters) HIP_TRY(h, hipMemcpy(iters, h->dIters, b * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (polish_iters) HIP_TRY(h, hipMemcpy(polish_iters, h->dPiters, b * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

int almpc_get_design(almpc_handle* h, double* H, double* F, double* P, double* d) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, "get_design before design");
    if (H) std::memcpy(H, h->H.data(), h->H.size() * sizeof(double));
    if (F) std::memcpy(F, h->F.data(), h->F.size() * sizeof(double));
    if (P) std::memcpy(P, h->P.data(), h->P.size() * sizeof(double));
    if (d && h->d.size() >= (size_t)h->nz) std::memcpy(d, h->d.data(), (size_t)h->nz * sizeof(double));   // (structured handles: P only)
    return ALMPC_OK;
}

int almpc_device_results(almpc_handle* h, const double** d_x, const double** d_e_x, const double** d_u,
                         const double** d_e_u) {
    if (!h) return ALMPC_ERR_INVALID;
    if (d_x) *d_x = h->dX;
    if (d_e_x) *d_e_x = h->dEx;
    if (d_u) *d_u = h->dU;
    if (d_e_u) *d_e_u = h->dEu;
    return ALMPC_OK;
}

int almpc_timing_set_stride(almpc_handle* h, int every) {
    if (!h || every < 1) return ALMPC_ERR_INVALID;
    h->timing_stride = every;
    h->step_count = 0;
    return ALMPC_OK;
}

int almpc_timing_reset(almpc_handle* h, int reserve_steps) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!(h->flags & ALMPC_FLAG_TIMING)) return fail(h, ALMPC_ERR_INVALID, "handle was created without ALMPC_FLAG_TIMING");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->ev_used = 0;
    h->step_count = 0;
    const size_t need = 4 * (size_t)(reserve_steps > 0 ? reserve_steps : 0);
    if (h->ev.size() < need) {
        const size_t old = h->ev.size();
        h->ev.resize(need, nullptr);
        for (size_t i = old; i < need; ++i) HIP_TRY(h, hipEventCreate(&h->ev[i]));
    }
    return ALMPC_OK;
}

int almpc_timing_summary(almpc_handle* h, int* steps, double* ms_admm, double* ms_polish, double* ms_rollout,
                         double* ms_total) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!(h->flags & ALMPC_FLAG_TIMING)) return fail(h, ALMPC_ERR_INVALID, "handle was created without ALMPC_FLAG_TIMING");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double a = 0, p = 0, r = 0, t = 0;
    for (size_t sidx = 0; sidx < h->ev_used; ++sidx) {
        hipEvent_t* ev = &h->ev[4 * sidx];
        float f = 0;
        if (h->ev_two[sidx]) {   // one-kernel step: the pair around the kernel is all there is
            HIP_TRY(h, hipEventElapsedTime(&f, ev[1], ev[2])); p += f; t += f;
            continue;
        }
        HIP_TRY(h, hipEventElapsedTime(&f, ev[0], ev[1])); a += f;
        HIP_TRY(h, hipEventElapsedTime(&f, ev[1], ev[2])); p += f;
        HIP_TRY(h, hipEventElapsedTime(&f, ev[2], ev[3])); r += f;
        HIP_TRY(h, hipEventElapsedTime(&f, ev[0], ev[3])); t += f;
    }
    if (steps) *steps = (int)h->ev_used;
    if (ms_admm) *ms_admm = a;
    if (ms_polish) *ms_polish = p;
    if (ms_rollout) *ms_rollout = r;
    if (ms_total) *ms_total = t;
    return ALMPC_OK;
}

int almpc_timing_samples(almpc_handle* h, int cap, int* count, float* ms_admm, float* ms_polish, float* ms_rollout, float* ms_total) {
    if (!h || cap < 0) return ALMPC_ERR_INVALID;
    if (!(h->flags & ALMPC_FLAG_TIMING)) return fail(h, ALMPC_ERR_INVALID, "handle was created without ALMPC_FLAG_TIMING");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t nrec = std::min((size_t)cap, h->ev_used);
    for (size_t sidx = 0; sidx < nrec; ++sidx) {
        hipEvent_t* ev = &h->ev[4 * sidx];
        float f = 0;
        if (h->ev_two[sidx]) {
            HIP_TRY(h, hipEventElapsedTime(&f, ev[1], ev[2]));
            if (ms_admm) ms_admm[sidx] = 0; if (ms_polish) ms_polish[sidx] = f; if (ms_rollout) ms_rollout[sidx] = 0; if (ms_total) ms_total[sidx] = f;
            continue;
        }
        HIP_TRY(h, hipEventElapsedTime(&f, ev[0], ev[1])); if (ms_admm) ms_admm[sidx] = f;
        HIP_TRY(h, hipEventElapsedTime(&f, ev[1], ev[2])); if (ms_polish) ms_polish[sidx] = f;
        HIP_TRY(h, hipEventElapsedTime(&f, ev[2], ev[3])); if (ms_rollout) ms_rollout[sidx] = f;
        HIP_TRY(h, hipEventElapsedTime(&f, ev[0], ev[3])); if (ms_total) ms_total[sidx] = f;
    }
    if (count) *count = (int)h->ev_used;
    return ALMPC_OK;
}

int almpc_get_timing(almpc_handle* h, float* ms_admm, float* ms_polish, float* ms_rollout, float* ms_total) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!(h->flags & ALMPC_FLAG_TIMING) || h->ev_used == 0) return fail(h, ALMPC_ERR_INVALID, "timing not enabled or no step timed yet");
    HIP_TRY(h, hipSetDevice(h->device));
    hipEvent_t* ev = &h->ev[4 * (h->ev_used - 1)];
    float a = 0, p = 0, r = 0, t = 0;
    if (h->ev_two[h->ev_used - 1]) {
        HIP_TRY(h, hipEventSynchronize(ev[2]));
        HIP_TRY(h, hipEventElapsedTime(&p, ev[1], ev[2]));
        t = p;
    } else {
    HIP_TRY(h, hipEventSynchronize(ev[3]));
    HIP_TRY(h, hipEventElapsedTime(&a, ev[0], ev[1]));
    HIP_TRY(h, hipEventElapsedTime(&p, ev[1], ev[2]));
    HIP_TRY(h, hipEventElapsedTime(&r, ev[2], ev[3]));
    HIP_TRY(h, hipEventElapsedTime(&t, ev[0], ev[3]));
    }
    if (ms_admm) *ms_admm = a;
    if (ms_polish) *ms_polish = p;
    if (ms_rollout) *ms_rollout = r;
    if (ms_total) *ms_total = t;
    return ALMPC_OK;
}

int almpc_dare(int n, int m, const double* A, const double* B, const double* Q, const double* R, double* P) {
    if (n < 1 || m < 1 || !A || !B || !Q || !R || !P) return ALMPC_ERR_INVALID;
    hm::mat Am(A, A + (size_t)n * n), Bm(B, B + (size_t)n * m), Qm(Q, Q + (size_t)n * n), Rm(R, R + (size_t)m * m), Pm;
    if (!hm::dare(Am, Bm, Qm, Rm, n, m, Pm)) return ALMPC_ERR_NUMERIC;
    std::memcpy(P, Pm.data(), (size_t)n * n * sizeof(double));
    return ALMPC_OK;
}

int almpc_dare_vjp(int n, int m, const double* A, const double* B, const double* Q, const double* R, const double* P, const double* g_P,
                   double* g_A, double* g_B, double* g_Q, double* g_R) {
    if (n < 1 || m < 1 || !A || !B || !Q || !R || !P || !g_P) return ALMPC_ERR_INVALID;
    const size_t nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
    hm::mat gA, gB, gQ, gR;
    const int st = hm::dare_vjp(hm::mat(A, A + nn), hm::mat(B, B + nm), hm::mat(Q, Q + nn), hm::mat(R, R + mm), hm::mat(P, P + nn),
                                hm::mat(g_P, g_P + nn), n, m, g_A ? &gA : nullptr, g_B ? &gB : nullptr, g_Q ? &gQ : nullptr, g_R ? &gR : nullptr);
    if (st != 0) {
        static const char* const why[] = {"", "R + B'PB is singular", "the closed loop A - B K is not stable: P is not the stabilising solution",
                                          "P does not solve the equation for this model"};
        g_nohandle_err = "dare_vjp: status " + std::to_string(st) + " (" + why[st] + ")";
        return ALMPC_ERR_NUMERIC;
    }
    if (g_A) std::copy(gA.begin(), gA.end(), g_A);
    if (g_B) std::copy(gB.begin(), gB.end(), g_B);
    if (g_Q) std::copy(gQ.begin(), gQ.end(), g_Q);
    if (g_R) std::copy(gR.begin(), gR.end(), g_R);
    return ALMPC_OK;
}

int almpc_c2d(int n, int m, const double* Ac, const double* Bc, double Ts, double* Ad, double* Bd) {
    if (n < 1 || m < 1 || !Ac || !Bc || !Ad || !Bd) return ALMPC_ERR_INVALID;
    if (!(Ts > 0.0 && std::isfinite(Ts))) return ALMPC_ERR_INVALID;
    hm::mat Am, Bm;
    if (hm::c2d(hm::mat(Ac, Ac + (size_t)n * n), hm::mat(Bc, Bc + (size_t)n * m), Ts, n, m, Am, Bm) != 0) return ALMPC_ERR_NUMERIC;
    std::copy(Am.begin(), Am.end(), Ad);
    std::copy(Bm.begin(), Bm.end(), Bd);
    return ALMPC_OK;
}

int almpc_c2d_batched(int device_id, int n, int m, int batch, const double* Ac_batch, const double* Bc_batch, double Ts,
                      double* Ad_batch, double* Bd_batch, int32_t* status) {
    if (n < 1 || m < 1 || batch < 1 || !Ac_batch || !Bc_batch || !Ad_batch || !Bd_batch || !status) return ALMPC_ERR_INVALID;
    if (!(Ts > 0.0 && std::isfinite(Ts))) return ALMPC_ERR_INVALID;
    if (n > C2D_MAX_N || m > C2D_MAX_M) return ALMPC_ERR_UNSUPPORTED;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count) return ALMPC_ERR_NO_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return ALMPC_ERR_HIP;
    using Tight = DevBuf<double, Mem::DeviceTight>;
    const size_t b = (size_t)batch, nn = (size_t)n * n, nm = (size_t)n * m;
    Tight dAc, dBc, dAd, dBd;
    DevBuf<int32_t, Mem::DeviceTight> dSt;
    // (Ad_batch, Bd_batch go up as well: the slots of an instance that fails come back as the caller left them)
    if (dAc.upload(Ac_batch, b * nn) != hipSuccess || dBc.upload(Bc_batch, b * nm) != hipSuccess || dAd.upload(Ad_batch, b * nn) != hipSuccess ||
        dBd.upload(Bd_batch, b * nm) != hipSuccess || dSt.alloc(b) != hipSuccess)
        return ALMPC_ERR_HIP;
    C2dParams cp;
    cp.n = n; cp.m = m; cp.batch = batch;
    cp.Ac = dAc; cp.A_stride = (long)nn; cp.Bc = dBc; cp.B_stride = (long)nm; cp.Ts = Ts;
    cp.Ad = dAd; cp.Bd = dBd; cp.poison = 0; cp.status = dSt; cp.lds_per_wave = 0;
    if (launch_c2d(cp, 0) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ALMPC_ERR_HIP;
    if (hipMemcpy(Ad_batch, dAd, b * nn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(Bd_batch, dBd, b * nm * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(status, dSt, b * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return ALMPC_ERR_HIP;
    return ALMPC_OK;
}

int almpc_dare_batched(int device_id, int n, int m, int batch, const double* A_batch, const double* B_batch, const double* Q,
                       const double* R, double* P_batch, int32_t* status) {
    if (n < 1 || m < 1 || batch < 1 || !A_batch || !B_batch || !Q || !R || !P_batch || !status) return ALMPC_ERR_INVALID;
    if (n > DARE_MAX_N || m > DARE_MAX_M) return ALMPC_ERR_UNSUPPORTED;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count) return ALMPC_ERR_NO_DEVICE;
    {
        const char* why = "";
        ALMPC_TRY(dare_device_check(n, m, hm::mat(R, R + (size_t)m * m), false, &why));
    }
    if (hipSetDevice(device_id) != hipSuccess) return ALMPC_ERR_HIP;
    using Tight = DevBuf<double, Mem::DeviceTight>;
    const size_t b = (size_t)batch, nn = (size_t)n * n, nm = (size_t)n * m;
    Tight dA, dB, dQ, dR, dP;
    DevBuf<int32_t, Mem::DeviceTight> dSt;
    // (P_batch goes up as well: the slot of an instance without a solution comes back as the caller left it)
    if (dA.upload(A_batch, b * nn) != hipSuccess || dB.upload(B_batch, b * nm) != hipSuccess || dQ.upload(Q, nn) != hipSuccess ||
        dR.upload(R, (size_t)m * m) != hipSuccess || dP.upload(P_batch, b * nn) != hipSuccess || dSt.alloc(b) != hipSuccess)
        return ALMPC_ERR_HIP;
    DareParams dp;
    dp.n = n; dp.m = m; dp.batch = batch;
    dp.A = dA; dp.A_stride = (long)nn; dp.B = dB; dp.B_stride = (long)nm; dp.Q = dQ; dp.R = dR;
    dp.P = dP; dp.P_stride = (long)nn; dp.fallback = nullptr; dp.status = dSt; dp.lds_per_wave = 0;
    if (launch_dare(dp, 0) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ALMPC_ERR_HIP;
    if (hipMemcpy(P_batch, dP, b * nn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(status, dSt, b * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return ALMPC_ERR_HIP;
    return ALMPC_OK;
}

int almpc_dare_vjp_batched(int device_id, int n, int m, int batch, const double* A_batch, const double* B_batch, const double* Q,
                           const double* R, const double* P_batch, const double* gP_batch, double* gA_batch, double* gB_batch,
                           double* gQ_batch, double* gR_batch, int32_t* status) {
    if (n < 1 || m < 1 || batch < 1 || !A_batch || !B_batch || !Q || !R || !P_batch || !gP_batch || !status) return ALMPC_ERR_INVALID;
    if (n > DARE_MAX_N || m > DARE_MAX_M) return ALMPC_ERR_UNSUPPORTED;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count) return ALMPC_ERR_NO_DEVICE;
    {
        const char* why = "";
        ALMPC_TRY(dare_device_check(n, m, hm::mat(R, R + (size_t)m * m), false, &why));
    }
    if (hipSetDevice(device_id) != hipSuccess) return ALMPC_ERR_HIP;
    using Tight = DevBuf<double, Mem::DeviceTight>;
    const size_t b = (size_t)batch, nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
    Tight dA, dB, dQ, dR, dP, dgP, dgA, dgB, dgQ, dgR;
    DevBuf<int32_t, Mem::DeviceTight> dSt;
    // (the outputs go up as well: the slots of an instance that is refused come back as the caller left them)
    const auto up = [](Tight& dst, const double* src, size_t cnt) { return src ? dst.upload(src, cnt) : hipSuccess; };
    if (up(dA, A_batch, b * nn) != hipSuccess || up(dB, B_batch, b * nm) != hipSuccess || up(dQ, Q, nn) != hipSuccess ||
        up(dR, R, mm) != hipSuccess || up(dP, P_batch, b * nn) != hipSuccess || up(dgP, gP_batch, b * nn) != hipSuccess ||
        up(dgA, gA_batch, b * nn) != hipSuccess || up(dgB, gB_batch, b * nm) != hipSuccess || up(dgQ, gQ_batch, b * nn) != hipSuccess ||
        up(dgR, gR_batch, b * mm) != hipSuccess || dSt.alloc(b) != hipSuccess)
        return ALMPC_ERR_HIP;
    DareVjpParams vp;
    vp.n = n; vp.m = m; vp.batch = batch;
    vp.A = dA; vp.A_stride = (long)nn; vp.B = dB; vp.B_stride = (long)nm; vp.P = dP; vp.P_stride = (long)nn; vp.gP = dgP; vp.gP_stride = (long)nn;
    vp.Q = dQ; vp.R = dR;
    vp.gA = gA_batch ? dgA.get() : nullptr; vp.gA_stride = (long)nn; vp.gB = gB_batch ? dgB.get() : nullptr; vp.gB_stride = (long)nm;
    vp.gQ = gQ_batch ? dgQ.get() : nullptr; vp.gQ_stride = (long)nn; vp.gR = gR_batch ? dgR.get() : nullptr; vp.gR_stride = (long)mm;
    vp.accumulate = 0; vp.rows = nullptr; vp.status = dSt; vp.lds_per_wave = 0;
    if (launch_dare_vjp(vp, 0) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ALMPC_ERR_HIP;
    const auto down = [](double* dst, const Tight& src, size_t cnt) {
        return dst ? hipMemcpy(dst, src, cnt * sizeof(double), hipMemcpyDeviceToHost) : hipSuccess;
    };
    if (down(gA_batch, dgA, b * nn) != hipSuccess || down(gB_batch, dgB, b * nm) != hipSuccess || down(gQ_batch, dgQ, b * nn) != hipSuccess ||
        down(gR_batch, dgR, b * mm) != hipSuccess || hipMemcpy(status, dSt, b * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return ALMPC_ERR_HIP;
    return ALMPC_OK;
}

// (dense: almpc_densenet_linearize, activation a bare code; else almpc_fnn_linearize, activation an ALMPC_NET_CODE)
static int net_linearize(bool dense, int device_id, int n, int m, int H, int L, int activation, const double* W_in, const double* W_h,
                         const double* b_h, const double* W_out, int batch, const double* x, const double* u, double* A,
                         double* B, double* f) {
    const Switches sw = read_switches();   // (no handle: the switches of this call)
    if (n < 1 || m < 1 || H < 1 || L < 0 || batch < 1 || !W_in || !W_out || !x || !u || !A || !B || (L > 0 && (!W_h || !b_h)))
        return ALMPC_ERR_INVALID;
    int net = NET_FNN;
    if (!setup_net(dense, activation, &net, &activation)) return ALMPC_ERR_UNSUPPORTED;
    const size_t nin = (size_t)n + m;
    if (fnn_wave_scratch_doubles(n, m, H, L, net) * sizeof(double) > 160 * 1024) return ALMPC_ERR_UNSUPPORTED;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count) return ALMPC_ERR_NO_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return ALMPC_ERR_HIP;
    using Tight = DevBuf<double, Mem::DeviceTight>;
    Tight dWin, dWh, dbh, dWout, dx, du, dA, dB, df;
    auto up = [](Tight& d, const double* src, size_t cnt) -> double* { return d.upload(src, cnt) == hipSuccess ? d.get() : nullptr; };
    FnnParams p;
    p.n = n; p.m = m; p.H = H; p.L = L; p.act = activation; p.batch = batch;
    p.ppi = 1; p.xs_group = n; p.us_group = m;
    p.W_in = up(dWin, W_in, (size_t)H * nin); p.W_h = up(dWh, W_h, net_wh_doubles(net, H, L)); p.b_h = up(dbh, b_h, (size_t)L * H);
    p.W_out = up(dWout, W_out, net_wout_doubles(net, n, H, L)); p.x = up(dx, x, (size_t)batch * n); p.u = up(du, u, (size_t)batch * m);
    p.A = up(dA, nullptr, (size_t)batch * n * n); p.B = up(dB, nullptr, (size_t)batch * n * m); p.f = f ? up(df, nullptr, (size_t)batch * n) : nullptr;
    int rc = ALMPC_OK;
    if (!p.W_in || !p.W_h || !p.b_h || !p.W_out || !p.x || !p.u || !p.A || !p.B || (f && !p.f)) rc = ALMPC_ERR_HIP;
    if (rc == ALMPC_OK) {
        hipDeviceProp_t prop;
        const int cus = hipGetDeviceProperties(&prop, device_id) == hipSuccess ? prop.multiProcessorCount : 256;
        if (launch_fnn_jacobian(sw, p, net, cus, 0) != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = ALMPC_ERR_HIP;
    }
    if (rc == ALMPC_OK) {
        if (hipMemcpy(A, p.A, (size_t)batch * n * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(B, p.B, (size_t)batch * n * m * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            (f && hipMemcpy(f, p.f, (size_t)batch * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
            rc = ALMPC_ERR_HIP;
    }
    return rc;
}
int almpc_fnn_linearize(int device_id, int n, int m, int H, int L, int activation, const double* W_in, const double* W_h,
                        const double* b_h, const double* W_out, int batch, const double* x, const double* u, double* A,
                        double* B, double* f) {
    return net_linearize(false, device_id, n, m, H, L, activation, W_in, W_h, b_h, W_out, batch, x, u, A, B, f);
}
int almpc_densenet_linearize(int device_id, int n, int m, int H, int L, int activation, const double* W_in, const double* W_h,
                             const double* b_h, const double* W_out, int batch, const double* x, const double* u, double* A,
                             double* B, double* f) {
    return net_linearize(true, device_id, n, m, H, L, activation, W_in, W_h, b_h, W_out, batch, x, u, A, B, f);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Multi-GPU: RCCL inside the library (see almpc_comm.hip.h and include/almpc.h)
int almpc_comm_unique_id(char* id128) {
    if (!id128) return ALMPC_ERR_INVALID;
    RcclApi& r = rccl_api();
    if (!r.ok) return ALMPC_ERR_UNSUPPORTED;
    ncclUniqueId id;
    if (r.GetUniqueId(&id) != ncclSuccess) return ALMPC_ERR_HIP;
    std::memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
    return ALMPC_OK;
}

int almpc_comm_init(almpc_handle* h, const char* id128, int rank, int world) {
    if (!h || !id128) return ALMPC_ERR_INVALID;
    if (world < 1 || rank < 0 || rank >= world) return fail(h, ALMPC_ERR_INVALID, "comm_init: need 0 <= rank < world");
    RcclApi& r = rccl_api();
    if (!r.ok) return fail(h, ALMPC_ERR_UNSUPPORTED, "comm_init: " + r.err);
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->comm) { (void)r.CommDestroy(h->comm); h->comm = nullptr; }
    ncclUniqueId id;
    std::memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    const ncclResult_t rc = r.CommInitRank(&h->comm, world, id, rank);
    if (rc != ncclSuccess) { h->comm = nullptr; return fail(h, ALMPC_ERR_HIP, std::string("ncclCommInitRank: ") + r.GetErrorString(rc)); }
    h->comm_rank = rank; h->comm_world = world;
    h->dU0.reset(); h->dU0all.reset();
    HIP_TRY(h, h->dComm4.once(4));
    HIP_TRY(h, h->dU0.alloc((size_t)h->batch * h->m));
    HIP_TRY(h, h->dU0all.alloc((size_t)world * h->batch * h->m));
    return ALMPC_OK;
}

int almpc_comm_summary(almpc_handle* h, int64_t* out4) {
    if (!h || !out4) return ALMPC_ERR_INVALID;
    if (!h->comm) return fail(h, ALMPC_ERR_NOT_DESIGNED, "comm_summary before comm_init");
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, "comm_summary before a step");
    RcclApi& r = rccl_api();
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_comm_summary, dim3(1), dim3(1024), 0, h->stream, h->batch, h->dStatus, h->dIters, h->dPiters, h->dComm4);
    HIP_TRY(h, hipGetLastError());
    ncclResult_t rc = r.AllReduce(h->dComm4, h->dComm4, 2, ncclInt64, ncclSum, h->comm, h->stream);
    if (rc == ncclSuccess) rc = r.AllReduce(h->dComm4 + 2, h->dComm4 + 2, 2, ncclInt64, ncclMax, h->comm, h->stream);
    if (rc != ncclSuccess) return fail(h, ALMPC_ERR_HIP, std::string("ncclAllReduce: ") + r.GetErrorString(rc));
    long long host[4];
    HIP_TRY(h, hipMemcpyAsync(host, h->dComm4, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 4; ++i) out4[i] = host[i];
    return ALMPC_OK;
}

int almpc_comm_allgather_first_input(almpc_handle* h, double* u0_all, const double** d_u0_all) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->comm) return fail(h, ALMPC_ERR_NOT_DESIGNED, "comm_allgather_first_input before comm_init");
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, "comm_allgather_first_input before a step");
    RcclApi& r = rccl_api();
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t cnt = (size_t)h->batch * h->m;
    hipLaunchKernelGGL(k_pack_first_input, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, h->batch, h->m, h->N, h->dU, h->dU0);
    HIP_TRY(h, hipGetLastError());
    const ncclResult_t rc = r.AllGather(h->dU0, h->dU0all, cnt, ncclFloat64, h->comm, h->stream);
    if (rc != ncclSuccess) return fail(h, ALMPC_ERR_HIP, std::string("ncclAllGather: ") + r.GetErrorString(rc));
    if (u0_all) {
        HIP_TRY(h, hipMemcpyAsync(u0_all, h->dU0all, cnt * h->comm_world * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (d_u0_all) *d_u0_all = h->dU0all;
    return ALMPC_OK;
}

int almpc_advance_plant(almpc_handle* h) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, "advance_plant before design");
    if (h->batched) return fail(h, ALMPC_ERR_UNSUPPORTED, "advance_plant: per-instance models have no shared plant (advance the states on the caller's side)");
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(enqueue_gated_redo(h));   // the plant must not be driven by an undecided instance's iterate
    const int per_block = 256 / h->n;
    const double* x0_in = h->dX0;
    const int x0_slot = h->io.x0_slot;
    io_release_x0(h);   // (a pinned x0 slot is read once more here; the new states go to the handle's own device buffer)
    hipLaunchKernelGGL(k_advance_plant, dim3((h->batch + per_block - 1) / per_block), dim3(256), (size_t)per_block * h->n * sizeof(double),
                       h->stream, h->n, h->m, h->N, h->batch, h->dA, h->dB, h->dU, x0_in, h->dX0);
    HIP_TRY(h, hipGetLastError());
    if (x0_slot >= 0) {   // the slot is free for the host again only once THIS read has finished too
        HIP_TRY(h, hipEventRecord(h->io.ev_used[x0_slot], h->stream));
        h->io.used_pending[x0_slot] = true;
    }
    return ALMPC_OK;
}

int almpc_debug_poison_lds(almpc_handle* h) {
    if (!h) return ALMPC_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    const int bytes = 160 * 1024;
    HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_poison_lds), (size_t)(bytes)));
    // one workgroup owns a whole CU's LDS; several waves of workgroups so that every CU is visited
    hipLaunchKernelGGL(k_poison_lds, dim3(1024), dim3(1024), bytes, h->stream, 0x7ff8dead0000beefULL, bytes / 8,
                       reinterpret_cast<unsigned long long*>(h->dSglobal.get()));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return ALMPC_OK;
}
}  // extern "C"

// ---- solution sensitivities (k_sens) --------------------------------------------------------------------------------------------
namespace {

// What a sensitivity call can look at: the last step of a condensed design with an input box only; the rows form
// (almpc_sensitivity_rows, rows_form) also that of a shared design with state rows.
int sens_check(almpc_handle* h, const char* who, bool rows_form = false) {
    if (!h) return ALMPC_ERR_INVALID;
    const std::string w(who);
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, w + " before design");
    if (h->structured) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": a structured handle forms no condensed inverse G = H'^-1 (the constraint-space form is not built)");
    if (h->ltv || h->sqp.ready) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": time-varying and SQP designs solve for a step around a trajectory, not for u(x0) (an almpc_design_ltv design, in its initial deviation: almpc_sensitivity_ltv)");
    if (h->relin.ready) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the re-linearisation pipeline's models depend on x0 themselves");
    if (h->mc > 0 && !rows_form)
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": designs with state rows (state box, terminal equality) need the constraint-space form (almpc_sensitivity_rows)");
    if (h->mc > 0 && (h->batched || h->ghat_inst))
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": per-instance models with state rows keep one constraint-space matrix per instance, for which the rows form is not built");
    if (!h->sens.stepped) return fail(h, ALMPC_ERR_INVALID, w + ": no step has run on this design");
    return ALMPC_OK;
}

// Operands every k_sens launch shares; the plain V of a shared design is unpacked once per design.
// rows (a shared design with state rows, sens_check passed in the rows form): the operands are Ghat and the table T1, made at the
// first such call on a design
int sens_params(almpc_handle* h, double act_tol, SensParams& p, bool rows = false, double act_tol_x = 0.0) {
    const int n = h->n, nz = h->nz, nzs = h->nzs;
    p = SensParams();
    p.n = n; p.m = h->m; p.N = h->N; p.nz = nz; p.nzs = nzs; p.batch = h->batch;
    p.cap2 = nz;
    if (h->batched) {
        p.G = h->bG; p.G_stride = (long)nz * nzs; p.V = h->bVs; p.V_stride = (long)n * nzs; p.d = h->bD; p.d_stride = nzs;
        p.A = h->bA; p.A_stride = (long)n * n; p.B = h->bB; p.B_stride = (long)n * h->m;
    } else {
        if (!h->sens.v_ok) {
            HIP_TRY(h, h->sens.V.grow((size_t)n * nzs));
            hipLaunchKernelGGL(k_sens_unpack_v, dim3(32), dim3(256), 0, h->stream, h->dVFrag.get(), nz, n, nzs, h->ksf, h->sens.V.get());
            HIP_TRY(h, hipGetLastError());
            h->sens.v_ok = true;
        }
        p.G = h->dG; p.V = h->sens.V; p.d = h->dD; p.A = h->dA; p.B = h->dB;
    }
    if (rows) {
        const int ne = h->eq_proj ? n : 0, eq0 = h->R - n;
        if (!h->sens.t1_ok) {
            HIP_TRY(h, h->sens.T1.grow((size_t)n * h->Rs));
            SensRowsTableParams tp;
            tp.n = n; tp.m = h->m; tp.N = h->N; tp.nz = nz; tp.nzs = nzs; tp.R = h->R; tp.Rs = h->Rs; tp.eq_proj = h->eq_proj; tp.eq0 = eq0; tp.ne = ne;
            tp.A = h->dA; tp.B = h->dB; tp.V = h->sens.V; tp.d = h->dD; tp.row_xidx = h->dRowXidx;
            // the design's H and F for the table's refinement of V (the stream is idle: wait_and_settle has run)
            if (h->H.size() != (size_t)nz * nz || h->F.size() != (size_t)nz * n) return fail(h, ALMPC_ERR_INVALID, "sensitivity_rows: the design's H and F are not kept");
            HIP_TRY(h, h->sens.HF.grow((size_t)nz * nz + (size_t)nz * n));
            HIP_TRY(h, hipMemcpy(h->sens.HF, h->H.data(), (size_t)nz * nz * sizeof(double), hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(h->sens.HF + (size_t)nz * nz, h->F.data(), (size_t)nz * n * sizeof(double), hipMemcpyHostToDevice));
            tp.H = h->sens.HF; tp.F = h->sens.HF + (size_t)nz * nz; tp.G = h->dG;
            tp.GhatE = h->eq_proj ? h->dGhatE.get() : nullptr; tp.WinvE = h->eq_proj ? h->dWinvE.get() : nullptr; tp.out = h->sens.T1;
            // (dynamic LDS far below the 64 KB that need no opt-in: (N + 1) n <= 1024 and nz <= 512 by the design's limits on state rows)
            hipLaunchKernelGGL(k_sens_rows_table, dim3((unsigned)n), dim3(256), (size_t)sens_rows_table_lds_doubles(n, h->N, nz) * sizeof(double), h->stream, tp);
            HIP_TRY(h, hipGetLastError());
            h->sens.t1_ok = true;
        }
        p.G = h->dGhat; p.V = h->sens.T1;
        p.R = h->R; p.Rs = h->Rs; p.cap2 = nz - ne; p.eq_proj = h->eq_proj; p.eq0 = eq0; p.ne = ne;
        p.x = h->dX; p.xmin = h->dXmin; p.xmax = h->dXmax; p.row_xidx = h->dRowXidx; p.row_eq = h->dRowEq;
        p.tau_x = act_tol_x > 0.0 ? act_tol_x : 1e-7;
    }
    p.umin = h->dUmin; p.umax = h->dUmax; p.u = h->dU; p.status = h->dStatus;
    p.tau = act_tol > 0.0 ? act_tol : 1e-9;
    p.ch = sens_ch(n);
    HIP_TRY(h, h->sens.ovf.grow((size_t)SENS_OVF_HEAD + h->batch));
    p.ovf = h->sens.ovf;
    return ALMPC_OK;
}

// The two tiers, back to back on the handle's stream: no host look in between (the second is gated on the list's count word)
// (ROWS: p.cap2 rows at most in an independent working set, one flag per row of A)
template <bool VJP, bool ROWS>
int sens_launch(almpc_handle* h, SensParams p) {
    const int n = h->n, nzs = h->nzs, cap2 = p.cap2, nfl = ROWS ? h->Rs : nzs;
    const size_t lds2 = cap2 > SENS_CAP1 ? (size_t)sens_lds_doubles(n, nzs, cap2, nfl) * sizeof(double) : 0;
    if (lds2 > 160 * 1024) return fail(h, ALMPC_ERR_UNSUPPORTED, "sensitivity: the second tier's working set does not fit LDS");
    HIP_TRY(h, hipMemsetAsync(h->sens.ovf, 0, SENS_OVF_HEAD * sizeof(int32_t), h->stream));
    p.cap = SENS_CAP1; p.lds_per_team = sens_lds_doubles(n, nzs, p.cap, nfl);
    const size_t lds1 = (size_t)SENS_WAVES * p.lds_per_team * sizeof(double);
    HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_sens<VJP, false, ROWS>), lds1));
    hipLaunchKernelGGL((k_sens<VJP, false, ROWS>), dim3((unsigned)((h->batch + SENS_WAVES - 1) / SENS_WAVES)), dim3(64 * SENS_WAVES), lds1, h->stream, p);
    HIP_TRY(h, hipGetLastError());
    if (cap2 > SENS_CAP1) {   // (a working set cannot outgrow the first tier otherwise)
        p.cap = cap2; p.lds_per_team = sens_lds_doubles(n, nzs, p.cap, nfl);
        HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_sens<VJP, true, ROWS>), lds2));
        hipLaunchKernelGGL((k_sens<VJP, true, ROWS>), dim3((unsigned)std::min(h->batch, 4 * h->num_cus)), dim3(SENS_WG), lds2, h->stream, p);
        HIP_TRY(h, hipGetLastError());
    }
    return ALMPC_OK;
}

// The LDS-fit test of the second tier on its own, in front of everything a call enqueues (the design-time tables included)
int sens_fits(almpc_handle* h, bool rows) {
    const int cap2 = h->nz - ((rows && h->eq_proj) ? h->n : 0);
    if (cap2 > SENS_CAP1 && (size_t)sens_lds_doubles(h->n, h->nzs, cap2, rows ? h->Rs : h->nzs) * sizeof(double) > 160 * 1024)
        return fail(h, ALMPC_ERR_UNSUPPORTED, "sensitivity: the second tier's working set does not fit LDS");
    return ALMPC_OK;
}

// almpc_sensitivity (rows_form false) and almpc_sensitivity_rows: a design without state rows takes the same path through both
int sens_jacobians(almpc_handle* h, const char* who, bool rows_form, uint32_t want, double act_tol, double act_tol_x) {
    ALMPC_TRY(sens_check(h, who, rows_form));
    if (!want || (want & ~(ALMPC_SENS_K0 | ALMPC_SENS_DU | ALMPC_SENS_DX))) return fail(h, ALMPC_ERR_INVALID, std::string(who) + ": want must be a mask of ALMPC_SENS_*");
    const bool rows = rows_form && h->mc > 0;
    if (rows) ALMPC_TRY(sens_fits(h, true));
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(wait_and_settle(h));   // (a synchronous look: redone instances take part)
    const size_t b = (size_t)h->batch, n = (size_t)h->n;
    h->sens.have = 0;
    SensParams p;
    ALMPC_TRY(sens_params(h, act_tol, p, rows, act_tol_x));
    HIP_TRY(h, h->sens.rows.grow(b));
    if (want & ALMPC_SENS_K0) HIP_TRY(h, h->sens.K0.grow(b * n * h->m));
    if (want & (ALMPC_SENS_DU | ALMPC_SENS_DX)) HIP_TRY(h, h->sens.dU.grow(b * n * h->nz));   // (dX is rolled out from dU)
    if (want & ALMPC_SENS_DX) HIP_TRY(h, h->sens.dX.grow(b * n * (h->N + 1) * n));
    p.want = want; p.K0 = h->sens.K0; p.dU = h->sens.dU; p.rows = h->sens.rows;
    if (rows) ALMPC_TRY((sens_launch<false, true>(h, p)));
    else ALMPC_TRY((sens_launch<false, false>(h, p)));
    if (want & ALMPC_SENS_DX) {
        SensDxParams q;
        q.n = h->n; q.m = h->m; q.N = h->N; q.nz = h->nz; q.batch = h->batch;
        q.A = p.A; q.A_stride = p.A_stride; q.B = p.B; q.B_stride = p.B_stride; q.dU = h->sens.dU; q.rows = h->sens.rows; q.dX = h->sens.dX;
        const size_t lds = (size_t)sens_dx_lds_doubles(h->n, h->m) * sizeof(double);
        HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_sens_dx), lds));
        hipLaunchKernelGGL(k_sens_dx, dim3((unsigned)std::min(h->batch, 16 * h->num_cus)), dim3(256), lds, h->stream, q);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, stream_wait_polling(h));
    h->sens.have = want | ((want & ALMPC_SENS_DX) ? ALMPC_SENS_DU : 0u);
    return ALMPC_OK;
}

// What every VJP is staged with: the loss gradients uploaded (g_x may be null), the result and its |W| words grown, and the four
// pointers of the kernel's parameters (SensParams, SensFaceParams) set
template <class Params>
int sens_vjp_stage(almpc_handle* h, const double* g_u, const double* g_x, Params& p) {
    const size_t b = (size_t)h->batch, n = (size_t)h->n, xs = n * (h->N + 1);
    HIP_TRY(h, h->sens.vrows.grow(b)); HIP_TRY(h, h->sens.gx0.grow(b * n)); HIP_TRY(h, h->sens.gu.grow(b * h->nz));
    HIP_TRY(h, hipMemcpyAsync(h->sens.gu, g_u, b * h->nz * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (g_x) {
        HIP_TRY(h, h->sens.gx.grow(b * xs));
        HIP_TRY(h, hipMemcpyAsync(h->sens.gx, g_x, b * xs * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    p.g_u = h->sens.gu; p.g_x = g_x ? h->sens.gx.get() : nullptr; p.g_x0 = h->sens.gx0; p.rows = h->sens.vrows;
    return ALMPC_OK;
}

int sens_vjp(almpc_handle* h, const char* who, bool rows_form, const double* g_u, const double* g_x, double act_tol, double act_tol_x,
             double* g_x0, int32_t* rows_out) {
    ALMPC_TRY(sens_check(h, who, rows_form));
    if (!g_u || !g_x0) return fail(h, ALMPC_ERR_INVALID, std::string(who) + ": null g_u or g_x0");
    const bool rows = rows_form && h->mc > 0;
    if (rows) ALMPC_TRY(sens_fits(h, true));
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(wait_and_settle(h));
    const size_t b = (size_t)h->batch, n = (size_t)h->n;
    SensParams p;
    ALMPC_TRY(sens_params(h, act_tol, p, rows, act_tol_x));
    ALMPC_TRY(sens_vjp_stage(h, g_u, g_x, p));
    if (rows) ALMPC_TRY((sens_launch<true, true>(h, p)));
    else ALMPC_TRY((sens_launch<true, false>(h, p)));
    HIP_TRY(h, hipMemcpyAsync(g_x0, h->sens.gx0, b * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (rows_out) HIP_TRY(h, hipMemcpyAsync(rows_out, h->sens.vrows, b * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, stream_wait_polling(h));
    return ALMPC_OK;
}

// ---- almpc_sensitivity_params_vjp: k_sens_pz (the VJP with z, nu and the bound gradients), then k_sens_params where a group behind
// the stage recursions is wanted; only the wanted groups are computed and copied.
// follow_dare (almpc_sensitivity_params_vjp_dare): k_sens_params also computes dL/dP, and one launch of k_dare_vjp adds what the loss
// gains through P_i = DARE(A_i, B_i, Q, R) to the Q, R, A, B groups in sens.pout, in front of the copies back.

// What the call can look at and be asked for, and the dynamic LDS of all three kernels, in front of everything it enqueues
int sens_params_vjp_check(almpc_handle* h, const char* who, bool follow_dare, const double* g_u, const almpc_param_grads* out) {
    ALMPC_TRY(sens_check(h, who));
    const std::string w(who);
    if (!g_u || !out) return fail(h, ALMPC_ERR_INVALID, w + ": null g_u or out");
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    if (follow_dare) {
        if (!h->kept.useR) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the design dropped R (R[1,1] == 0): there is no DARE to follow");
        if (h->n > DARE_MAX_N || h->m > DARE_MAX_M) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": n <= 48 and m <= 16 (k_dare_vjp)");
        if (h->kept.R.size() != m * m) return fail(h, ALMPC_ERR_INVALID, w + ": the design's weights are not kept");
    }
    if (!out->u_ref && !out->Q && !out->P && !out->A && !out->R && !out->S && !out->B && !out->x0 && !out->f && !out->u_min && !out->u_max && !out->rows)
        return fail(h, ALMPC_ERR_INVALID, w + ": every pointer of out is null");
    if (h->kept.Q.size() != n * n || h->kept.S.size() != m * m || (!h->batched && h->P.size() != n * n))
        return fail(h, ALMPC_ERR_INVALID, w + ": the design's weights are not kept");
    const size_t lds1 = (size_t)SENS_WAVES * sens_pz_lds_doubles(h->n, h->nzs, SENS_CAP1) * sizeof(double);
    const size_t lds2 = h->nz > SENS_CAP1 ? (size_t)sens_pz_lds_doubles(h->n, h->nzs, h->nz) * sizeof(double) : 0;
    const size_t lds3 = (size_t)sens_grad_lds_doubles(h->n) * sizeof(double);
    if (lds1 > 160 * 1024 || lds2 > 160 * 1024 || lds3 > 160 * 1024) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the working set does not fit LDS");
    return ALMPC_OK;
}

// k_sens_pz's two tiers, as sens_launch
int sens_pz_launch(almpc_handle* h, SensParams p) {
    const int n = h->n, nz = h->nz, nzs = h->nzs;
    HIP_TRY(h, hipMemsetAsync(h->sens.ovf, 0, SENS_OVF_HEAD * sizeof(int32_t), h->stream));
    p.cap = SENS_CAP1; p.lds_per_team = sens_pz_lds_doubles(n, nzs, p.cap);
    const size_t lds1 = (size_t)SENS_WAVES * p.lds_per_team * sizeof(double);
    HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_sens_pz<false>), lds1));
    hipLaunchKernelGGL((k_sens_pz<false>), dim3((unsigned)((h->batch + SENS_WAVES - 1) / SENS_WAVES)), dim3(64 * SENS_WAVES), lds1, h->stream, p);
    HIP_TRY(h, hipGetLastError());
    if (nz > SENS_CAP1) {
        p.cap = nz; p.lds_per_team = sens_pz_lds_doubles(n, nzs, p.cap);
        HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_sens_pz<true>), p.lds_per_team * sizeof(double)));
        hipLaunchKernelGGL((k_sens_pz<true>), dim3((unsigned)std::min(h->batch, 4 * h->num_cus)), dim3(SENS_WG), p.lds_per_team * sizeof(double), h->stream, p);
        HIP_TRY(h, hipGetLastError());
    }
    return ALMPC_OK;
}

// k_sens_params' outputs in sens.pout: u_ref, Q, P, A, R, S, B, each [batch][its size]
struct ParamGradLayout {
    size_t ur, Q, P, A, R, S, B, total;
    ParamGradLayout(size_t b, size_t n, size_t m, size_t nz)
        : ur(0), Q(ur + b * nz), P(Q + b * n * n), A(P + b * n * n), R(A + b * n * n), S(R + b * m * m), B(S + b * m * m), total(B + b * n * m) {}
};

// k_sens_params behind k_sens_pz's z, nu and rows: the wanted groups (with_gP: dL/dP whether or not it is wanted, for the DARE chain).
// The shared weights are the handle's kept ones; per-instance weights are on the device already.
int sens_params_launch(almpc_handle* h, const SensParams& p, const almpc_param_grads* out, bool with_gP, const ParamGradLayout& L, SensGradParams& q) {
    const size_t n = (size_t)h->n, m = (size_t)h->m, xs = n * (h->N + 1);
    KeptDev w;
    ALMPC_TRY(kept_on_device(h, h->weighted ? 0u : KEPT_Q | KEPT_S | (h->kept.R.size() == m * m ? KEPT_R : 0u) | (h->batched ? 0u : KEPT_P), w));
    const int grid = std::min(h->batch, 8 * h->num_cus);
    HIP_TRY(h, h->sens.pout.grow(L.total));
    HIP_TRY(h, h->sens.traj.grow((size_t)grid * 3 * xs));
    q = SensGradParams();
    q.n = h->n; q.m = h->m; q.N = h->N; q.nz = h->nz; q.batch = h->batch; q.useR = h->kept.useR; q.useS = h->kept.useS;
    q.A = p.A; q.A_stride = p.A_stride; q.B = p.B; q.B_stride = p.B_stride; q.Q = w.Q; q.S = w.S;
    if (h->weighted) { q.Q = h->wiQ; q.Q_stride = (long)(n * n); q.S = h->kept.useS ? h->wiS.get() : nullptr; q.S_stride = h->kept.useS ? (long)(m * m) : 0; }
    if (h->batched) { q.P = h->bP; q.P_stride = h->bP_stride; }
    else { q.P = w.P; q.P_stride = 0; }
    q.ex = h->dEx; q.ev = h->dEu; q.u = h->dU; q.g_u = p.g_u; q.g_x = p.g_x; q.z = p.z; q.nu = p.nu; q.rows = p.rows; q.traj = h->sens.traj;
    double* o = h->sens.pout;
    q.gur = out->u_ref ? o + L.ur : nullptr; q.gQ = out->Q ? o + L.Q : nullptr; q.gP = (out->P || with_gP) ? o + L.P : nullptr;
    q.gA = out->A ? o + L.A : nullptr; q.gR = out->R ? o + L.R : nullptr; q.gS = out->S ? o + L.S : nullptr; q.gB = out->B ? o + L.B : nullptr;
    const size_t lds = (size_t)sens_grad_lds_doubles(h->n) * sizeof(double);
    HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_sens_params), lds));
    hipLaunchKernelGGL(k_sens_params, dim3((unsigned)grid), dim3(256), lds, h->stream, q);
    HIP_TRY(h, hipGetLastError());
    return ALMPC_OK;
}

// The DARE chain behind it (launch: a group the DARE reaches is wanted, and q is k_sens_params' launch): k_dare_vjp on dL/dP (at gP_at of sens.pout),
// added to the Q, R, A, B groups of q.  Then its status words, in front of the copies back: without dare_status a refused instance
// fails the call, and nothing is copied out.
int sens_dare_chain(almpc_handle* h, const char* who, bool launch, const SensGradParams& q, size_t gP_at, int32_t* dare_status) {
    const size_t b = (size_t)h->batch, n = (size_t)h->n, m = (size_t)h->m;
    std::vector<int32_t> stt(b, 0);
    if (launch) {
        HIP_TRY(h, h->sens.dstat.grow(b));
        HIP_TRY(h, hipMemsetAsync(h->sens.dstat, 0, b * sizeof(int32_t), h->stream));   // (an instance with rows < 0 is skipped: 0)
        KeptDev w;
        ALMPC_TRY(kept_on_device(h, h->weighted ? 0u : KEPT_Q | KEPT_R, w));
        DareVjpParams vp;
        vp.n = h->n; vp.m = h->m; vp.batch = h->batch;
        vp.A = q.A; vp.A_stride = q.A_stride; vp.B = q.B; vp.B_stride = q.B_stride; vp.P = q.P; vp.P_stride = q.P_stride;
        vp.gP = h->sens.pout + gP_at; vp.gP_stride = (long)(n * n);
        vp.Q = w.Q; vp.R = w.R;
        if (h->weighted) { vp.Q = h->wiQ; vp.Q_stride = (long)(n * n); vp.R = h->wiR; vp.R_stride = (long)(m * m); }
        vp.gA = q.gA; vp.gA_stride = (long)(n * n); vp.gB = q.gB; vp.gB_stride = (long)(n * m);
        vp.gQ = q.gQ; vp.gQ_stride = (long)(n * n); vp.gR = q.gR; vp.gR_stride = (long)(m * m);
        vp.accumulate = 1; vp.rows = q.rows; vp.status = h->sens.dstat; vp.lds_per_wave = 0;
        HIP_TRY(h, launch_dare_vjp(vp, h->stream));
        HIP_TRY(h, hipMemcpyAsync(stt.data(), h->sens.dstat, b * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, stream_wait_polling(h));
    }
    if (dare_status) std::copy(stt.begin(), stt.end(), dare_status);
    else
        for (size_t i = 0; i < b; ++i)
            if (stt[i] != 0)
                return fail(h, ALMPC_ERR_NUMERIC, std::string(who) + ": the terminal weight of instance " + std::to_string(i) +
                            " is not the stabilising DARE solution of its model (k_dare_vjp status " + std::to_string(stt[i]) + ")");
    return ALMPC_OK;
}

// The wanted groups back to the host (pout: k_sens_params ran), and the wait
int sens_params_back(almpc_handle* h, const almpc_param_grads* out, const SensParams& p, const double* pout, const ParamGradLayout& L) {
    const size_t b = (size_t)h->batch, n = (size_t)h->n, m = (size_t)h->m, nz = (size_t)h->nz;
    const auto back = [&](double* dst, const double* src, size_t count) {
        return dst ? hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToHost, h->stream) : hipSuccess;
    };
    HIP_TRY(h, back(out->x0, h->sens.gx0, b * n));
    HIP_TRY(h, back(out->f, p.z, b * nz));
    HIP_TRY(h, back(out->u_min, p.gmin, b * m));
    HIP_TRY(h, back(out->u_max, p.gmax, b * m));
    if (pout) {
        HIP_TRY(h, back(out->u_ref, pout + L.ur, b * nz));
        HIP_TRY(h, back(out->Q, pout + L.Q, b * n * n));
        HIP_TRY(h, back(out->P, pout + L.P, b * n * n));
        HIP_TRY(h, back(out->A, pout + L.A, b * n * n));
        HIP_TRY(h, back(out->R, pout + L.R, b * m * m));
        HIP_TRY(h, back(out->S, pout + L.S, b * m * m));
        HIP_TRY(h, back(out->B, pout + L.B, b * n * m));
    }
    if (out->rows) HIP_TRY(h, hipMemcpyAsync(out->rows, h->sens.vrows, b * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, stream_wait_polling(h));
    return ALMPC_OK;
}

int sens_params_vjp(almpc_handle* h, const double* g_u, const double* g_x, double act_tol, const almpc_param_grads* out,
                    bool follow_dare = false, int32_t* dare_status = nullptr) {
    const char* who = follow_dare ? "sensitivity_params_vjp_dare" : "sensitivity_params_vjp";
    ALMPC_TRY(sens_params_vjp_check(h, who, follow_dare, g_u, out));
    const bool chain = follow_dare && (out->Q || out->R || out->A || out->B);   // (a group the DARE reaches)
    const bool want2 = out->u_ref || out->Q || out->P || out->A || out->R || out->S || out->B;   // (a group of k_sens_params)
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(wait_and_settle(h));
    const size_t b = (size_t)h->batch, m = (size_t)h->m, nz = (size_t)h->nz;
    SensParams p;
    ALMPC_TRY(sens_params(h, act_tol, p));
    ALMPC_TRY(sens_vjp_stage(h, g_u, g_x, p));
    HIP_TRY(h, h->sens.pz.grow(b * (2 * nz + 2 * m)));
    p.z = h->sens.pz; p.nu = p.z + b * nz; p.gmin = p.nu + b * nz; p.gmax = p.gmin + b * m;
    ALMPC_TRY(sens_pz_launch(h, p));
    const ParamGradLayout L(b, (size_t)h->n, m, nz);
    SensGradParams q;
    if (want2) ALMPC_TRY(sens_params_launch(h, p, out, chain, L, q));
    if (follow_dare) ALMPC_TRY(sens_dare_chain(h, who, chain, q, L.P, dare_status));
    return sens_params_back(h, out, p, want2 ? h->sens.pout.get() : nullptr, L);
}

// ---- the same on a structured handle (k_sens_face, k_sens_face_rate): the Riccati recursion on the face, no condensed operand ----
// One path for almpc_sensitivity_stagewise[_vjp] (rate false: designs with S = 0) and almpc_sensitivity_stagewise_rate[_vjp] (rate
// true: with or without S).  k_sens_face_rate runs where the call takes S and the design has it (rate && h->kept.useS); a rate call on a
// design without S launches k_sens_face on the operands of the plain call: the same bytes.

// What these calls can look at: the last step of a structured design with an input box only
int sens_face_check(almpc_handle* h, const char* who, bool rate) {
    if (!h) return ALMPC_ERR_INVALID;
    const std::string w(who);
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, w + " before design");
    // (in front of the handle's kind: almpc_design_ltv exists on condensed handles only, and its refusal names the call that serves it)
    if (h->ltv || h->sqp.ready) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": time-varying and SQP designs solve for a step around a trajectory, not for u(x0) (an almpc_design_ltv design, in its initial deviation: almpc_sensitivity_ltv)");
    if (!h->structured) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the handle is a condensed one, whose sensitivities come from G = H'^-1 (almpc_sensitivity)");
    if (h->relin.ready) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the re-linearisation pipeline's models depend on x0 themselves");
    if (!rate && h->kept.useS) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": with an input-rate weight S the stage state is [e_k; v_(k-1)], for which the recursion is not built");
    if (h->has_box || h->terminal_eq || (h->sd.ready && (h->sd.has_box || h->sd.has_eq)))
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": state rows (state box, terminal equality) are not held on the face of the stage-wise recursion");
    if (!h->rQ || !h->rR || !(h->r_batched_P ? h->bP.get() : h->rP.get()))
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the shape is outside the primal stage-wise solver, whose weights the recursion reads (n <= 32, m <= 16, m N <= 1024)");
    if (rate && h->kept.useS && (h->weighted || h->kept.S.size() != (size_t)h->m * h->m))
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the design's shared input-rate weight is not kept");
    const int lds = h->kept.useS ? sens_face_rate_lds_doubles(h->n, h->m, h->N) : sens_face_lds_doubles(h->n, h->m, h->N);   // (useS: a rate call)
    if ((size_t)lds * sizeof(double) > (size_t)LDS_BUDGET)
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": a stage of the recursion does not fit LDS");
    if (!h->sens.stepped) return fail(h, ALMPC_ERR_INVALID, w + ": no step has run on this design");
    return ALMPC_OK;
}

// Operands of a launch: the models, weights and results k_riccati is launched with (launch_riccati) in q.f; with_S (k_sens_face_rate)
// also S, which goes to the device once per design, and that kernel's slice of LDS
int sens_face_params(almpc_handle* h, double act_tol, bool with_S, SensFaceRateParams& q) {
    q = SensFaceRateParams();
    SensFaceParams& p = q.f;
    p.n = h->n; p.m = h->m; p.N = h->N; p.batch = h->batch;
    p.A = h->batched ? h->bA : h->dA; p.A_stride = h->batched ? (long)h->n * h->n : 0;
    p.B = h->batched ? h->bB : h->dB; p.B_stride = h->batched ? (long)h->n * h->m : 0;
    p.Q = h->rQ; p.R = h->rR;
    p.P = h->r_batched_P ? h->bP : h->rP; p.P_stride = h->r_batched_P ? h->rP_stride : 0;
    p.umin = h->dUmin; p.umax = h->dUmax; p.u = h->dU; p.status = h->dStatus;
    p.tau = act_tol > 0.0 ? act_tol : 1e-7;   // (ten times what k_sdual's confirmation leaves a working-set row away from its bound)
    p.lds_per_wave = with_S ? sens_face_rate_lds_doubles(h->n, h->m, h->N) : sens_face_lds_doubles(h->n, h->m, h->N);
    if (!with_S) return ALMPC_OK;
    KeptDev w;
    ALMPC_TRY(kept_on_device(h, KEPT_S, w));
    q.S = w.S;
    return ALMPC_OK;
}

// (q.S is set exactly where sens_face_params was asked for k_sens_face_rate's operands)
template <bool VJP>
int sens_face_launch(almpc_handle* h, const SensFaceRateParams& q) {
    const bool with_S = q.S != nullptr;
    const size_t per_wave = (size_t)q.f.lds_per_wave * sizeof(double);
    const int waves = waves_in_lds(per_wave, with_S ? SENS_FACE_RATE_WAVES : SENS_FACE_WAVES), wgs = capped_grid(h->batch, waves, 16 * h->num_cus);
    const bool quad = h->n == 12 && h->m == 4;
    if (with_S && quad) HIP_TRY(h, LAUNCH_WAVES((k_sens_face_rate<VJP, 12, 4>), wgs, waves, waves * per_wave, h->stream, q));
    else if (with_S) HIP_TRY(h, LAUNCH_WAVES((k_sens_face_rate<VJP, 0, 0>), wgs, waves, waves * per_wave, h->stream, q));
    else if (quad) HIP_TRY(h, LAUNCH_WAVES((k_sens_face<VJP, 12, 4>), wgs, waves, waves * per_wave, h->stream, q.f));
    else HIP_TRY(h, LAUNCH_WAVES((k_sens_face<VJP, 0, 0>), wgs, waves, waves * per_wave, h->stream, q.f));
    return ALMPC_OK;
}

int sens_face_jacobians(almpc_handle* h, const char* who, uint32_t want, double act_tol, bool rate) {
    ALMPC_TRY(sens_face_check(h, who, rate));
    if (!want || (want & ~(ALMPC_SENS_K0 | ALMPC_SENS_DU | ALMPC_SENS_DX))) return fail(h, ALMPC_ERR_INVALID, std::string(who) + ": want must be a mask of ALMPC_SENS_*");
    const bool with_S = rate && h->kept.useS;
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(wait_and_settle(h));
    const size_t b = (size_t)h->batch, n = (size_t)h->n;
    h->sens.have = 0;
    SensFaceRateParams q;
    ALMPC_TRY(sens_face_params(h, act_tol, with_S, q));
    HIP_TRY(h, h->sens.rows.grow(b));
    if (want & ALMPC_SENS_K0) HIP_TRY(h, h->sens.K0.grow(b * n * h->m));
    if (want & (ALMPC_SENS_DU | ALMPC_SENS_DX)) {   // (the forward pass writes dU on its way to dX)
        HIP_TRY(h, h->sens.dU.grow(b * n * h->nz));
        HIP_TRY(h, h->sens.Kst.grow(b * h->nz * (n + (with_S ? h->m : 0))));
    }
    if (want & ALMPC_SENS_DX) HIP_TRY(h, h->sens.dX.grow(b * n * (h->N + 1) * n));
    q.f.want = want; q.f.K0 = h->sens.K0; q.f.dU = h->sens.dU; q.f.dX = h->sens.dX; q.f.Kst = h->sens.Kst; q.f.rows = h->sens.rows;
    ALMPC_TRY(sens_face_launch<false>(h, q));
    HIP_TRY(h, stream_wait_polling(h));
    h->sens.have = want | ((want & ALMPC_SENS_DX) ? ALMPC_SENS_DU : 0u);
    return ALMPC_OK;
}

int sens_face_vjp(almpc_handle* h, const char* who, const double* g_u, const double* g_x, double act_tol, double* g_x0, int32_t* rows_out,
                  bool rate) {
    ALMPC_TRY(sens_face_check(h, who, rate));
    if (!g_u || !g_x0) return fail(h, ALMPC_ERR_INVALID, std::string(who) + ": null g_u or g_x0");
    const bool with_S = rate && h->kept.useS;
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(wait_and_settle(h));
    const size_t b = (size_t)h->batch, n = (size_t)h->n;
    SensFaceRateParams q;
    ALMPC_TRY(sens_face_params(h, act_tol, with_S, q));
    ALMPC_TRY(sens_vjp_stage(h, g_u, g_x, q.f));
    ALMPC_TRY(sens_face_launch<true>(h, q));
    HIP_TRY(h, hipMemcpyAsync(g_x0, h->sens.gx0, b * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (rows_out) HIP_TRY(h, hipMemcpyAsync(rows_out, h->sens.vrows, b * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, stream_wait_polling(h));
    return ALMPC_OK;
}

// ---- the same for a step of a time-varying design (k_sens_ltv): the face recursion with the kept stage models, in the initial deviation ----
// almpc_sensitivity_ltv, almpc_sensitivity_ltv_vjp.  RATE is the design's branch (kept.useS); the weights are the design's own device
// copies (wQ, wR, wS: batched_design_front), the terminal weights its bP.

// What these calls can look at: the last step of an almpc_design_ltv design that kept its stage models, with an input box only
int sens_ltv_check(almpc_handle* h, const char* who) {
    if (!h) return ALMPC_ERR_INVALID;
    const std::string w(who);
    if (!h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, w + " before design");
    if (!h->ltv || h->sqp.ready || h->relin.ready)
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the design is not almpc_design_ltv's (condensed time-invariant designs: almpc_sensitivity, almpc_sensitivity_rows; "
                                                  "structured handles: almpc_sensitivity_stagewise_rate; the re-linearisation pipeline's models depend on x0 themselves; "
                                                  "the SQP loop's Jacobians belong to the iterate before the update)");
    if (h->has_box || h->terminal_eq || h->mc > 0)
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": state rows (state box, terminal equality) are not held on the face of the stage-wise recursion");
    if (!h->cert.kept || !h->lA || !h->lB)
        return fail(h, ALMPC_ERR_INVALID, w + ": the design released its stage models (almpc_set_keep_stage_models(h, 1) before almpc_design_ltv)");
    if (h->n > SENS_LTV_MAX_N || h->m > SENS_LTV_MAX_M || (long)(h->N + 1) * (h->n + h->m) > SENS_LTV_MAX_STATES)
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": needs n <= 16, m <= 16 and (N + 1)(n + m) <= 1024, the shapes a step of an LTV design runs at");
    if (!h->wQ || !h->wR || !h->wS || !h->bP) return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": the design's weights are not kept");
    if (!h->sens.stepped) return fail(h, ALMPC_ERR_INVALID, w + ": no step has run on this design");
    return ALMPC_OK;
}

void sens_ltv_params(almpc_handle* h, double act_tol, SensLtvParams& q) {
    q = SensLtvParams();
    SensFaceParams& p = q.f;
    const long n = h->n, m = h->m, N = h->N;
    p.n = h->n; p.m = h->m; p.N = h->N; p.batch = h->batch;
    p.A = h->lA; p.A_stride = N * n * n;
    p.B = h->lB; p.B_stride = N * n * m;
    p.Q = h->wQ; p.R = h->wR; q.S = h->wS; q.useR = h->kept.useR;
    p.P = h->bP; p.P_stride = h->bP_stride;
    p.umin = h->dUmin; p.umax = h->dUmax; p.u = h->dU; p.status = h->dStatus;
    p.tau = act_tol > 0.0 ? act_tol : 1e-7;   // (k_sens_face's rule and default)
    p.lds_per_wave = sens_ltv_lds_doubles(h->n, h->m, h->N, h->kept.useS != 0);
}

template <bool VJP>
int sens_ltv_launch(almpc_handle* h, const SensLtvParams& q) {
    const size_t per_wave = (size_t)q.f.lds_per_wave * sizeof(double);
    const int waves = waves_in_lds(per_wave, SENS_LTV_WAVES), wgs = capped_grid(h->batch, waves, 16 * h->num_cus);
    const bool quad = h->n == 12 && h->m == 4, rate = h->kept.useS != 0;
    if (rate && quad) HIP_TRY(h, LAUNCH_WAVES((k_sens_ltv<VJP, true, 12, 4>), wgs, waves, waves * per_wave, h->stream, q));
    else if (rate) HIP_TRY(h, LAUNCH_WAVES((k_sens_ltv<VJP, true, 0, 0>), wgs, waves, waves * per_wave, h->stream, q));
    else if (quad) HIP_TRY(h, LAUNCH_WAVES((k_sens_ltv<VJP, false, 12, 4>), wgs, waves, waves * per_wave, h->stream, q));
    else HIP_TRY(h, LAUNCH_WAVES((k_sens_ltv<VJP, false, 0, 0>), wgs, waves, waves * per_wave, h->stream, q));
    return ALMPC_OK;
}

int sens_ltv_jacobians(almpc_handle* h, uint32_t want, double act_tol) {
    const char* who = "sensitivity_ltv";
    ALMPC_TRY(sens_ltv_check(h, who));
    if (!want || (want & ~(ALMPC_SENS_K0 | ALMPC_SENS_DU | ALMPC_SENS_DX))) return fail(h, ALMPC_ERR_INVALID, std::string(who) + ": want must be a mask of ALMPC_SENS_*");
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(wait_and_settle(h));
    const size_t b = (size_t)h->batch, n = (size_t)h->n;
    h->sens.have = 0;
    SensLtvParams q;
    sens_ltv_params(h, act_tol, q);
    HIP_TRY(h, h->sens.rows.grow(b));
    if (want & ALMPC_SENS_K0) HIP_TRY(h, h->sens.K0.grow(b * n * h->m));
    if (want & (ALMPC_SENS_DU | ALMPC_SENS_DX)) {   // (the forward pass writes dU on its way to dX; K0 alone allocates no gain scratch)
        HIP_TRY(h, h->sens.dU.grow(b * n * h->nz));
        HIP_TRY(h, h->sens.Kst.grow(b * h->nz * (n + (h->kept.useS ? h->m : 0))));
    }
    if (want & ALMPC_SENS_DX) HIP_TRY(h, h->sens.dX.grow(b * n * (h->N + 1) * n));
    q.f.want = want; q.f.K0 = h->sens.K0; q.f.dU = h->sens.dU; q.f.dX = h->sens.dX; q.f.Kst = h->sens.Kst; q.f.rows = h->sens.rows;
    ALMPC_TRY(sens_ltv_launch<false>(h, q));
    HIP_TRY(h, stream_wait_polling(h));
    h->sens.have = want | ((want & ALMPC_SENS_DX) ? ALMPC_SENS_DU : 0u);
    return ALMPC_OK;
}

int sens_ltv_vjp(almpc_handle* h, const double* g_u, const double* g_x, double act_tol, double* g_x0, int32_t* rows_out) {
    const char* who = "sensitivity_ltv_vjp";
    ALMPC_TRY(sens_ltv_check(h, who));
    if (!g_u || !g_x0) return fail(h, ALMPC_ERR_INVALID, std::string(who) + ": null g_u or g_x0");
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(wait_and_settle(h));
    const size_t b = (size_t)h->batch, n = (size_t)h->n;
    SensLtvParams q;
    sens_ltv_params(h, act_tol, q);
    ALMPC_TRY(sens_vjp_stage(h, g_u, g_x, q.f));
    ALMPC_TRY(sens_ltv_launch<true>(h, q));
    HIP_TRY(h, hipMemcpyAsync(g_x0, h->sens.gx0, b * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (rows_out) HIP_TRY(h, hipMemcpyAsync(rows_out, h->sens.vrows, b * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, stream_wait_polling(h));
    return ALMPC_OK;
}

// ---- certificate of the last step: cost, KKT residual, input gradient, costates from the returned trajectories and the design ----
// Three forms on one host path: Plain (almpc_certificate: a time-invariant design, k_cert), Ltv (almpc_certificate_ltv: k_cert_ltv on
// almpc_design_ltv's kept stage models, also the predicted states), Relin (almpc_relin_fnn_certificate: the pipeline's step is a
// per-instance time-invariant design, so k_cert on the step's own A_i, B_i, P_i and the setup's weights)
enum class CertForm { Plain, Ltv, Relin };
constexpr uint32_t CERT_ALL = ALMPC_CERT_COST | ALMPC_CERT_RES | ALMPC_CERT_GRAD | ALMPC_CERT_COSTATE;
constexpr uint32_t CERT_LTV_ALL = CERT_ALL | ALMPC_CERT_STATES;

// What a form can look at: the last step of a design of its kind.  With state rows the trajectory alone determines the cost (and
// the states) only.
int cert_check(almpc_handle* h, CertForm form, uint32_t want) {
    if (!h) return ALMPC_ERR_INVALID;
    const bool ltv = form == CertForm::Ltv, relin = form == CertForm::Relin;
    const std::string w(ltv ? "certificate_ltv" : relin ? "relin_fnn_certificate" : "certificate");
    if (relin ? !h->relin.ready && !h->designed : !h->designed) return fail(h, ALMPC_ERR_NOT_DESIGNED, w + (relin ? " before relin_fnn_setup" : " before design"));
    if (!want || (want & ~(ltv ? CERT_LTV_ALL : CERT_ALL)))
        return fail(h, ALMPC_ERR_INVALID, w + ": want must be a mask of ALMPC_CERT_*" + (ltv ? " and ALMPC_CERT_STATES" : ""));
    // the design's kind (Ltv: and that it left its stage models)
    if (ltv) {
        if (!h->ltv || h->sqp.ready || h->relin.ready)
            return fail(h, ALMPC_ERR_UNSUPPORTED, "certificate_ltv: the design is not almpc_design_ltv's (time-invariant designs: almpc_certificate; the re-linearisation "
                                                  "pipeline: almpc_relin_fnn_certificate; the SQP loop has no certificate)");
        if (!h->cert.kept || !h->lA || !h->lB || (h->cert.kept_c && !h->lC) || !h->cert.xref || !h->cert.uref)
            return fail(h, ALMPC_ERR_INVALID, "certificate_ltv: the design released its stage models (almpc_set_keep_stage_models(h, 1) before almpc_design_ltv)");
    } else if (relin) {
        if (!h->relin.ready) return fail(h, ALMPC_ERR_UNSUPPORTED, "relin_fnn_certificate: the design is not the re-linearisation pipeline's (almpc_certificate, almpc_certificate_ltv)");
    } else {
        if (h->ltv || h->sqp.ready) return fail(h, ALMPC_ERR_UNSUPPORTED, "certificate: the QP of a time-varying or SQP design has a defect term and a trajectory of its own");
        if (h->relin.ready) return fail(h, ALMPC_ERR_UNSUPPORTED, "certificate: the re-linearisation pipeline's QP has a defect term and a trajectory of its own");
    }
    const bool state_rows = h->has_box || h->terminal_eq || h->mc > 0 || (!ltv && h->sd.ready && (h->sd.has_box || h->sd.has_eq));
    if (state_rows && (want & ~(ALMPC_CERT_COST | (ltv ? ALMPC_CERT_STATES : 0u))))
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": with state rows (state box, terminal equality) their multipliers enter the costates, and the trajectory does not determine them: " +
                                              (ltv ? "ALMPC_CERT_COST and ALMPC_CERT_STATES alone are served" : "ALMPC_CERT_COST alone is served"));
    if (ltv) {
        if (h->n > CERT_LTV_MAX_N || h->m > CERT_LTV_MAX_M || (long)(h->N + 1) * (h->n + h->m) > CERT_LTV_MAX_STATES)
            return fail(h, ALMPC_ERR_UNSUPPORTED, "certificate_ltv: needs n <= 16, m <= 16 and (N + 1)(n + m) <= 1024, the shapes a step of an LTV design runs at");
    } else if (h->n > CERT_MAX_N || h->m > CERT_MAX_M || (size_t)cert_lds_doubles(h->n, h->m) * sizeof(double) > (size_t)LDS_BUDGET)
        return fail(h, ALMPC_ERR_UNSUPPORTED, w + ": needs n <= 64, m <= 16 and the operands of an instance in 160 KB of LDS");
    // the weights the form's kernel reads are there (Ltv: batched_design_front left them on the device -- wQ, wR, wS)
    const almpc_handle::Kept& k = h->kept;
    const size_t nn = (size_t)h->n * h->n, mm = (size_t)h->m * h->m;
    if (relin) {
        if (k.Q.size() != nn || k.R.size() != mm || k.S.size() != mm || !h->bA || !h->bB || !h->bP)
            return fail(h, ALMPC_ERR_UNSUPPORTED, "relin_fnn_certificate: the pipeline's weights and models are not kept");
    } else if (ltv) {
    } else if (h->structured) {
        // (a guard: almpc_create gives a structured handle only to the primal stage-wise solver's shapes, and every design of one
        // leaves that solver's weights on the device -- riccati_weights)
        if (!h->rQ || !h->rR || !(h->r_batched_P ? h->bP.get() : h->rP.get()))
            return fail(h, ALMPC_ERR_UNSUPPORTED, "certificate: the shape is outside the primal stage-wise solver, whose weights the kernel reads (n <= 32, m <= 16, m N <= 1024)");
        if (k.S.size() != mm) return fail(h, ALMPC_ERR_UNSUPPORTED, "certificate: the design's input-rate weight is not kept");
    } else if (h->weighted) {
        if (!h->wiQ || !h->wiR || (k.useS && !(h->wiS_given && h->wiS))) return fail(h, ALMPC_ERR_UNSUPPORTED, "certificate: the design's per-instance weights are not kept");
    } else if (k.Q.size() != nn || k.R.size() != mm || k.S.size() != mm || (!h->batched && h->P.size() != nn)) {
        return fail(h, ALMPC_ERR_UNSUPPORTED, "certificate: the design's weights are not kept");
    }
    if (relin ? !h->relin.have_prev || !h->designed || !h->sens.stepped : !h->sens.stepped)
        return fail(h, ALMPC_ERR_INVALID, w + (relin ? ": no step has run since relin_fnn_setup" : ": no step has run on this design"));
    return ALMPC_OK;
}

// The wanted outputs of the four both kernels have, grown, into the parameters of either (the LTV form adds x and ex itself)
template <class Params>
int cert_outputs(almpc_handle* h, uint32_t want, Params& p) {
    const size_t b = (size_t)h->batch;
    almpc_handle::Cert& c = h->cert;
    if (want & ALMPC_CERT_COST) { HIP_TRY(h, c.cost.grow(b)); p.cost = c.cost; }
    if (want & ALMPC_CERT_RES) { HIP_TRY(h, c.res.grow(b)); p.res = c.res; }
    if (want & ALMPC_CERT_GRAD) { HIP_TRY(h, c.grad.grow(b * h->nz)); p.grad = c.grad; }
    if (want & ALMPC_CERT_COSTATE) { HIP_TRY(h, c.costate.grow(b * (size_t)h->n * (h->N + 1))); p.costate = c.costate; }
    return ALMPC_OK;
}

// k_cert's operands.  Models and per-instance weights are on the device already; shared weights are the handle's kept ones (a
// structured design: the primal stage-wise solver's).  relin: the step's own Jacobians (k_c2d's result with almpc_set_model_time)
// and P -- one for the batch, or the last step's P_i (almpc_set_terminal_weight) -- in the per-instance slots, the setup's Q, R, S.
int cert_params(almpc_handle* h, bool relin, uint32_t want, CertParams& p) {
    p = CertParams();
    const size_t n = (size_t)h->n, m = (size_t)h->m, nn = n * n, mm = m * m;
    const bool riccati = h->structured && !relin;
    p.n = h->n; p.m = h->m; p.N = h->N; p.batch = h->batch;
    p.useR = h->kept.useR; p.useS = h->kept.useS;
    p.A = h->batched ? h->bA : h->dA; p.A_stride = h->batched ? (long)nn : 0;
    p.B = h->batched ? h->bB : h->dB; p.B_stride = h->batched ? (long)(n * m) : 0;
    if (riccati) {
        p.Q = h->rQ; p.R = h->rR;
        p.P = h->r_batched_P ? h->bP : h->rP; p.P_stride = h->r_batched_P ? h->rP_stride : 0;
    } else {
        if (h->weighted) { p.Q = h->wiQ; p.Q_stride = (long)nn; p.R = h->wiR; p.R_stride = (long)mm; p.S = h->wiS; p.S_stride = (long)mm; }
        if (h->batched) { p.P = h->bP; p.P_stride = h->bP_stride; }
    }
    KeptDev w;
    ALMPC_TRY(kept_on_device(h, (!riccati && !h->weighted ? KEPT_Q | KEPT_R : 0u) | ((p.useS || relin) && !h->weighted ? KEPT_S : 0u) |
                                    (!riccati && !h->batched ? KEPT_P : 0u), w));
    if (w.Q) { p.Q = w.Q; p.R = w.R; }
    if (w.S) p.S = w.S;
    if (w.P) p.P = w.P;
    p.umin = h->dUmin; p.umax = h->dUmax;
    p.ex = h->dEx; p.eu = h->dEu; p.u = h->dU;
    p.lds_per_wave = cert_lds_doubles(h->n, h->m);
    return cert_outputs(h, want, p);
}

int cert_launch(almpc_handle* h, const CertParams& p) {
    const size_t per_wave = (size_t)p.lds_per_wave * sizeof(double);
    const int waves = waves_in_lds(per_wave, CERT_WAVES), wgs = capped_grid(h->batch, waves, 16 * h->num_cus);
    if (h->n <= 16) HIP_TRY(h, LAUNCH_WAVES((k_cert<16>), wgs, waves, waves * per_wave, h->stream, p));
    else if (h->n <= 32) HIP_TRY(h, LAUNCH_WAVES((k_cert<32>), wgs, waves, waves * per_wave, h->stream, p));
    else HIP_TRY(h, LAUNCH_WAVES((k_cert<64>), wgs, waves, waves * per_wave, h->stream, p));
    return ALMPC_OK;
}

// k_cert_ltv from u, e_u and what the design kept: the stage models, its references and its weights on the device
int cert_ltv_launch(almpc_handle* h, uint32_t want) {
    CertLtvParams p = CertLtvParams();
    p.n = h->n; p.m = h->m; p.N = h->N; p.batch = h->batch;
    p.useR = h->kept.useR; p.useS = h->kept.useS;
    p.A = h->lA; p.B = h->lB; p.c = h->cert.kept_c ? h->lC.get() : nullptr;
    p.Q = h->wQ; p.R = h->wR; p.S = h->wS;   // (the design's weights, symmetrised: batched_design_front)
    p.P = h->bP; p.P_stride = h->bP_stride;
    p.umin = h->dUmin; p.umax = h->dUmax;
    p.xbar = h->dXref; p.xref = h->cert.xref; p.uref = h->cert.uref;   // (dXref: the design's almpc_set_reference(xbar, ubar, 1))
    p.eu = h->dEu; p.u = h->dU;
    ALMPC_TRY(cert_outputs(h, want, p));
    const size_t xs = (size_t)h->batch * h->n * (h->N + 1);
    if (want & ALMPC_CERT_STATES) { HIP_TRY(h, h->cert.x.grow(xs)); HIP_TRY(h, h->cert.ex.grow(xs)); p.x = h->cert.x; p.ex = h->cert.ex; }
    p.lds_per_wave = cert_ltv_lds_doubles(h->n, h->N);
    const size_t per_wave = (size_t)p.lds_per_wave * sizeof(double);
    const int waves = waves_in_lds(per_wave, CERT_LTV_WAVES), wgs = capped_grid(h->batch, waves, CERT_LTV_WGS_PER_CU * h->num_cus);
    if (p.c) HIP_TRY(h, LAUNCH_WAVES((k_cert_ltv<true>), wgs, waves, waves * per_wave, h->stream, p));
    else HIP_TRY(h, LAUNCH_WAVES((k_cert_ltv<false>), wgs, waves, waves * per_wave, h->stream, p));
    return ALMPC_OK;
}

int certificate(almpc_handle* h, CertForm form, uint32_t want) {
    ALMPC_TRY(cert_check(h, form, want));
    HIP_TRY(h, hipSetDevice(h->device));
    ALMPC_TRY(wait_and_settle(h));   // (a synchronous look: the certificate is of the results a caller would read, redone instances included)
    h->cert.have = 0;
    if (form == CertForm::Ltv) ALMPC_TRY(cert_ltv_launch(h, want));
    else {
        CertParams p;
        ALMPC_TRY(cert_params(h, form == CertForm::Relin, want, p));
        ALMPC_TRY(cert_launch(h, p));
    }
    HIP_TRY(h, stream_wait_polling(h));
    h->cert.have = want; h->cert.ltv_form = form == CertForm::Ltv;
    return ALMPC_OK;
}

// The getters and the device views of either pair: the last certificate call's buffers, where it was of this form (ltv: the _ltv
// pair, with x and e_x / d_x and d_ex)
int get_certificate(almpc_handle* h, bool ltv, double* cost, double* res, double* grad, double* costate, double* x, double* e_x) {
    if (!h) return ALMPC_ERR_INVALID;
    const std::string w(ltv ? "certificate_ltv" : "certificate");
    const uint32_t have = h->cert.ltv_form == ltv ? h->cert.have : 0u;
    const uint32_t need = (cost ? ALMPC_CERT_COST : 0u) | (res ? ALMPC_CERT_RES : 0u) | (grad ? ALMPC_CERT_GRAD : 0u) |
                          (costate ? ALMPC_CERT_COSTATE : 0u) | ((x || e_x) ? ALMPC_CERT_STATES : 0u);
    if (!have || (need & ~have))
        return fail(h, ALMPC_ERR_INVALID, "get_" + w + ": not computed for the last step (almpc_" + w + " with these ALMPC_CERT_* bits first)");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t b = (size_t)h->batch, xs = (size_t)h->n * (h->N + 1);
    if (cost) HIP_TRY(h, hipMemcpy(cost, h->cert.cost, b * sizeof(double), hipMemcpyDeviceToHost));
    if (res) HIP_TRY(h, hipMemcpy(res, h->cert.res, b * sizeof(double), hipMemcpyDeviceToHost));
    if (grad) HIP_TRY(h, hipMemcpy(grad, h->cert.grad, b * h->nz * sizeof(double), hipMemcpyDeviceToHost));
    if (costate) HIP_TRY(h, hipMemcpy(costate, h->cert.costate, b * xs * sizeof(double), hipMemcpyDeviceToHost));
    if (x) HIP_TRY(h, hipMemcpy(x, h->cert.x, b * xs * sizeof(double), hipMemcpyDeviceToHost));
    if (e_x) HIP_TRY(h, hipMemcpy(e_x, h->cert.ex, b * xs * sizeof(double), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

int device_certificate(almpc_handle* h, bool ltv, const double** d_cost, const double** d_res, const double** d_grad, const double** d_costate,
                       const double** d_x, const double** d_ex) {
    if (!h) return ALMPC_ERR_INVALID;
    const uint32_t have = h->cert.ltv_form == ltv ? h->cert.have : 0u;
    if (!have) return fail(h, ALMPC_ERR_INVALID, std::string(ltv ? "device_certificate_ltv" : "device_certificate") + ": not computed for the last step");
    if (d_cost) *d_cost = (have & ALMPC_CERT_COST) ? h->cert.cost.get() : nullptr;
    if (d_res) *d_res = (have & ALMPC_CERT_RES) ? h->cert.res.get() : nullptr;
    if (d_grad) *d_grad = (have & ALMPC_CERT_GRAD) ? h->cert.grad.get() : nullptr;
    if (d_costate) *d_costate = (have & ALMPC_CERT_COSTATE) ? h->cert.costate.get() : nullptr;
    if (d_x) *d_x = (have & ALMPC_CERT_STATES) ? h->cert.x.get() : nullptr;
    if (d_ex) *d_ex = (have & ALMPC_CERT_STATES) ? h->cert.ex.get() : nullptr;
    return ALMPC_OK;
}

}  // namespace

extern "C" {

int almpc_certificate(almpc_handle* h, uint32_t want) { return certificate(h, CertForm::Plain, want); }

int almpc_set_keep_stage_models(almpc_handle* h, int on) {
    if (!h) return ALMPC_ERR_INVALID;
    h->cert.keep = on != 0;
    return ALMPC_OK;
}

int almpc_certificate_ltv(almpc_handle* h, uint32_t want) { return certificate(h, CertForm::Ltv, want); }

int almpc_relin_fnn_certificate(almpc_handle* h, uint32_t want) { return certificate(h, CertForm::Relin, want); }

int almpc_get_certificate(almpc_handle* h, double* cost, double* res, double* grad, double* costate) {
    return get_certificate(h, false, cost, res, grad, costate, nullptr, nullptr);
}

int almpc_get_certificate_ltv(almpc_handle* h, double* cost, double* res, double* grad, double* costate, double* x, double* e_x) {
    return get_certificate(h, true, cost, res, grad, costate, x, e_x);
}

int almpc_device_certificate(almpc_handle* h, const double** d_cost, const double** d_res, const double** d_grad, const double** d_costate) {
    return device_certificate(h, false, d_cost, d_res, d_grad, d_costate, nullptr, nullptr);
}

int almpc_device_certificate_ltv(almpc_handle* h, const double** d_cost, const double** d_res, const double** d_grad, const double** d_costate,
                                 const double** d_x, const double** d_ex) {
    return device_certificate(h, true, d_cost, d_res, d_grad, d_costate, d_x, d_ex);
}

int almpc_sensitivity(almpc_handle* h, uint32_t want, double act_tol) {
    return sens_jacobians(h, "sensitivity", false, want, act_tol, 0.0);
}

int almpc_sensitivity_rows(almpc_handle* h, uint32_t want, double act_tol_u, double act_tol_x) {
    return sens_jacobians(h, "sensitivity_rows", true, want, act_tol_u, act_tol_x);
}

int almpc_get_sensitivity(almpc_handle* h, double* K0, double* dU, double* dX, int32_t* rows) {
    if (!h) return ALMPC_ERR_INVALID;
    const uint32_t need = (K0 ? ALMPC_SENS_K0 : 0u) | (dU ? ALMPC_SENS_DU : 0u) | (dX ? ALMPC_SENS_DX : 0u);
    if (!h->sens.have || (need & ~h->sens.have))
        return fail(h, ALMPC_ERR_INVALID, "get_sensitivity: not computed for the last step (almpc_sensitivity with these ALMPC_SENS_* bits first)");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t b = (size_t)h->batch, n = (size_t)h->n;
    if (K0) HIP_TRY(h, hipMemcpy(K0, h->sens.K0, b * n * h->m * sizeof(double), hipMemcpyDeviceToHost));
    if (dU) HIP_TRY(h, hipMemcpy(dU, h->sens.dU, b * n * h->nz * sizeof(double), hipMemcpyDeviceToHost));
    if (dX) HIP_TRY(h, hipMemcpy(dX, h->sens.dX, b * n * (h->N + 1) * n * sizeof(double), hipMemcpyDeviceToHost));
    if (rows) HIP_TRY(h, hipMemcpy(rows, h->sens.rows, b * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ALMPC_OK;
}

int almpc_device_sensitivity(almpc_handle* h, const double** d_K0, const double** d_dU, const double** d_dX, const int32_t** d_rows) {
    if (!h) return ALMPC_ERR_INVALID;
    if (!h->sens.have) return fail(h, ALMPC_ERR_INVALID, "device_sensitivity: not computed for the last step");
    if (d_K0) *d_K0 = (h->sens.have & ALMPC_SENS_K0) ? h->sens.K0.get() : nullptr;
    if (d_dU) *d_dU = (h->sens.have & ALMPC_SENS_DU) ? h->sens.dU.get() : nullptr;
    if (d_dX) *d_dX = (h->sens.have & ALMPC_SENS_DX) ? h->sens.dX.get() : nullptr;
    if (d_rows) *d_rows = h->sens.rows.get();
    return ALMPC_OK;
}

int almpc_sensitivity_vjp(almpc_handle* h, const double* g_u, const double* g_x, double act_tol, double* g_x0, int32_t* rows) {
    return sens_vjp(h, "sensitivity_vjp", false, g_u, g_x, act_tol, 0.0, g_x0, rows);
}

int almpc_sensitivity_rows_vjp(almpc_handle* h, const double* g_u, const double* g_x, double act_tol_u, double act_tol_x, double* g_x0,
                               int32_t* rows) {
    return sens_vjp(h, "sensitivity_rows_vjp", true, g_u, g_x, act_tol_u, act_tol_x, g_x0, rows);
}

int almpc_sensitivity_params_vjp(almpc_handle* h, const double* g_u, const double* g_x, double act_tol, const almpc_param_grads* out) {
    return sens_params_vjp(h, g_u, g_x, act_tol, out);
}

int almpc_sensitivity_params_vjp_dare(almpc_handle* h, const double* g_u, const double* g_x, double act_tol, const almpc_param_grads* out,
                                      int32_t* dare_status) {
    return sens_params_vjp(h, g_u, g_x, act_tol, out, true, dare_status);
}

int almpc_sensitivity_stagewise(almpc_handle* h, uint32_t want, double act_tol) {
    return sens_face_jacobians(h, "sensitivity_stagewise", want, act_tol, false);
}

int almpc_sensitivity_stagewise_vjp(almpc_handle* h, const double* g_u, const double* g_x, double act_tol, double* g_x0, int32_t* rows) {
    return sens_face_vjp(h, "sensitivity_stagewise_vjp", g_u, g_x, act_tol, g_x0, rows, false);
}

int almpc_sensitivity_stagewise_rate(almpc_handle* h, uint32_t want, double act_tol) {
    return sens_face_jacobians(h, "sensitivity_stagewise_rate", want, act_tol, true);
}

int almpc_sensitivity_stagewise_rate_vjp(almpc_handle* h, const double* g_u, const double* g_x, double act_tol, double* g_x0, int32_t* rows) {
    return sens_face_vjp(h, "sensitivity_stagewise_rate_vjp", g_u, g_x, act_tol, g_x0, rows, true);
}

int almpc_sensitivity_ltv(almpc_handle* h, uint32_t want, double act_tol) { return sens_ltv_jacobians(h, want, act_tol); }

int almpc_sensitivity_ltv_vjp(almpc_handle* h, const double* g_u, const double* g_x, double act_tol, double* g_x0, int32_t* rows) {
    return sens_ltv_vjp(h, g_u, g_x, act_tol, g_x0, rows);
}

}  // extern "C"

extern "C" {

#ifdef ALMPC_STAMPS
// diagnostic build: allocate / fetch the stamp buffer ([waves][16] int64)
int almpc_dbg_stamps_enable(almpc_handle* h, int waves) {
    DevBuf<long long, Mem::DeviceTight> buf;
    if (buf.alloc((size_t)waves * 16) != hipSuccess) return -3;
    long long* d = buf.release();   // (never freed: g_stamps points at it for the life of the process)
    (void)hipMemset(d, 0, (size_t)waves * 16 * sizeof(long long));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(almpc::g_stamps), &d, sizeof(d));
    return 0;
}
int almpc_dbg_stamps_fetch(almpc_handle* h, long long* out, int waves) {
    long long* d = nullptr;
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(&d, HIP_SYMBOL(almpc::g_stamps), sizeof(d));
    if (!d) return -1;
    return hipMemcpy(out, d, (size_t)waves * 16 * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
#endif

}  // extern "C"

#include "almpc_hostio.inc.h"
