/*
 * ndp_nmpc.h -- C-ABI of the MI355X-native batched NMPC + downwash control step.
 *
 * Drop-in boundary for the hot path of Li-Jinjie/ndp_nmpc_qd.  In the reference this
 * boundary is acados_template's ctypes binding of the generated solver
 * (AcadosOcpSolver.set / get / solve_for_x0, used at
 *  ndp_nmpc/scripts/nmpc_ctl/nmpc_body_rate_ctl.py:84-112 and
 *  ndp_nmpc/scripts/ndp_nmpc_ctl/ndp_nmpc_body_rate_ctl.py:82-112)
 * plus torch's CUDA module call in dnwash_nn_est/downwash_nn.py:21-29.
 * Each entry point below names the reference interface it replaces.
 *
 * Conventions
 *  - plain C, no C++ types, no exceptions across the boundary;
 *  - every function returns 0 on success, >0 = solver status of the worst instance
 *    (acados ints: 1 NaN, 4 QP failure), <0 = API misuse or HIP error
 *    (text via ndp_last_error);
 *  - host arrays are row-major, batch-major: x0[B][10], xr[B][N+1][10], ur[B][N][4],
 *    f[B][N+1][3] (fp32), other[B][N+1][10], ego_xy[B][2], u0[B][4];
 *    state order [px,py,pz,vx,vy,vz,qw,qx,qy,qz] (nmpc_body_rate_ctl.py:130),
 *    control order [wx,wy,wz,c] (:144);
 *  - the caller owns every pointer for the duration of the call only; the library owns
 *    device memory and the persistent SQP iterate (the warm start acados keeps);
 *  - a handle is internally serialised (mutex): update / reset / get may be called from
 *    different threads, as rospy does (nmpc_node.py:94,152,237);
 *  - *_device variants take device pointers (HBM-resident inputs) and a hipStream_t
 *    passed as void*; they enqueue work and do not synchronise.
 */
#ifndef NDP_NMPC_H
#define NDP_NMPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDP_NX 10
#define NDP_NU 4
#define NDP_MLP_NPARAM 17859 /* 6-128-64-128-3 with biases, nn_net.py:7-18 */
#define NDP_MLP_W23_LIMIT 65504.0f /* |W2|, |W3| must stay below the largest finite fp16 (ndp_set_mlp_weights) */

/* Version of this interface: bumped whenever an exported signature or the layout of ndp_cfg changes.  A binding built against
 * another header must refuse to run: ndp_abi_version() is what the loaded library was built with, ndp_cfg_size() its
 * sizeof(ndp_cfg) (ndp_create / ndp_default_cfg read and write that many bytes of the caller's struct). */
#define NDP_ABI_VERSION 9
int ndp_abi_version(void);
size_t ndp_cfg_size(void);

#define NDP_QP_AUTO 0       /* exact early exit when no bound is active, else interior point */
#define NDP_QP_IPM_ALWAYS 1 /* always run the interior-point loop (what HPIPM does) */
#define NDP_AS_GAMMA_FLOOR 1e8 /* ndp_cfg.as_gamma >= NDP_AS_GAMMA_FLOOR * max_i(dt * Rd[i]) when as_iter_max > 0 (ndp_create) */

#define NDP_PREC_F64 0        /* product path: v_mfma_f64_16x16x4_f64 */
#define NDP_PREC_F32_STUDY 1  /* f64 kernel, operands of the sweeps' matrix instructions rounded to fp32 (numerics only) */
#define NDP_PREC_BF16_STUDY 2 /* ... rounded to bf16 */
#define NDP_PREC_F32_MFMA 3   /* the Riccati sweeps on v_mfma_f32_16x16x4_f32 */
#define NDP_PREC_BF16_MFMA 4  /* the Riccati sweeps on v_mfma_f32_16x16x16_bf16 (bf16 in, fp32 accumulate) */
/* What status 0 means in each mode: the step satisfies its QP's KKT conditions up to a relative residual (the largest of the
 * equality residual and the input box's natural residual, each over the largest term that enters it; tests/kkt_certificate.py) of
 *   NDP_PREC_F64 (and every mode for a QP it hands to the fp64 path): 1e-9 after the active-set iterations, 3e5 tol after the
 *     interior-point loop (an answer mu / lambda inside a bound with a small multiplier lambda);
 *   NDP_PREC_F32_MFMA 1e-3 (7e-5 measured);  NDP_PREC_BF16_MFMA 1 (0.71 measured: a bf16-operand sweep is not a solve);
 *   NDP_PREC_COND_F32 / _BF16 0.3: a condensed result is kept only when its fp64 stationarity residual is at most 0.3, else the fp64
 *     path solves the QP (fp32 results: <= 0.13 measured; bf16 results: >= 0.81, i.e. in practice never kept). */
#define NDP_PREC_COND_F32 5   /* BASELINE configs[4] as worded -- "fp32 vs bf16 MFMA on the CONDENSED QP": the first solve of every QP in condensed
                               * form (prediction matrices, H = R + Gamma' Q Gamma and the gradient as tiled products on v_mfma_f32_16x16x4_f32, fp32
                               * Cholesky in LDS, csrc/cond_qp.hpp); kept when it passes the fp64 inside-the-box and stationarity tests, else the fp64 Riccati path
                               * solves the QP.  A STUDY mode (the reference does not condense: qp_solver_cond_N = N): N a multiple of 4, <= 40 */
#define NDP_PREC_COND_BF16 6  /* ... the products on v_mfma_f32_16x16x16_bf16 (fp32 accumulate, fp32 Cholesky) */

typedef struct ndp_cfg {
    int32_t batch;      /* B: independent OCP instances in this handle            */
    int32_t N;          /* shooting intervals        params/nmpc_params.py:9      */
    int32_t n_rti;      /* SQP-RTI iterations per step (reference: 1)             */
    int32_t use_fd;     /* 1 = NDP model, disturbance force in p (ndp_...ctl.py:146-162) */
    int32_t qp_mode;    /* NDP_QP_*                                               */
    int32_t iter_max;   /* interior-point iteration cap (acados default 50)       */
    int32_t device;     /* HIP device ordinal                                     */
    int32_t qp_precision; /* NDP_PREC_*: 0 = product path (fp64).  BASELINE config 5 ("fp32 vs bf16 MFMA on the QP") only:
                           * 3 / 4 run the Riccati sweeps on the fp32 / bf16-input matrix instructions (everything else stays
                           * fp64); 1 / 2 are the first round's operand-rounding studies on the fp64 kernel */
    int32_t work_queue; /* instances whose QP needs the interior-point loop are re-distributed over all SIMDs through an
                         * work list (producer + consumer launch per step): 0 = automatic, 1 = on, 2 = off.  Automatic: the N = 40 /
                         * 2-iteration shape always takes the list; the reference shape (N = 20, 1 iteration) with qp_mode AUTO and a
                         * batch >= 2 x the device's SIMD count starts in place and switches by what its steps do -- the list on when
                         * >= 4 % of the instances of a window of 8 steps went into the interior-point loop, off at <= 1.5 % (the list
                         * costs a step that lists nothing 8-15 %, and gains 70 % when a fifth of the instances iterate); decided at
                         * launch time, so a captured graph keeps its form */
    int32_t ipm_refine; /* interior point: while a STATE bound's barrier term lambda / t exceeds refine_gamma, the 4x4 block is
                         * factorised L D L' and applied by substitution (an explicit inverse costs the recursion its definiteness
                         * there) and every Newton system's solution is refined this many times with the factorisation at hand
                         * (default 2; 0 = never: round 3's loop).  The loop is in absolute form, so an iteration's answer is as
                         * accurate as its last solve -- cond ~ lambda / t.
                         * The reference's velocity box (+-20 m/s, nmpc_body_rate_ctl.py:59-61) is never active in its envelope:
                         * this only acts on boxes shrunk on purpose.
                         * WHERE IT ACTS: the three-slot kernels only (N <= 27: run-time and compile-time horizons alike), in place and
                         * through the work list.  The five-slot kernels (N >= 28, e.g. config 5's N = 40) and the lean late-force step
                         * (ndp_step_device_prefetched) carry no stiff sweep and no second solve -- they sit at the register limit.
                         * ndp_create REFUSES ipm_refine > 0 for a shape whose kernels have no such path (N >= 28, or qp_precision != 0:
                         * error -2; set ipm_refine = 0 -- a strongly active state bound at a tight tolerance then ends in status 4,
                         * never in a silent answer).  The lean late-force step of an N <= 27 handle runs without it as well
                         * (ndp_refine_active() = what the handle's ordinary steps do). */
    double dt;          /* T_horizon / N_node        params/nmpc_params.py:10,12  */
    double mass;        /* params/fhnp_params.py:9   */
    double gravity;     /* params/fhnp_params.py:12  */
    double r_horiz;     /* params/downwash_params.py:10 */
    double Qd[10];      /* diag(Q)   nmpc_body_rate_ctl.py:48 */
    double Rd[4];       /* diag(R)   nmpc_body_rate_ctl.py:49 */
    double lbu[4], ubu[4]; /* nmpc_body_rate_ctl.py:56-58 */
    double lbv[3], ubv[3]; /* nmpc_body_rate_ctl.py:59-61 (stages 1..N-1) */
    double mu0, thr0, tol, tau; /* interior-point constants */
    double auto_margin;         /* NDP_QP_AUTO accepts the equality-constrained minimiser only if it is this far inside every
                                 * bound (default 0.1); closer to a bound the interior-point loop runs, as in the reference */
    double ts_nmpc;             /* control period, params/nmpc_params.py:11 (0.02): spacing of the reference list entries */
    double mu_floor;            /* interior point: the centring target sigma*mu never goes below mu_floor * tol (default 0.1) --
                                 * slacks are differences, so driving mu far below tol only loses digits */
    double refine_gamma;        /* see ipm_refine (default 1e4) */
    /* NDP_QP_AUTO, active set on the INPUT bounds (nmpc_body_rate_ctl.py:56-58 -- the only bounds ever active in the reference's
     * envelope): when the equality-constrained minimiser leaves the box, inputs beyond a bound are pinned there, pins whose
     * multiplier has the wrong sign are released, and the QP is solved again -- ONE Riccati sweep per iteration -- until the set
     * reproduces itself; the KKT conditions of the box-constrained QP then hold: it IS the solution HPIPM iterates towards
     * (any method converging the same strictly convex QP is parity-equivalent).  The set is kept per instance between control steps
     * (the warm start the reference leaves off, nmpc_body_rate_ctl.py:73-74): a step whose set still holds costs one sweep.
     * as_iter_max: sweeps with pins allowed behind the first one (default 8; 0 = off: rounds 1-5's behaviour, early exit only
     * auto_margin inside every bound, else the interior-point loop).  A violated VELOCITY bound, a set that does not settle, a failed
     * factorisation: the interior-point loop takes the QP, as before.  ndp_reset / ndp_set_iterate empty the kept sets.
     * as_gamma: the weight that holds a pinned input on its bound (default 1e12: the input is then within multiplier / 1e12 of
     * the bound and set onto it exactly).  With as_iter_max > 0, ndp_create refuses (-2) an as_gamma that is not finite or is below
     * NDP_AS_GAMMA_FLOOR * max_i(dt * Rd[i]): a weaker pin leaves the rest of the QP solved as if the input were free (1e6 at the
     * defaults: u off by 4e-6; 1e-3: off by 1.9), yet the input is written onto its bound with status 0. */
    int32_t as_iter_max;
    int32_t reserved0;
    double as_gamma;
} ndp_cfg;

typedef struct ndp_handle ndp_handle;

/* Fills cfg with the reference constants (the params package), batch = 1, N = 20. */
int ndp_default_cfg(ndp_cfg *cfg);

/* Replaces AcadosOcpSolver(ocp, json_file, build=...) (nmpc_body_rate_ctl.py:84):
 * allocates device state for cfg->batch instances.  Fails (<0) when no HIP device is usable. */
int ndp_create(const ndp_cfg *cfg, ndp_handle **out);
int ndp_destroy(ndp_handle *h);
const char *ndp_last_error(const ndp_handle *h); /* h may be NULL: last create error */

/* Replaces nn_model.load_state_dict(torch.load(...)) (downwash_nn.py:14-16).
 * blob: W1[128][6] b1 W2[64][128] b2 W3[128][64] b3 W4[3][128] b4, fp32, n = NDP_MLP_NPARAM.
 * Supported range: every parameter finite, |W2| and |W3| below NDP_MLP_W23_LIMIT.  Layers 2 and 3 run on fp16 pairs w = hi + lo / 2^11
 * (hi = fp16(w), lo = fp16((w - hi) * 2^11), fp16 subnormals kept): 22 significand bits down to an absolute resolution of 2^-35, so
 * weights may be scaled down by 2^-10 and more at the 1e-5 bar; a W2 / W3 entry of 65520 or more would become an fp16 infinity and every
 * force NaN.  Layers 1 and 4 and the biases are fp32; hidden activations that feed a split are capped at 65000.
 * Returns -2 with a reason in ndp_last_error, the weights installed before still in force, for n != NDP_MLP_NPARAM, a non-finite
 * parameter, or a W2 / W3 entry outside the range. */
int ndp_set_mlp_weights(ndp_handle *h, const float *blob, size_t n);

/* Replaces NMPCBodyRateController.reset (nmpc_body_rate_ctl.py:86-91):
 * iterate x_k := xr[k] (k=0..N), u_k := ur[k] (k=0..N-1), for every instance. */
int ndp_reset(ndp_handle *h, const double *xr, const double *ur);
int ndp_reset_device(ndp_handle *h, const void *d_xr, const void *d_ur, void *stream);

/* Replaces update(x0, xr, ur[, f]) = 2N+2 solver.set calls + solver.solve_for_x0(x0)
 * (nmpc_body_rate_ctl.py:93-112; ndp_nmpc_body_rate_ctl.py:91-112), batched.
 *   f      : [B][N+1][3] fp32 disturbance force, or NULL            (NDP: p_k[4:7])
 *   other  : [B][N+1][10] neighbour reference window, or NULL.  When given (and f is NULL,
 *            use_fd = 1) the force is predicted on the device exactly as
 *            NDPLeaderNode.sub_xf_pred_callback does (ndp_nmpc_leader_node.py:60-76):
 *            f = MLP((other - xr)[:, 0:6]) if |other[0].xy - ego_xy|^2 < r_horiz^2 else 0
 *   ego_xy : [B][2] ego odometry xy for that gate, or NULL = gate always open
 *   u0     : [B][4] out, u_0 after the full step
 * Returns the worst per-instance status (0 = all converged). */
int ndp_step(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
             const double *other, const double *ego_xy, double *u0);
int ndp_step_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                    const void *d_other, const void *d_ego_xy, void *d_u0, void *stream);
/* ndp_step plus, from the same call (one synchronisation, no further round trips), what the reference's callers read
 * after solve_for_x0: the new iterate (solver.get(i,"x"/"u"), nmpc_node.py:237), solver.status
 * (nmpc_body_rate_ctl.py:109) and the interior-point iterations.  Any of the four output pointers may be NULL.
 *
 * How a host-array step moves its data (both forms; the reference's call shape is host arrays in, host array out,
 * nmpc_body_rate_ctl.py:93-112).  The handle owns two slots of page-locked host mirrors (allocated by the first host step).
 * The caller's arrays are packed into a slot's input mirror by the handle's pack threads (NDP_PACK_THREADS, default: half
 * the hardware threads, at most 8, beside the caller); the kernel reads that mirror over PCIe and writes u0 / status /
 * iterations -- and a copy of the new iterate when X_out / U_out are given -- into the slot's output mirror itself: one
 * launch and one wait per call, no DMA operation, at every batch size.
 * The persistent iterate itself always lives in HBM (ndp_device_iterate_x / _u), whatever the batch size. */
int ndp_step_ex(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                const double *other, const double *ego_xy, double *u0, double *X_out, double *U_out,
                int32_t *status_out, int32_t *ipm_iters_out);
/* ndp_step_ex with the disturbance force in DOUBLE precision, f[B][N+1][3] fp64 (or NULL).  The reference concatenates the force
 * into a float64 parameter vector (p_k = [q_r, f_k], ndp_nmpc_body_rate_ctl.py:97-99) and hands that to acados: its own caller
 * only ever supplies DownwashNN's fp32 values (downwash_nn.py:28), for which this call and ndp_step_ex agree bit
 * for bit, but any other caller of the same Python API gets its float64 force to the last digit only through this entry (the
 * fp32 form would round it: 6e-8 relative).  The drop-in class's .solver facade always takes this one. */
int ndp_step_ex_f64(ndp_handle *h, const double *x0, const double *xr, const double *ur, const double *f, double *u0,
                    double *X_out, double *U_out, int32_t *status_out, int32_t *ipm_iters_out);
/* The same step in two halves, so that a caller can keep two control ticks in flight: ndp_step_begin packs the inputs into a
 * slot's page-locked mirror, enqueues ONE launch -- whose waves read that mirror over PCIe and write u0 / status / iterations into
 * the slot's page-locked output block themselves (zero-copy: no H2D / D2H copy operation) -- and returns without waiting;
 * ndp_step_end waits for the OLDEST begun step and hands its results over.  With a second ndp_step_begin issued before the first
 * ndp_step_end, the packing of tick i+1 runs while tick i's kernel does -- the reference's control loop has that freedom too: x0
 * comes from odometry, not from the previous u0 (nmpc_node.py:202-226).  At most two steps may be in flight (a third
 * ndp_step_begin returns -14); steps complete in order; the warm start of tick i+1 is tick i's iterate, as always (stream order).
 *   flags bit 0: ndp_step_end will be asked for the iterate (X_out / U_out) of this step.
 * Every begun step must be drained with ndp_step_end BEFORE ndp_reset / ndp_set_iterate (they wait for the device, but the
 * results of a step still in flight would be lost and its slot stays busy) and before ndp_destroy (which frees the mirrors a
 * running kernel reads and writes: it synchronises the handle's stream first, but steps begun on it are the caller's to finish).
 * ndp_step / ndp_step_ex = begin + end under one lock. */
int ndp_step_begin(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                   const double *other, const double *ego_xy, int flags);
int ndp_step_end(ndp_handle *h, double *u0, double *X_out, double *U_out, int32_t *status_out, int32_t *ipm_iters_out);
/* ndp_step_device with the neighbour windows addressed the way a multi-GPU exchange leaves them (the reference's PredXU
 * traffic, nmpc_node.py:116-133 -> ndp_nmpc_leader_node.py:60-76):
 *   other_stride   : doubles per node of d_other, 10 (full windows) or 6 (positions + velocities, all the gate and the MLP
 *                    read, downwash_nn.py:22) -- d_other is [rows][N+1][other_stride]
 *   d_other_index  : int32[B], row of d_other holding instance i's neighbour, < 0 = no neighbour (force 0: the plain NMPC
 *                    followers of a formation, three_qd_ndp_nmpc.launch:8,12); NULL = row i */
int ndp_step_device_ex(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                       const void *d_other, int other_stride, const void *d_other_index, const void *d_ego_xy,
                       void *d_u0, void *stream);

/* The downwash one tick ahead, beside the control step.  In the reference the network does not run inside the control loop: a
 * subscriber callback predicts the force when a neighbour message arrives (ndp_nmpc_leader_node.py:60-76) and the next control tick
 * uses the latest one (nmpc_node.py:202-209).  The same split on the device, as two launches that overlap:
 *   ndp_downwash_prefetch_device : gate + MLP for the NEXT control step on the handle's second stream (LDS-free kernel, resident
 *                                  beside the control-step kernel); d_other / other_stride / d_other_index / d_ego_xy as in
 *                                  ndp_step_device_ex, d_ego_ref = that tick's xr.  after_stream: a stream whose work so far (the
 *                                  producer of those windows) it must follow, or NULL; inside a stream capture pass the
 *                                  capturing stream on the first call (fork), NULL afterwards, and ndp_prefetch_join at the end.
 *                                  on_stream: NULL = the handle's second stream, or a stream of the caller's to launch on
 *                                  instead (it must not share a hardware queue with the control steps' stream: create it at
 *                                  another priority).  The two chains of launches order themselves through device-side tick
 *                                  words, so they may also be captured into two SEPARATE graphs and replayed side by side --
 *                                  measured on ROCm 7.2: parallel branches inside ONE hipGraph run one after the other.
 *   ndp_step_device_prefetched   : the control step that consumes the oldest unconsumed prediction: linearises without the
 *                                  force, takes it when it is there (normally long before) and corrects the dynamics defects --
 *                                  the force enters them additively.  One prediction per step, in order; at most two
 *                                  predictions may be ahead (two force slots).  A prediction that does not arrive within 100 ms
 *                                  (no matching prefetch call) = zero force, per-instance status 5, counted.
 *   ndp_prefetch_join            : makes `stream` wait for the second stream's work so far (end of a capture, or before reading
 *                                  the slots).
 *   ndp_prefetch_stats           : synchronises; out5 = {predictions completed, steps that took theirs, control-step waves whose
 *                                  wait timed out, downwash launches whose wait for a free slot timed out, control-step waves
 *                                  that started before their prediction was complete (they wait for it and read it past the L2)}.
 *   ndp_device_force_slot        : the two force slots, [B][N+1][3] fp32 (prediction m is in slot m & 1).
 * Not combined with the interior-point work list (cfg.work_queue = 2) and fp64 only. */
int ndp_downwash_prefetch_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index,
                                 const void *d_ego_ref, const void *d_ego_xy, void *after_stream, void *on_stream);
int ndp_step_device_prefetched(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, void *d_u0, void *stream);
int ndp_prefetch_join(ndp_handle *h, void *stream);
int ndp_prefetch_stats(ndp_handle *h, unsigned long long *out5);
void *ndp_device_force_slot(ndp_handle *h, int slot);

/* Replaces DownwashNN.update(other_pred_x, ego_pred_x) (downwash_nn.py:21-29), batched, with the
 * optional r_horiz gate.  f_out: [B][N+1][3] fp32. */
int ndp_downwash(ndp_handle *h, const double *other, const double *ego_ref, const double *ego_xy, float *f_out);
int ndp_downwash_device(ndp_handle *h, const void *d_other, const void *d_ego_ref, const void *d_ego_xy,
                        void *d_f_out, void *stream);

/* Replaces solver.get(i,"x"/"u") / solver.set(i,"x"/"u") (nmpc_node.py:237; nmpc_body_rate_ctl.py:88-91):
 * whole iterate of every instance, X[B][N+1][10], U[B][N][4]. */
int ndp_get_iterate(ndp_handle *h, double *X, double *U);
int ndp_set_iterate(ndp_handle *h, const double *X, const double *U);

/* Replaces solver.status (nmpc_body_rate_ctl.py:109): per-instance status of the last step and the
 * interior-point iterations it took (0 = early exit).  Either pointer may be NULL. */
int ndp_get_status(ndp_handle *h, int32_t *status, int32_t *ipm_iters);

/* What NDP_QP_AUTO's active-set iterations did in the last step (cfg.as_iter_max; no counterpart in the reference, whose HPIPM is
 * cold-started every call, nmpc_body_rate_ctl.py:71-74): sweeps[B] = Riccati sweeps the step's QPs took before the interior-point
 * loop, if that ran at all (1 = the first solve's set held); act[B][4N] = the set kept for the next step, element 4k + i = input i of
 * stage k: +1 on its upper bound, -1 on its lower, 0 free.  Either pointer may be NULL. */
int ndp_get_active_set(ndp_handle *h, int32_t *sweeps, int8_t *act);
/* The kept set handed in (same layout; entries -1, 0, +1): the warm start of the next step's QPs -- an instance that moves to another
 * handle / rank takes its set along with its iterate (ndp_set_iterate empties the set: call this after it).  A set that does not fit the
 * next QP costs sweeps, never the answer: the iterations end in a set that reproduces itself or in the interior-point loop. */
int ndp_set_active_set(ndp_handle *h, const int8_t *act);

/* Device views for callers that keep everything in HBM (bench, multi-GPU driver).  The getters above and
 * ndp_synchronize also wait for the last stream a *_device call was given. */
void *ndp_device_iterate_x(ndp_handle *h);
void *ndp_device_iterate_u(ndp_handle *h);
void *ndp_device_force(ndp_handle *h);   /* [B][N+1][3] fp32 written by the fused downwash */
int ndp_synchronize(ndp_handle *h);
int ndp_refine_active(ndp_handle *h);        /* 1: cfg.ipm_refine > 0 and this handle's control steps carry the refinement path (see ndp_cfg.ipm_refine); 0: ignored */
int ndp_work_queue_enabled(ndp_handle *h);   /* 1 if the handle's NEXT step runs the interior-point work list (cfg.work_queue; the automatic rule's current state) */

/* Initial-state sensitivities (acados: eval_param_sens + get(stage, "sens_u" / "sens_x") with respect to x0).  The derivative of the
 * QP each step solves with respect to x0 -- linearisation point, xr, ur and the force held fixed -- column j = d / dx0[j]:
 *   - QP finished by the active set or the equality-constrained early exit: with the final set held fixed (exact: the solution is
 *     piecewise affine in x0); the rows of pinned inputs are exactly 0;
 *   - QP finished by the interior-point loop (ipm_iters > 0): the derivative of its last Newton system (barrier-smoothed, HPIPM's meaning);
 *   - an instance with a nonzero status: NaN in all of its outputs.
 * ndp_sens_enable: level 1 writes du0/dx0 [B][4][10] (the stage-0 gain of the last Riccati sweep); level 2 also runs a forward sweep with
 * the 10-column right-hand side [I ; 0] and writes dU/dx0 [B][N][4][10] and dX/dx0 [B][N+1][10][10] (stage 0: the identity); 0 frees the
 * buffers.  Served for N <= 27, qp_precision 0, n_rti = 1 (else -2 and ndp_last_error says why).  Every later in-place or work-list step
 * (ndp_step*, ndp_step_begin / _end, ndp_step_device*, a graph captured around them) writes them; a captured graph keeps the form it was
 * captured with.  With sensitivities on, ndp_step_device_prefetched, ndp_tick*, ndp_xchg_tick* and ndp_rollout_device return -2.
 * ndp_get_sens: waits for the handle's work and copies; any pointer may be NULL; dU / dX on a level-1 handle: -2.
 * ndp_device_sens_*: the device buffers (NULL when not allocated at the current level). */
int ndp_sens_enable(ndp_handle *h, int level);
int ndp_sens_level(ndp_handle *h);
int ndp_get_sens(ndp_handle *h, double *du0_dx0, double *dU_dx0, double *dX_dx0);
void *ndp_device_sens_u0(ndp_handle *h);
void *ndp_device_sens_u(ndp_handle *h);
void *ndp_device_sens_x(ndp_handle *h);

/* Parameter sensitivities: the derivative of the same QP with respect to its data xr [N+1][10], ur [N][4] and the force f [N+1][3], with the
 * linearisation point, x0 and the final active set held fixed -- the same three cases as above (fixed set: exact, the rows of pinned
 * inputs exactly 0; interior point: its last Newton system; nonzero status: NaN).  Row i = d u0[i]:
 *   du0/dxr [B][4][N+1][10], du0/dur [B][4][N][4], du0/df [B][4][N+1][3] (float64; the force itself is read as float32).
 * Stage 0's reference rows are 0 (x0 is fixed) and so is f_N (it reaches no dynamics).  The force enters the dynamics additively, so
 * du0/df is written in every configuration: with cfg.use_fd = 0 it is the derivative with respect to an additive force at f = 0.
 * Computed by the adjoint of the last Riccati sweep (RtiWave::psens_out) in the same launch as the x0 sensitivities.  Served by the
 * fused step (any N <= 27) and by every N = 20 form; an unfused step at another horizon returns -2 (no kernel: see DESIGN.md).
 * ndp_sens_params_enable(h, 1): needs ndp_sens_enable level >= 1 (else -2), so every refusal of a sensitivity handle covers them; 0 frees
 * the buffers, and so does ndp_sens_enable(h, 0).  ndp_sens_params_enabled: 1 / 0.
 * ndp_get_sens_params: waits for the handle's work and copies; any pointer may be NULL; -2 when off.
 * ndp_device_sens_xr / _ur / _f: the device buffers (NULL when off). */
int ndp_sens_params_enable(ndp_handle *h, int on);
int ndp_sens_params_enabled(ndp_handle *h);
int ndp_get_sens_params(ndp_handle *h, double *du0_dxr, double *du0_dur, double *du0_df);
void *ndp_device_sens_xr(ndp_handle *h);
void *ndp_device_sens_ur(ndp_handle *h);
void *ndp_device_sens_f(ndp_handle *h);

/* Adjoint of the control step (reverse mode, a vector-Jacobian product): the derivative of one recorded step's QP -- with the same
 * meaning as the sensitivities above (fixed final set: exact, pinned inputs' rows exactly 0; interior point: its last Newton system;
 * nonzero status: NaN in every output of the instance) -- contracted with upstream gradients of its outputs u0 [B][4], X [B][N+1][10] and
 * U [B][N][4] (the new iterate; gu0 adds to U_0), written as dL/dx0 [B][10], dL/dxr [B][N+1][10], dL/dur [B][N][4], dL/df [B][N+1][3] (fp64;
 * stage 0's xr row and f_N are exactly 0; dL/df as du0/df: in every configuration).  Needs no sensitivities on, whatever ndp_sens_level.
 * The tape: what determines one step, copied by the caller device-to-device on its stream BEFORE the step --
 *   X_lin [B][N+1][10], U_lin [B][N][4] (ndp_device_iterate_x / _u) and act_lin [B][4N] int8 (ndp_device_active_set; NULL = empty sets),
 * plus the step's own x0, xr, ur and the fp32 force it used (the caller's f, or ndp_device_force after a step with neighbour windows;
 * NULL = no force).  The tape is caller-owned: any recorded step can be differentiated later, in any order.  At N = 20: 2.7 KB per instance.
 * ndp_step_vjp_device enqueues on `stream`: the step is recomputed from the tape (the same program, into a workspace of the handle -- the
 * engine's iterate, kept sets, sensitivity buffers and the tape are never written; two calls on one tape give bit-identical results),
 * then one adjoint sweep of its last QP.  Upstream pointers: NULL = 0, not all NULL; output pointers: NULL = not written.
 * d_u0_check [B][4] fp64 / d_status_check [B] int32 (optional): the recompute's u0 and status, equal to the recorded step's.
 * Served for qp_precision 0, n_rti = 1, N <= 27 (N = 20 and the run-time-horizon kernel); anything else returns -2 with a reason in
 * ndp_last_error and launches nothing. */
void *ndp_device_active_set(ndp_handle *h);
int ndp_step_vjp_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                        const void *d_X_lin, const void *d_U_lin, const void *d_act_lin,
                        const void *d_gu0, const void *d_gX, const void *d_gU,
                        void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_u0_check, void *d_status_check, void *stream);

/* The same adjoint with the gradient in the controller's own numbers beside it: the cost weights Qd [10], Rd [4]
 * (nmpc_body_rate_ctl.py:48-49) and the mass (fhnp_params.py:9).  ndp_step_vjp_device's arguments, meaning, tape, workspace and refusals
 * (its four outputs come out bit-equal), plus d_gmodel [B][16] fp64, required: per instance, columns 0..9 dL/dQd, 10..13 dL/dRd, 14 dL/dmass,
 * 15 written as 0.  One row per instance on purpose: the caller sums (or weights) over the batch, there is no atomic and no second launch,
 * and two calls are bit-identical.  Fixed final set: exact; the cost is linear in the weights, so with v the adjoint, x+ / u+ the new
 * iterate and s = dt (stage N: 1)
 *   dL/dQd[r] = -sum_k s v_k[r] (x+_k[r] - xr_k[r]) for r < 6, dL/dQd[6] = 0 exactly (its residual is the constant 0),
 *   dL/dQd[7+a] = -sum_k s (E(qr_k) v_q,k)[a] (E(qr_k) q+_k)[a],  dL/dRd[i] = -dt sum_{k<N} v_u,k[i] (u+_k[i] - ur_k[i]) (pinned inputs: 0),
 *   dL/dmass = -(1/m) sum_k dL/df_k . f_k with the fp32 force the step read (the force enters the model as f / m only); exactly 0 without one.
 * Interior point: its last Newton system; a nonzero status or a failed adjoint factorisation: NaN in all 16.  Served as
 * ndp_step_vjp_device is (qp_precision 0, n_rti = 1, N <= 27: kernels of its own for N = 20 and the run-time horizon); -2 with a reason otherwise. */
int ndp_step_vjp_model_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                              const void *d_X_lin, const void *d_U_lin, const void *d_act_lin,
                              const void *d_gu0, const void *d_gX, const void *d_gU,
                              void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_gmodel, void *d_u0_check, void *d_status_check,
                              void *stream);

/* Forward mode of the control step (a Jacobian-vector product): the derivative of one recorded step's QP -- the same derivative as the
 * adjoint's above (fixed final set: exact; interior point: its last Newton system) -- along n_tan directions of its data per call.  A
 * direction is (tx0 [10], txr [N+1][10], tur [N][4], tf [N+1][3]); its result is the first-order change of the step's whole output,
 * du0 [4], dX [N+1][10], dU [N][4] (du0 = dU_0; dX_0 = tx0).  All fp64 and instance-major, T = n_tan:
 *   d_tx0 [B][T][10], d_txr [B][T][N+1][10], d_tur [B][T][N][4], d_tf [B][T][N+1][3]     (NULL = 0, not all four NULL)
 *   d_du0 [B][T][4],  d_dX  [B][T][N+1][10], d_dU  [B][T][N][4]                         (NULL = not written, not all three NULL)
 * The row of a pinned input in dU is exactly 0; stage 0's txr row and tf_N move nothing; a nonzero status or a failed factorisation of
 * the tangent solve gives NaN in every output of the instance.  <g, JVP(t)> = <VJP(g), t> holds against ndp_step_vjp_device on one tape.
 * Tape, workspace, ordering, repeatability, d_u0_check and d_status_check: exactly ndp_step_vjp_device's (the two share the workspace; calls
 * on one handle are ordered).  The step is recomputed, then every direction costs one more Riccati sweep; T directions in one call give
 * what T calls of one give, bit for bit.  -2 with a reason in ndp_last_error, nothing launched: the adjoint's refusals (n_rti != 1,
 * qp_precision != 0, N >= 28, a missing x0 / xr / ur / X_lin / U_lin, d_f without use_fd), n_tan outside 1..NDP_JVP_MAX_TANGENTS, d_tf
 * without use_fd. */
#define NDP_JVP_MAX_TANGENTS 8
int ndp_step_jvp_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                        const void *d_X_lin, const void *d_U_lin, const void *d_act_lin, int n_tan,
                        const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf,
                        void *d_du0, void *d_dX, void *d_dU, void *d_u0_check, void *d_status_check, void *stream);

/* Forward mode along directions of the controller's own numbers as well: the cost weights Qd [10], Rd [4] and the mass -- the transpose of
 * ndp_step_vjp_model_device's d_gmodel.  ndp_step_jvp_device's arguments, meaning, tape, workspace, outputs and NaN rule, plus
 *   d_tmodel [B][T][16] fp64, required (-2 without it: "without it: ndp_step_jvp_device"): per instance and direction, columns 0..9 Qd',
 *   10..13 Rd', 14 mass', 15 not read by the step (the closed loop's plant share, ndp_closed_loop_jvp_model_device).
 * The four data tangents may all be NULL here.  The model direction ADDS to the data direction (the tangent is linear), so both may be given
 * together.  Same QP, same blocks, pins held at 0, dx_0 = tx0 or 0; with rho the residual of the NEW iterate (x+ - xr; attitude: E(qr) q+;
 * inputs: u+ - ur) and s = dt (stage N: 1) the added data are
 *   gradient rows r < 6: + s Qd'[r] rho_k[r];  attitude rows: + s (E(qr_k)' diag(Qd'[7], Qd'[8], Qd'[9]) E(qr_k) q+_k)[row - 6];
 *   input rows: + dt Rd'[i] rho_u,k[i] (pinned: 0);  defects, k < N: -(mass' / m^2) [h^2/2 f_k; h f_k; 0] with the fp32 force the step read.
 * Qd'[6] enters nowhere (its residual is the constant 0): a direction in column 6 alone gives exact zeros, and so does a mass direction
 * when the step read no force.  T directions in one call are T calls of one, bit for bit.
 * With d_tmodel all zeros the outputs EQUAL ndp_step_jvp_device's on the same data tangents as numbers, not bit for bit: the added terms are
 * zeros added to the data entries, which can turn a -0.0 entry into +0.0, so the sign of a zero may differ; no nonzero value differs.
 * Duality: <gu0, du0> + <gX, dX> + <gU, dU> = <gx0, tx0> + <gxr, txr> + <gur, tur> + <gf, tf> + sum_{j<15} gmodel[j] tmodel[j] against
 * ndp_step_vjp_model_device on the same tape, to rounding.
 * Refusals (-2, nothing launched): ndp_step_jvp_device's but for "no tangent"; d_tmodel NULL.  Kernels of their own (rti_mjvp_kernel, N = 20
 * and the run-time horizon): ndp_step_jvp_device launches what it launched. */
int ndp_step_jvp_model_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                              const void *d_X_lin, const void *d_U_lin, const void *d_act_lin, int n_tan,
                              const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf, const void *d_tmodel,
                              void *d_du0, void *d_dX, void *d_dU, void *d_u0_check, void *d_status_check, void *stream);

/* Changes the model of a live handle: Qd [10] replaces ndp_cfg.Qd (nmpc_body_rate_ctl.py:48), Rd [4] ndp_cfg.Rd (nmpc_body_rate_ctl.py:49),
 * mass ndp_cfg.mass (fhnp_params.py:9).  Qd / Rd NULL = keep; mass <= 0 or NaN = keep.  Refused with -2 and a reason in ndp_last_error,
 * changing nothing: a non-finite entry, a negative Qd, a non-positive Rd, an infinite mass, and -- with as_iter_max > 0 -- an Rd that breaks
 * ndp_create's rule as_gamma >= NDP_AS_GAMMA_FLOOR * max_i(dt * Rd[i]).
 * The call waits for the handle's work in flight, then updates the configuration, the kernel parameters and the device's constants table
 * together.  The iterate, kept active sets, tapes, network weights, estimator state and sensitivity buffers stay as they are: a training
 * loop keeps its warm start.  A step after the call is bit-equal to the same step on a handle created with these values and given the same
 * iterate and kept sets.  The mass also reaches ndp_plant_step, the actuator command, the thrust estimator and the reference windows'
 * flatness map from the next call on.
 * The kernel parameters travel by value in the kernel arguments: launches enqueued after the call see the new model; anything the caller
 * captured earlier into a graph of their own keeps the old arguments and must be captured again.  A tape recorded before the call can
 * still be differentiated, but the adjoint recomputes the step with the handle's CURRENT model: restore the model the step ran with first. */
int ndp_set_model(ndp_handle *h, const double *Qd, const double *Rd, double mass);

/* Adjoint of DownwashNN.update + the r_horiz gate (downwash_nn.py:21-29, ndp_nmpc_leader_node.py:60-76) as ndp_step_device_ex
 * evaluates them: the vector-Jacobian product of the 6-128-64-128-3 network (nn_net.py:7-18) with d_gf [B][N+1][3] fp64
 * (ndp_step_vjp_device's d_gf as it lies; rounded to fp32).  d_other / other_stride (6 or 10) / d_other_index (int32 [B], < 0 = no
 * neighbour, NULL = row i) / d_ego_ref [B][N+1][10] / d_ego_xy ([B][2], NULL = gate open) as the step that produced the force took them.
 * The forward is recomputed with the step's own arithmetic, so the ReLU masks are those of the force the step used; the capped ReLU's
 * upper branch has derivative 0 like the lower one.  Outputs, each NULL = not computed, not both NULL:
 *   d_gz [B][N+1][6] fp64 : dL/d((other - ego_ref)[:, 0:6]) per row, 0 on closed / neighbour-less instances (the gate is
 *                            piecewise constant: its own derivative is 0 and is not represented)
 *   d_gw [NDP_MLP_NPARAM] fp32, blob order of ndp_set_mlp_weights, OVERWRITTEN (the caller accumulates).
 * A row whose d_gf is not finite (an instance whose step failed) contributes 0 to d_gw and gets NaN in its own d_gz row.
 * Products are exact fp32; the weight gradient is summed per workgroup and then in a fixed order (no atomics): two calls with the same
 * inputs are bit-identical.  Nothing of the engine's state is written.  The partial sums live in one workspace of the handle (allocated
 * by ndp_create, so the call may be captured into a graph): calls on one handle must be ordered against each other -- the same stream, or
 * streams ordered by events; two in flight at once would share the workspace.  -6: weights never set; -2 with a reason in ndp_last_error:
 * other_stride not 6 or 10, d_gf NULL, no output asked for. */
int ndp_downwash_vjp_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index,
                            const void *d_ego_ref, const void *d_ego_xy, const void *d_gf,
                            void *d_gz, void *d_gw, void *stream);
/* Forward mode of DownwashNN.update + the r_horiz gate: the Jacobian-vector product of the same network along n_tan directions per call,
 * the mirror of ndp_downwash_vjp_device and the producer of ndp_step_jvp_device's d_tf.  d_other / other_stride / d_other_index /
 * d_ego_ref / d_ego_xy as the step that produced the force took them; the forward is recomputed with the step's own arithmetic, so the
 * ReLU masks are those of the force the step used (capped ReLU: derivative 0 on both flat branches).  A direction is
 *   d_tz [B][T][N+1][6] fp64 : the direction of (other - ego_ref)[..., 0:6] per row (rounded to fp32 as d_gf is), NULL = 0
 *   d_tw [T][NDP_MLP_NPARAM] fp32 : the direction of the weights, blob order of ndp_set_mlp_weights, NULL = 0 (and none of its work runs)
 * with T = n_tan, not both NULL.  Outputs:
 *   d_df [B][T][N+1][3] fp64, required: the first-order change of the force, exactly ndp_step_jvp_device's d_tf layout (hand it over as
 *                             it lies); exactly 0 in every direction on closed / neighbour-less instances (the gate is held fixed)
 *   d_f_check [B][N+1][3] fp32, optional: the recomputed force, bit-equal to ndp_downwash_device's on open rows, 0 elsewhere.
 * The tangent is linear: nothing on its path is capped or converted to fp16, so any finite fp32 direction is served (no range limit on
 * d_tz or d_tw).  Products are exact fp32; W2 and W3 are read from the forward's fp16 pair image (hi + lo / 2^11: the weight to 2^-22).
 * T directions in one call give, bit for bit, what T calls with one direction each give; two calls are bit-identical.  No workspace of
 * the handle is used and nothing of the engine's state is written, so calls need no ordering against each other.
 * -1: NULL handle (or d_other / d_ego_ref missing); -6: weights never set; -2 with a reason in ndp_last_error, nothing launched:
 * other_stride not 6 or 10, n_tan outside 1..NDP_JVP_MAX_TANGENTS, no tangent given, d_df NULL. */
int ndp_downwash_jvp_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index,
                            const void *d_ego_ref, const void *d_ego_xy, int n_tan,
                            const void *d_tz, const void *d_tw, void *d_df, void *d_f_check, void *stream);
/* ndp_set_mlp_weights from device memory (d_blob: NDP_MLP_NPARAM fp32, the same order), enqueued on `stream`, no host synchronisation:
 * a training loop's update.  The device builds the same bytes as the host form.  This form does NOT check the values (that would take a
 * synchronisation): the range stated at ndp_set_mlp_weights is the caller's to keep -- a non-finite parameter or |W2|, |W3| >= 65520
 * (an fp16 infinity) gives NaN forces. */
int ndp_set_mlp_weights_device(ndp_handle *h, const void *d_blob, void *stream);
/* Test hook: host copies of the network's two device images, taken after a device synchronisation.
 *   frag_out  18432 32-bit words: the forward's fragment blob (fp32 values, then fp16 pairs -- compare it as words, not as floats)
 *   fragt_out 16384 floats: layers 2 and 3 transposed, the backward's records
 * Either may be NULL (skipped).  Returns -1 for a NULL handle. */
int ndp_debug_mlp_fragments(ndp_handle *h, void *frag_out, float *fragt_out);

/* Per-kernel timing with HIP events recorded on the stream each kernel is launched on:
 * on = n > 0 brackets every n-th launch of each kernel (n = 1: every launch), on = 0 stops and clears.
 * ndp_timing_read: name is "rti" or "mlp"; total over the bracketed launches.  Returns <0 if nothing was timed. */
int ndp_timing_enable(ndp_handle *h, int on);
int ndp_timing_read(ndp_handle *h, const char *name, double *total_ms, int64_t *launches);

/* ---- "next" row f3: the step after the path (hover-throttle estimator + actuator command), batched.
 * Replaces, per vehicle, HoverThrottleEstimator(ts).update(vz, throttle) -> k_throttle
 * (hv_throttle_est/hover_throttle_estimator.py:15-53, differentiator.py:10-23, params/estimator_params.py:13-18;
 *  called from nmpc_node.py:251-253) and nmpc_u_2_att_tgt's thrust = c * mass / k_throttle (nmpc_node.py:273-283).
 * One estimator per instance of the handle; state lives on the device.
 *   ndp_throttle_reset : x = [0, k_init], P = I, differentiator cleared
 *   ndp_throttle_update: vz[B], throttle[B] (the thrust command sent last tick) -> k_throttle[B]
 *   ndp_actuator_cmd   : u0[B][4] = [wx,wy,wz,c] -> cmd[B][4] = [wx,wy,wz, c*mass/k_throttle (0 if k == 0)] */
int ndp_throttle_reset(ndp_handle *h);
int ndp_throttle_update(ndp_handle *h, const double *vz, const double *throttle, double *k_throttle);
int ndp_throttle_update_device(ndp_handle *h, const void *d_vz, const void *d_throttle, void *d_k_throttle, void *stream);
int ndp_actuator_cmd(ndp_handle *h, const double *u0, const double *k_throttle, double *cmd);
int ndp_actuator_cmd_device(ndp_handle *h, const void *d_u0, const void *d_k_throttle, void *d_cmd, void *stream);
int ndp_throttle_get_state(ndp_handle *h, double *state /* [B][8]: x0 x1 P00 P01 P10 P11 vz_prev az_prev */);

/* ---- "next" row f2: the step beside the path -- the follower's reference relay (nmpc_follower_node.py:44-77).
 *   ndp_relay_formation: one formation_ref message per instance, form[B][3]; three AlphaFilters (alpha 0.8,
 *                        y0 = first message; hv_throttle_est/alpha_filter.py:11-20) -> filtered offset, kept on the device
 *   ndp_relay_reference: leader windows xr_lead[B][N+1][10] -> follower reference xr_out (x[:,0:3] += offset);
 *                        the leader's ur is used unchanged (:72-74), so it needs no copy
 *   ndp_relay_reset    : filters back to "no message seen" */
int ndp_relay_reset(ndp_handle *h);
int ndp_relay_formation(ndp_handle *h, const double *form, double *offset_out /* [B][3] or NULL */);
int ndp_relay_reference(ndp_handle *h, const double *xr_lead, double *xr_out);
int ndp_relay_reference_device(ndp_handle *h, const void *d_xr_lead, void *d_xr_out, void *stream);

/* ---- "next" row f1: the step before the path -- reference window generation, batched.
 * Replaces, per vehicle, NMPCRefPublisher.reset(traj_coeff, ros_t) + get_nmpc_pts(ros_t)
 * (pt_pub/pt_publisher.py:57-103): trajectory point from the piecewise polynomials (pt_pub/base_pt_publisher.py:81-133,
 * polym_optimizer.py:104-139), differential flatness (pt_publisher.py:188-248), x/u packing (:115-146), and the
 * 0.1 s node spacing of params/nmpc_params.py:40-43.  Past the end of the trajectory every node hovers at final_pt.
 *   ndp_ref_set_trajectory: the arrays of TrajCoefficients.msg for every instance, all with n_seg segments:
 *       coeff_x/y/z[B][n_seg*8] (minimum snap), coeff_yaw[B][n_seg*4] (minimum acceleration),
 *       time_cum[B][n_seg+1], time_seg[B][n_seg], final_pt[B][3]
 *   ndp_ref_window        : t[B] = trajectory time of node 0 ((ros_t - start_ros_t).to_sec()) ->
 *       xr[B][N+1][10], ur[B][N][4], node k at t + k*dt.  The device form writes buffers that ndp_step_device reads.
 *   Accuracy / range contract of the flatness map on the device: reciprocals and the thrust norm by hardware seeds + two Newton steps,
 *   sin / cos of the yaw by Cody-Waite reduction -- within a few 1e-16 of the Python publisher (held to 1e-12 by
 *   tests/test_ref_window_row.py), for FINITE yaw with |yaw| < 1e5 rad; a trajectory whose yaw polynomial leaves that range (or is
 *   not finite) is outside what these calls serve. */
int ndp_ref_set_trajectory(ndp_handle *h, int n_seg, const double *coeff_x, const double *coeff_y, const double *coeff_z,
                           const double *coeff_yaw, const double *time_cum, const double *time_seg, const double *final_pt);
int ndp_ref_window(ndp_handle *h, const double *t, double *xr, double *ur);
int ndp_ref_window_device(ndp_handle *h, const void *d_t, void *d_xr, void *d_ur, void *stream);

/* The reference's own bookkeeping of that window (NMPCRefPublisher, pt_pub/pt_publisher.py:36-103): a list of 5N+1 reference
 * points per vehicle, ts_nmpc apart; every control tick drops the oldest entry and appends the point at ros_t + T_horizon;
 * the controller's window is every 5th entry (params/nmpc_params.py:40-43).  Kept on the device as a ring per vehicle.
 *   ndp_ref_list_reset  : _gen_long_list_w_traj (:62-76) from the trajectory of ndp_ref_set_trajectory: points at
 *                         i*ts_nmpc, i = 0..5N-1, the first one duplicated in front
 *   ndp_ref_list_fix_pt : gen_fix_pt_ref (:40-55): every entry = x_odom[B][10], u = [0, 0, 0, mass*g] (quirk_b1 = 1: the
 *                         reference's value although u[3] is an acceleration) or [0, 0, 0, g] (quirk_b1 = 0)
 *   ndp_ref_list_window : t[B] = (ros_t - start_ros_t).to_sec(): get_nmpc_pts (:79-97) = pop, append the point at
 *                         t + T_horizon, return the window; t = NULL: get_nmpc_ref_from_long_list only (:99-103)
 *   *_device            : the two halves separately, on device buffers.  The list position is host state baked into each
 *                         launch's arguments: these calls must NOT be captured into a hipGraph (a replay would reuse the
 *                         position of the captured tick); ndp_ref_window_device has no such state and is capturable.
 * Device layout: phase-major, every entry stored twice, so that every window is contiguous (csrc/kern_args.hpp: RingGeom) -- the
 * stand-alone window call is a dense copy and ndp_tick's control step reads its windows in place. */
int ndp_ref_list_reset(ndp_handle *h);
int ndp_ref_list_fix_pt(ndp_handle *h, const double *x_odom, int quirk_b1);
int ndp_ref_list_window(ndp_handle *h, const double *t, double *xr, double *ur);
int ndp_ref_list_advance_device(ndp_handle *h, const void *d_t, void *stream);
int ndp_ref_list_window_device(ndp_handle *h, void *d_xr, void *d_ur, void *stream);

/* ---- The node's control tick, end to end on the device: odometry in, actuator command out, references resident.
 * Replaces, per vehicle and control period, ControllerNode.nmpc_callback + hover_throttle_callback (nmpc_node.py:211-231,251-253):
 *     nmpc_x_ref, nmpc_u_ref = ref_pub.get_nmpc_pts(now)        (:162; pt_pub/pt_publisher.py:78-103)   -- f1, the list on the device
 *     k_throttle = hv_th_estimator.update(vz, body_rate_cmd.thrust)   (:251-253)                         -- f3
 *     u0 = nmpc_ctl.update(x0, nmpc_x_ref, nmpc_u_ref[, disturb_force])   (:202-209,223-224)            -- a5 / a6, a7, a8
 *     body_rate_cmd = nmpc_u_2_att_tgt(*u0)                    (:225,273-283)                            -- f3
 * with the downwash force predicted from the NEIGHBOUR's window of the same tick (ndp_nmpc_leader_node.py:60-76; the neighbour
 * is another instance of this handle: its window is read out of its list, nothing is copied) and gated on the ego ODOMETRY xy
 * (:65-74).  Only what is new information crosses PCIe: 80 bytes of odometry per vehicle and tick (+ 8 each for t,
 * vz, throttle when given) in, 32 bytes of command (+ 4 status) out -- against 3.4 KB per vehicle for ndp_step's x0 + xr + ur +
 * neighbour columns.  ONE launch per tick at the reference configuration (N = 20, 1 RTI iteration): the control step's wave first
 * makes its vehicle's newest list entry -- node N of its window -- and the neighbour's, runs the estimator, reads the rest of both
 * windows straight out of the list (the phase-major layout makes every window contiguous), and writes the actuator command itself,
 * beside u0.  Other shapes: a small launch (tick_pre_kernel: list advance + estimator) in front of the control step.
 *   ndp_tick_config : other_index[B] = the instance whose window is vehicle i's neighbour (< 0: none, plain NMPC vehicle), or NULL
 *                     = no vehicle has one; gate_on_odometry = 1: the r_horiz gate of ndp_nmpc_leader_node.py:65-74, 0: always open.
 *                     Neighbours need use_fd = 1 and ndp_set_mlp_weights.
 *   ndp_tick_reset  : nmpc_ctl.reset(*ref_pub.get_nmpc_ref_from_long_list()) (nmpc_node.py:92,151-152): iterate := the list's
 *                     current window.  Call after ndp_ref_list_fix_pt (start-up) / ndp_ref_list_reset (a new trajectory).
 *   ndp_tick_begin  : x_odom[B][10] = odom_2_nmpc_x(px4_odom) of every vehicle; t[B] = (ros_t - start_ros_t).to_sec() -> the
 *                     list is advanced (get_nmpc_pts), or NULL -> the list stays (hover at the fixed point; a vehicle whose
 *                     trajectory has ended keeps being advanced: its points are final_pt); vz[B] or NULL = x_odom[:,5];
 *                     throttle[B] or NULL = the thrust this handle commanded on the previous tick (0 before the first).
 *                     flags bit 0: run the estimator this tick (the reference stops its timer while a trajectory is tracked,
 *                     nmpc_node.py:146,196); bit 1: ndp_tick_end will be asked for u0 as well; bit 2: NDP_TICK_T_UNIFORM.  Returns without waiting; at most two
 *                     ticks (or steps) in flight, drained in order, as with ndp_step_begin.
 *   ndp_tick_end    : waits for the oldest tick: cmd[B][4] = [wx, wy, wz, thrust]; u0[B][4], status[B], ipm_iters[B] or NULL.
 *                     Returns the worst status.
 *   ndp_tick        : begin + end under one lock.
 *   ndp_tick_device : the same launches on device pointers and a caller's stream; d_u0 may be NULL; status: ndp_get_status.
 *                     d_t: device-accessible [B] doubles -- EXCEPT with NDP_TICK_T_UNIFORM, where d_t is a HOST pointer to one double
 *                     that is read inside the call (before it returns), not by the device.
 *                     The list position is host state baked into the launches: not capturable into a hipGraph. */
/* The tick with neighbours on OTHER ranks / GPUs: their windows arrive through the caller's exchange (ndp_xchg_*, peer-mapped windows)
 * in d_windows[rows][N+1][stride] (stride 6: the position / velocity columns the gate and the network read; or 10); other_index[B] = the
 * row of every vehicle's neighbour (< 0: none).  A tick is then three enqueues on one stream, the exchange between them:
 *   ndp_tick_advance_device   : list advance (d_t as in ndp_tick_device; NULL: none) + estimator (flags bit 0) -- this rank's window
 *                               of the tick is complete (node N included);
 *   ndp_tick_window_pv_device : that window's columns [B][N+1][6] into the exchange's send buffer;      ... the exchange ...
 *   ndp_tick_step_device      : the control step against the exchanged windows + the actuator command.
 * Bit-equal with ndp_tick_device on the same vehicles in ONE handle.  ndp_tick_config switches back to neighbours of the same handle. */
int ndp_tick_config_remote(ndp_handle *h, const void *d_windows, int stride, int64_t rows, const int32_t *other_index, int gate_on_odometry);
int ndp_tick_advance_device(ndp_handle *h, const void *d_x_odom, const void *d_t, const void *d_vz, const void *d_throttle, int flags, void *stream);
int ndp_tick_window_pv_device(ndp_handle *h, void *d_pv, void *stream);
int ndp_tick_step_device(ndp_handle *h, const void *d_x_odom, void *d_cmd, void *d_u0, void *stream);
#define NDP_TICK_ESTIMATE 1
#define NDP_TICK_WANT_U0 2
#define NDP_TICK_T_UNIFORM 4   /* t points at ONE double (host memory, also for ndp_tick_device): the trajectory time of every vehicle
                                * (one host, one clock, the trajectories started together).  It travels in the kernel arguments: no
                                * vehicle's first load of the tick has to cross PCIe. */
int ndp_tick_config(ndp_handle *h, const int32_t *other_index, int gate_on_odometry);
int ndp_tick_reset(ndp_handle *h);
int ndp_tick_begin(ndp_handle *h, const double *x_odom, const double *t, const double *vz, const double *throttle, int flags);
int ndp_tick_end(ndp_handle *h, double *cmd, double *u0, int32_t *status_out, int32_t *ipm_iters_out);
int ndp_tick(ndp_handle *h, const double *x_odom, const double *t, const double *vz, const double *throttle, int flags,
             double *cmd, double *u0, int32_t *status_out, int32_t *ipm_iters_out);
int ndp_tick_device(ndp_handle *h, const void *d_x_odom, const void *d_t, const void *d_vz, const void *d_throttle, int flags,
                    void *d_cmd, void *d_u0, void *stream);

/* ---- "next" row f4: plant step for closed-loop rollouts on the device (dop_sim is absent from the reference).
 * x[B][10] in/out, u[B][4], f[B][3] force or NULL; RK4 with `substeps` over dt, quaternion renormalised. */
int ndp_plant_step(ndp_handle *h, double *x, const double *u, const double *f, double dt, int substeps);
int ndp_plant_step_device(ndp_handle *h, void *d_x, const void *d_u, const void *d_f, double dt, int substeps, void *stream);
/* Closed-loop rollout of every instance on the device (what nmpc_node.py's control timer + a simulator would do tick by
 * tick): reset at the trajectory's window at t0, then for k = 0..ticks-1: reference window at t0 + k*dt_tick
 * (ndp_ref_set_trajectory must have been called) -> control step from the plant state -> plant step with u0.
 * d_x[B][10] plant state in/out; d_log[ticks][B][10] receives the state after every tick, or NULL.  3 launches per tick
 * enqueued back to back on the stream; nothing returns to the host in between, nothing is synchronised. */
int ndp_rollout_device(ndp_handle *h, int ticks, double t0, double dt_tick, int substeps, void *d_x, void *d_log, void *stream);

/* ---- f4, the plant over a GIVEN input sequence, with reverse and forward mode: B vehicles simulated over `ticks` ticks of inputs and
 * forces in ONE launch (one lane per vehicle, the state in registers from the first tick to the last) instead of one ndp_plant_step_device
 * launch and one copy into a log per tick.  What shooting methods and system identification from logged flights call, and the link of the
 * closed loop the control step's and the downwash network's derivatives chain with.  Mass and gravity are the handle's (cfg).
 * ndp_plant_rollout_device:
 *   d_x0 [B][10] fp64                 the initial states
 *   d_u  [ticks][B][4] fp64           the inputs, one per tick
 *   d_f  [ticks][B][3] fp64 or NULL   the external forces, each HELD over its tick as ndp_plant_step_device holds it; NULL = none
 *   d_xs [ticks][B][10] fp64          receives the state after every tick
 *   Row k of d_xs is BIT-EQUAL to what k + 1 successive ndp_plant_step_device calls give with the same dt and substeps (RK4 with
 *   `substeps` over dt, the quaternion renormalised once per tick), with d_f and with NULL.  d_x0 may be any tick's slot of d_xs (a lane
 *   reads its own row first and writes its own rows only).  Nothing of the engine's state is written and nothing is allocated: the call can
 *   be captured into a graph, and calls need no ordering against each other.
 *   -1: NULL handle, d_x0, d_u or d_xs; -2 with a reason in ndp_last_error: ticks < 1, substeps outside 1..NDP_PLANT_MAX_SUBSTEPS.  A
 *   refused call enqueues nothing (so for the two calls below). */
#define NDP_PLANT_MAX_SUBSTEPS 16
int ndp_plant_rollout_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_u, const void *d_f,
                             void *d_xs, void *stream);
/* Reverse mode of the call above.  For L = sum over k of <d_gxs[k], xs[k]> it writes, each NULL = not computed, not all three NULL:
 *   d_gx0 [B][10] fp64         dL/dx0
 *   d_gu  [ticks][B][4] fp64   dL/du
 *   d_gf  [ticks][B][3] fp64   dL/df -- also with d_f NULL (the derivative at f = 0; bit-equal to the call with an all-zero d_f)
 * Inputs: d_x0, d_u, d_f as the forward took them; d_xs [ticks][B][10] the forward's log, required -- tick k restarts from xs[k-1] (x0 at
 * k = 0), the chain is never re-integrated from its start; d_gxs [ticks][B][10] fp64 the upstream gradient of every logged state,
 * required (a terminal-only loss passes zeros elsewhere).  Outputs are OVERWRITTEN and must not alias an input.
 * The derivative is that of the arithmetic performed: the RK4 stages with u and the force held over the tick, then q / |q| applied once per
 * tick to the un-normalised end state -- so a d_gxs[k] parallel to the quaternion of xs[k] moves nothing.  That end state and the substeps'
 * start states are recomputed from the tick's input state (O(substeps^2) substeps per tick, nothing stored).  One lane per vehicle, no
 * atomics, no workspace: two calls are bit-identical, an output does not depend on which others are asked for, and calls need no ordering
 * against each other.  -1: NULL handle, d_x0, d_u, d_xs or d_gxs; -2: as the forward call, or no output asked for. */
int ndp_plant_rollout_vjp_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_u, const void *d_f,
                                 const void *d_xs, const void *d_gxs, void *d_gx0, void *d_gu, void *d_gf, void *stream);
/* Forward mode of ndp_plant_rollout_device, T = n_tan directions (1..NDP_JVP_MAX_TANGENTS) in one call.  Directions, each NULL = 0, not
 * all three NULL:
 *   d_tx0 [B][T][10] fp64, d_tu [ticks][B][T][4] fp64, d_tf [ticks][B][T][3] fp64
 * Outputs:
 *   d_dxs [ticks][B][T][10] fp64, required: the first-order change of every logged state
 *   d_xs_check [ticks][B][10] fp64, optional: the recomputed primal, bit-equal to ndp_plant_rollout_device's log
 * No log is needed: the primal is carried along.  One lane per (vehicle, direction): T directions in one call give what T calls give, bit
 * for bit.  No atomics, no workspace, nothing of the engine's state written.  -1: NULL handle, d_x0 or d_u; -2: as the forward call,
 * n_tan out of range, no tangent given, d_dxs NULL. */
int ndp_plant_rollout_jvp_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_u, const void *d_f,
                                 int n_tan, const void *d_tx0, const void *d_tu, const void *d_tf, void *d_dxs, void *d_xs_check,
                                 void *stream);

/* ---- the closed loop over GIVEN reference windows and forces (the "ext" form), recorded, and its reverse mode: one call per direction
 * instead of a host loop of control steps, plant steps, tapes and their adjoints.  What tuning the controller's weights on a closed-loop
 * tracking loss, or shooting over x_0 and the references, calls.  Device pointers only.
 * ndp_closed_loop_device starts from the engine's current iterate and kept sets, as a loop of ndp_step_device calls would, and for
 * k = 0..ticks-1 runs the control step from the plant state (x_0, then xs[k-1]) with xr[k], ur[k], f[k] (u0 written straight into us[k]),
 * then the plant tick with us[k] and fp[k] (held over the tick) into xs[k].  Everything is enqueued on `stream`, nothing is synchronised.
 *   d_x0 [B][10] fp64; d_xr [ticks][B][N+1][10] fp64; d_ur [ticks][B][N][4] fp64
 *   d_f  [ticks][B][N+1][3] fp32  the force the controller sees, or NULL (needs use_fd = 1)
 *   d_fp [ticks][B][3] fp64       the force on the plant, or NULL
 *   d_xs [ticks][B][10] x_{k+1} and d_us [ticks][B][4] u0_k, required; d_Xs [ticks][B][N+1][10] the step's predicted states, or NULL;
 *   d_status int32 [ticks][B] the steps' status words, or NULL
 *   d_tape: ndp_closed_loop_tape_bytes(h, ticks) bytes, or NULL = not recorded.  Slot k (ticks slots of bytes / ticks each) holds what
 *   step k started from: X_lin [B][N+1][10] fp64 | U_lin [B][N][4] fp64 | act_lin [B][4N] int8 -- the three arrays ndp_step_vjp_device
 *   takes, as they lie.  The tape is the caller's; x0, xr, ur, f and fp are the caller's arrays and are not copied.
 * xs, us, Xs, the status words and the engine's iterate and kept sets afterwards are BIT-EQUAL to the loop of ndp_step_device (external
 * force) and ndp_plant_step_device.  Two launches per tick (the step; the link: plant tick, status, tape slot k+1, Xs[k]), one more for
 * slot 0; a step through the work list has its own three.
 *   -1: NULL handle, d_x0, d_xr, d_ur, d_xs or d_us.  -2 with a reason in ndp_last_error, nothing enqueued: ticks < 1, substeps outside
 *   1..NDP_PLANT_MAX_SUBSTEPS, d_f without use_fd, sensitivities on (as ndp_rollout_device).
 * ndp_closed_loop_vjp_device: reverse mode of that flight for L = sum_k <gxs[k], x_{k+1}> + <gus[k], u0_k> + <gXs[k], X_k> -- the PARTIAL
 * derivative every derivative here is: each tick's linearisation point (its tape slot) and final active set are held fixed.  Inputs as the
 * forward took them, its d_xs, d_us and d_tape (required); upstreams d_gxs [ticks][B][10], d_gus [ticks][B][4], d_gXs [ticks][B][N+1][10]
 * (NULL = 0, not all NULL); outputs, fp64, each NULL = not written, not all NULL: d_gx0 [B][10], d_gxr, d_gur as xr, ur, d_gf
 * [ticks][B][N+1][3], d_gfp [ticks][B][3], d_gmodel [B][16]; d_status_check int32 [ticks][B] (optional) the recomputed status words.
 * Tick by tick from the last, two launches each (the link; the step's adjoint kernel on the handle's workspace) and one behind tick 0:
 *   lambda = gxs[k] + (gx_p + gx0)            both of tick k + 1, added to each other first; nothing at the last tick
 *   (gx_p, gu_p, gfp[k]) = the plant tick's adjoint at (x_k, u0_k, fp_k) on lambda      (ndp_plant_rollout_vjp_device's arithmetic)
 *   (gx0, gxr[k], gur[k], gf[k]) = the step's adjoint on tape slot k with gu0 = gus[k] + gu_p and gX = gXs[k]
 *   d_gx0 = gx_p + gx0 of tick 0.
 * d_gmodel: one row per vehicle, no atomics, summed last tick first: columns 0..13 sum_k dL/dQd, dL/dRd of the step (ndp_step_vjp_model_device),
 * 14 the controller's mass share, 15 the PLANT's mass share -(1/m) sum_k <gfp[k], fp[k]> (exactly 0 with d_fp NULL).  The handle has one
 * mass: dL/dmass = column 14 + column 15.  Gravity is not differentiated.  With d_gmodel NULL the plain adjoint kernel runs; the other
 * outputs are bit-equal either way.  Gradients agree with chaining ndp_step_vjp_device and ndp_plant_rollout_vjp_device by hand to rounding
 * (the plant's adjoint may round differently in the last place from one kernel to the next); forward values are bit-equal.
 * The engine's iterate, kept sets, sensitivity buffers and the tape are never written; two calls are bit-identical; an output does not
 * depend on which others are asked for; the workspace is the handle's (first call).  A nonzero status in tick k of vehicle v gives NaN in
 * v's outputs of ticks <= k, in its d_gx0 and in its d_gmodel row; its later ticks and every other vehicle are unaffected, bit for bit.
 *   -1 and -2 as the forward; -2 also: the adjoint's own refusals (n_rti != 1, qp_precision != 0, N >= 28), no upstream, no output, d_tape NULL. */
int ndp_closed_loop_tape_bytes(ndp_handle *h, int ticks, size_t *bytes);
int ndp_closed_loop_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_xr, const void *d_ur,
                           const void *d_f, const void *d_fp, void *d_xs, void *d_us, void *d_Xs, void *d_status, void *d_tape, void *stream);
int ndp_closed_loop_vjp_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_xr, const void *d_ur,
                               const void *d_f, const void *d_fp, const void *d_xs, const void *d_us, const void *d_tape, const void *d_gxs,
                               const void *d_gus, const void *d_gXs, void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_gfp,
                               void *d_gmodel, void *d_status_check, void *stream);
/* ndp_closed_loop_jvp_device: forward mode of that flight, T = n_tan directions (1..NDP_JVP_MAX_TANGENTS) in one call -- the same PARTIAL
 * derivative: each tick's linearisation point (its tape slot) and final active set are held fixed.  Inputs as the forward took them, its
 * d_xs, d_us and d_tape (required).  Directions, fp64, each NULL = 0, not all five NULL:
 *   d_tx0 [B][T][10]; d_txr [ticks][B][T][N+1][10]; d_tur [ticks][B][T][N][4]; d_tf [ticks][B][T][N+1][3] (needs use_fd = 1; fp64 although
 *   d_f is fp32, as ndp_step_jvp_device takes it); d_tfp [ticks][B][T][3]
 * Outputs, fp64, OVERWRITTEN:
 *   d_dxs [ticks][B][T][10], required: the first-order change of x_{k+1};  d_dus [ticks][B][T][4], required: that of u0_k
 *   d_dXs [ticks][B][T][N+1][10], d_dUs [ticks][B][T][N][4], optional: those of the step's predicted states and inputs
 *   d_status_check int32 [ticks][B], optional: the recomputed status words
 * Nothing is repacked: dxs[k-1] is tick k's d_tx0 as ndp_step_jvp_device reads it, dus[k] is what that step writes as du0, and both are
 * the rows of the plant's tangent.  Tick by tick from the first, two launches each and one in front of tick 0 (tape slot 0 into the
 * workspace), everything on `stream`, nothing synchronised:
 *   (dus[k], dXs[k], dUs[k]) = the step's forward mode on tape slot k at x_k along (d_tx0 or dxs[k-1], txr[k], tur[k], tf[k])
 *   dxs[k] = the plant tick's tangent at (x_k, u0_k, fp_k) along (d_tx0 or dxs[k-1], dus[k], tfp[k])   (ndp_plant_rollout_jvp_device's
 *   arithmetic, one lane per (vehicle, direction), the lane recomputes the tick's primal); the same launch copies tape slot k + 1.
 * Tick 0's step is launched also when it receives no direction (only d_tfp given): its forward mode on four NULLs writes the zeros -- or a
 * failed vehicle's NaNs -- and the tick's status word.
 * The engine's iterate, kept sets, sensitivity buffers and the tape are never written.  The workspace is the handle's, shared with the
 * adjoint calls: calls on one handle are ordered.  Two calls are bit-identical; T directions in one call equal T one-direction calls bit for
 * bit; an output does not depend on which optional outputs are asked for.  dUs[k][.][.][0] is dus[k], bit for bit, and each step's outputs
 * are ndp_step_jvp_device's on the same slot and directions, bit for bit; dxs agrees with ndp_plant_rollout_jvp_device(ticks = 1) to
 * rounding (the plant's tangent may round differently in the last place from one kernel to the next).
 * A nonzero recomputed status in tick k of vehicle v gives NaN in v's rows of dxs and dus of every tick >= k, in every direction, and in its
 * dXs / dUs of tick k; its earlier ticks and every other vehicle are unaffected, bit for bit.  At a later tick whose own status is 0 the
 * step's forward mode runs on a NaN tx0: its dXs are NaN (stage 0 is tx0 as given, and every later stage inherits it through the
 * dynamics), its dUs are NaN in the free rows and exactly 0 in the rows its final set pins (the step writes a pinned row as 0 without
 * reading the sweep); the link makes dus[k] NaN either way.
 * Duality: <G, dxs> + <H, dus> + <A, dXs> = <gx0, tx0> + <gxr, txr> + <gur, tur> + <gf, tf> + <gfp, tfp> against
 * ndp_closed_loop_vjp_device's gradients for the upstreams G, H, A on the same record, to rounding.
 *   -1: NULL handle, d_x0, d_xr, d_ur, d_xs or d_us.  -2 with the call's name and a reason in ndp_last_error, nothing enqueued and no buffer
 *   touched: the forward's refusals, the derivative's own (n_rti != 1, qp_precision != 0, N >= 28), d_tape NULL, n_tan out of range, no
 *   direction given, d_tf or d_f without use_fd, d_dxs or d_dus NULL. */
int ndp_closed_loop_jvp_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_xr, const void *d_ur,
                               const void *d_f, const void *d_fp, const void *d_xs, const void *d_us, const void *d_tape, int n_tan,
                               const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf, const void *d_tfp, void *d_dxs,
                               void *d_dus, void *d_dXs, void *d_dUs, void *d_status_check, void *stream);
/* ndp_closed_loop_jvp_model_device: the same forward mode along directions of the model as well -- how the flight changes with the cost
 * weights and the mass, the transpose of ndp_closed_loop_vjp_device's d_gmodel.  ndp_closed_loop_jvp_device's arguments, plus
 *   d_tmodel [B][T][16] fp64, required: per vehicle and direction, constant over the ticks; columns 0..9 Qd', 10..13 Rd', 14 the
 *   CONTROLLER's mass', 15 the PLANT's mass'.  The handle has one mass: a direction of it goes into both columns; column 15 alone is a
 *   model mismatch of the plant.  The five data directions may all be NULL.
 * Per tick the step's forward mode is ndp_step_jvp_model_device's (rti_mjvp_kernel) along (tx, txr[k], tur[k], tf[k], tmodel), and the
 * plant tick's tangent is taken along tfp[k] - (tmodel[15] / m) fp_k: the plant sees the mass only as fp / m (with d_fp NULL column 15
 * moves nothing).  The same launches per tick, the same workspace, NaN rule and refusals (but for "no tangent"; -2 also: d_tmodel NULL).
 * Duality: <G, dxs> + <H, dus> + <A, dXs> = ndp_closed_loop_jvp_device's right side + sum_v <gmodel[v], tmodel[v]> (all 16 columns) against
 * ndp_closed_loop_vjp_device's d_gmodel on the same record, to rounding. */
int ndp_closed_loop_jvp_model_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_xr, const void *d_ur,
                                     const void *d_f, const void *d_fp, const void *d_xs, const void *d_us, const void *d_tape, int n_tan,
                                     const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf, const void *d_tfp,
                                     const void *d_tmodel, void *d_dxs, void *d_dus, void *d_dXs, void *d_dUs, void *d_status_check,
                                     void *stream);

/* ---- the closed loop of a FORMATION in one call per direction: ndp_closed_loop_device with the force on the plant made inside the loop
 * from the neighbours' actual states (ndp_plant_force_multi_device), and its reverse mode across the vehicles.  The controller keeps
 * seeing a given d_f (the "ext" form): the step and its derivative kernels run unchanged.  Device pointers only.
 * ndp_closed_loop_formation_config(h, other_index, K): other_index a HOST array int32 [B][K], 1 <= K <= NDP_MAX_NEIGH (else -2 with a
 *   reason); NULL clears the configuration (K not read).  Synchronous set-up, as ndp_tick_config: waits for the handle's work, then keeps
 *   on the handle a device copy of the index and its reverse lists offset int32 [B+1], edge int32 [offset[B]]: vehicle v's list
 *   edge[offset[v] .. offset[v+1]) holds e = w K + j for every slot with other_index[w][j] == v, in ascending e.  Empty slots (o < 0 or
 *   o >= B) and self slots (o == w: their two shares cancel exactly) are in no list.  The lists are built on the host.
 * ndp_plant_force_scatter_device(h, d_gz, d_gx, stream): ndp_plant_force_multi_vjp_device's g_z [B][K][6] fp64 (K the configured one) onto
 *   the states, d_gx [B][10] fp64, OVERWRITTEN.  One lane per vehicle, a gather, no atomics:
 *     d_gx[v][0:6] = (sum over v's list, in list order, of gz[e]) - (sum in slot order of gz[v K + j] over v's own slots that are neither
 *     empty nor self); each of the two sums starts from its first term as it is (an empty sum is +0), then one subtraction.
 *   Columns 6..9 are exactly 0.  -1: NULL handle, d_gz or d_gx; -2: nothing configured.
 * ndp_closed_loop_formation_device: ndp_closed_loop_device, except that the plant force is an OUTPUT log d_fps [ticks][B][3] fp64
 *   (required).  Per tick: fps[k] = ndp_plant_force_multi_device(x_k, the configured index, K, gate, plant_scale) from the states of that
 *   tick before any of them moves (ndp_rollout_formation_multi_device's rule); the step from x_k with xr[k], ur[k], f[k]; the link with
 *   fps[k] held over the tick.  Three launches per tick (the force, the step, the link), no new kernel.  Everything it writes -- xs, us,
 *   fps, Xs, the status words, the tape, the engine's iterate and kept sets -- is BIT-EQUAL to the host loop of
 *   ndp_plant_force_multi_device, ndp_step_device and ndp_plant_step_device.  The tape's layout and ndp_closed_loop_tape_bytes are those of
 *   ndp_closed_loop_device.  With every slot empty it is ndp_closed_loop_device with d_fp NULL, bit for bit, and fps is exact zeros.
 *   -1: NULL handle, d_x0, d_xr, d_ur, d_xs, d_us or d_fps.  -2, nothing enqueued: ndp_closed_loop_device's refusals, then nothing
 *   configured.  -6: ndp_set_mlp_weights was never called (as the force call).
 * ndp_closed_loop_formation_vjp_device: reverse mode of that flight for
 *     L = sum_k <gxs[k], x_{k+1}> + <gus[k], u0_k> + <gXs[k], X_k> + <gfps[k], fps[k]>
 *   -- ndp_closed_loop_vjp_device's PARTIAL derivative (linearisation points and final sets held fixed), the force's gates held fixed too
 *   (ndp_plant_force_multi_vjp_device).  Inputs as the forward took them, its d_xs, d_us, d_fps and d_tape (required); upstreams NULL = 0,
 *   not all four NULL; outputs each NULL = not written, not all NULL: d_gx0, d_gxr, d_gur, d_gf, d_gmodel as ndp_closed_loop_vjp_device's
 *   (column 15 of d_gmodel: -(1/m) sum_k <gfp_k, fps[k]> with gfp_k the plant's own share, without gfps[k]), d_gw [NDP_MLP_NPARAM] fp32,
 *   OVERWRITTEN: the gradient in the network's weights.  d_gfp is gone: its role is taken by d_gfps (upstream) and d_gw.
 *   Tick by tick from the last, four launches each (the link; the force's adjoint and, with d_gw, its reduction; the step's adjoint) and
 *   one behind tick 0:
 *     lambda = gxs[k] + ((gx_p + gx0) + gx_f)    the three of tick k + 1; gx_f = the gather of ndp_plant_force_scatter_device over tick
 *                                                k + 1's g_z, formed inside the link's launch; a vehicle that hears nobody and is heard by
 *                                                nobody adds no gx_f at all; nothing at the last tick
 *     (gx_p, gu_p, gfp_k) = the plant tick's adjoint at (x_k, u0_k, fps[k]) on lambda, gF_k = gfps[k] + gfp_k
 *     (g_z, g_w of the tick) = ndp_plant_force_multi_vjp_device at x_k on gF_k
 *     (gx0, gxr[k], gur[k], gf[k]) = the step's adjoint, as in ndp_closed_loop_vjp_device
 *     d_gx0 = (gx_p + gx0) + gx_f of tick 0.
 *   d_gw: the ticks' fp32 g_w are added into an fp64 accumulator, last tick first (the first as it is), by spare workgroups of the next
 *   link's launch; the tail launch rounds the sum once to fp32.  No atomics: two calls are bit-identical.
 *   With every slot empty every output is bit-equal to ndp_closed_loop_vjp_device with d_fp = zeros, and d_gw is exact zeros.
 *   The engine's iterate, kept sets and the tape are never written; an output does not depend on which others are asked for; the
 *   workspaces are the handle's (first call), shared with the other derivative calls: calls on one handle are ordered.
 *   Failed steps: a nonzero recomputed status in tick k of vehicle v gives NaN in v's outputs of ticks <= k, as in
 *   ndp_closed_loop_vjp_device; through the coupling the NaN then goes wherever the arithmetic carries it (v's g_z of tick k reaches its
 *   neighbours' lambda of tick k - 1).  A vehicle in a component of the index graph with no failed member is unaffected, bit for bit.
 *   A vehicle that hears a non-finite relative state (x[o] - x[v])[0:6] through an open slot flew under a meaningless force -- the
 *   network's ReLU swallows a NaN, so fps[k] may well be finite -- and its gF_k is made NaN.  d_gw leaves out the vehicles whose gF is
 *   not finite (the force adjoint's rule).  With the gate OFF a triple one of whose members has a NaN state at every tick therefore adds
 *   nothing to d_gw: it equals the call with that triple's upstreams zeroed.  With the gate ON this does NOT hold: a NaN position closes
 *   every slot that names the vehicle (the comparison is false), its neighbours fly on without hearing it, as in the forward, and keep
 *   feeding d_gw.  Per-tick chains of ndp_plant_force_multi_vjp_device do not have the rule: behind a failed vehicle their g_w keeps the
 *   rows of its neighbours' other slots, so the two routes' g_w differ there (and only there).  What a vehicle's ticks behind its last
 *   failed one gave stays in.  d_status_check tells.
 *   -1, -2, -6 as the forward; -2 also: the adjoint's own refusals, d_tape NULL, no upstream, no output. */
int ndp_closed_loop_formation_config(ndp_handle *h, const int32_t *other_index, int K);
int ndp_plant_force_scatter_device(ndp_handle *h, const void *d_gz, void *d_gx, void *stream);
int ndp_closed_loop_formation_device(ndp_handle *h, int ticks, double dt, int substeps, int gate, double plant_scale, const void *d_x0,
                                     const void *d_xr, const void *d_ur, const void *d_f, void *d_xs, void *d_us, void *d_fps, void *d_Xs,
                                     void *d_status, void *d_tape, void *stream);
int ndp_closed_loop_formation_vjp_device(ndp_handle *h, int ticks, double dt, int substeps, int gate, double plant_scale, const void *d_x0,
                                         const void *d_xr, const void *d_ur, const void *d_f, const void *d_xs, const void *d_us,
                                         const void *d_fps, const void *d_tape, const void *d_gxs, const void *d_gus, const void *d_gXs,
                                         const void *d_gfps, void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_gw, void *d_gmodel,
                                         void *d_status_check, void *stream);

/* ---- f4, the formation form (plant = a1 dynamics + downwash model): the downwash force the neighbour's ACTUAL state
 * puts on the ACTUAL vehicle, and the closed loop around it -- the experiment the downwash prediction is for (the reference has no
 * simulator; the force model is its own network, dnwash_nn_est/downwash_nn.py:22-28, behind the gate of ndp_nmpc_leader_node.py:65-68).
 * ndp_plant_force*: for vehicle v with o = other_index[v] the network at (x[o] - x[v])[0:6] (fp64 difference rounded to fp32, as
 *   ndp_downwash forms (other - ego_ref)[0:6]); the gate is o >= 0 && (!gate || |x[o].xy - x[v].xy|^2 < r_horiz^2), strict.  f[B][3] is
 *   fp64 (what ndp_plant_step reads) = scale * (double)net, bit-equal to ndp_downwash_device's value for the same six inputs, or exactly
 *   0 (gate closed; no neighbour: o < 0, o >= B, other_index NULL -- then no weights are needed).  d_xy[B][2] (or NULL) receives
 *   x[v][0:2]: the dense buffer ndp_step_device_ex takes as d_ego_xy.  One launch, one network row per vehicle; it reads x only. */
int ndp_plant_force_device(ndp_handle *h, const void *d_x, const void *d_other_index, int gate, double scale, void *d_f, void *d_xy,
                           void *stream);
int ndp_plant_force(ndp_handle *h, const double *x, const int32_t *other_index, int gate, double scale, double *f);
/* ndp_rollout_formation_device: ndp_rollout_device with the downwash acting on the plant.  Reset at the trajectory's window at t0, then
 *   per tick k: reference window at t0 + k*dt_tick -> plant force (scale plant_scale: the model-mismatch knob) + ego xy from the plant
 *   states -> control step -> plant step with that force.  The force is made from the states of one and the same tick, before any of them
 *   moves, and is HELD over the tick's plant call: it is not re-evaluated inside the RK4 substeps.
 *   The control step with NDP_FORM_COMPENSATE (needs use_fd = 1) is the fused step of ndp_step_device_ex: d_other = this tick's reference
 *   windows of the whole batch, d_other_index as given, d_ego_xy = the plant's xy when NDP_FORM_GATE is set -- the reference's own rule,
 *   the neighbour's window against the ego odometry.  Without it the step is the plain one (f = NULL) on a use_fd 0 or 1 handle: the
 *   paper's baseline, blind in the same downwash.  d_other_index NULL: nobody has a neighbour -- ndp_rollout_device's states, bit for bit.
 *   d_x[B][10] plant state in/out.  Each may be NULL: d_log[ticks][B][10] the state after every tick, d_log_u[ticks][B][4] u0,
 *   d_log_f[ticks][B][3] the plant force, d_worst_status int32[B] the largest status of each vehicle's steps.  Everything is enqueued on one
 *   stream; nothing returns to the host, nothing is synchronised.  -8 (nothing enqueued, the handle stays usable): NDP_FORM_COMPENSATE on
 *   a use_fd = 0 handle, no weights installed (and d_other_index given), no trajectory set.  With sensitivities on: -2, as
 *   ndp_rollout_device. */
int ndp_rollout_formation_device(ndp_handle *h, int ticks, double t0, double dt_tick, int substeps, const void *d_other_index, int flags,
                                 double plant_scale, void *d_x, void *d_log, void *d_log_u, void *d_log_f, void *d_worst_status, void *stream);
#define NDP_FORM_GATE        1   /* r_horiz gate in the plant force and in the controller's prediction */
#define NDP_FORM_COMPENSATE  2   /* the controller predicts the force (needs use_fd = 1); else it runs blind */

/* ---- Downwash from SEVERAL neighbours.  Every entry point above gives a vehicle one neighbour, as the reference does: its leader subscribes
 * to one neighbour's prediction (ndp_nmpc_leader_node.py:40), although its flagship is a formation of three (three_qd_ndp_nmpc.launch), where a
 * vehicle can fly under two others at once.  The calls below take other_index as int32[B][K], K slots per vehicle, 1 <= K <= NDP_MAX_NEIGH,
 * and SUPERPOSE the slots' forces.  Superposition is a modelling assumption: the network was trained on pairs (dnwash_nn_est/downwash_nn.py:
 * 22-28 sees one relative state).  The gate (ndp_nmpc_leader_node.py:65-68) is per slot, the same strict expression; a slot with index < 0 is
 * empty; the same index in two slots counts twice.  Slots are summed in slot order, the first open slot's value taken as it is, closed
 * slots adding nothing -- so K = 1 reproduces the single-neighbour call bit for bit, and any K equals the sum, in slot order, of K
 * single-neighbour results.  K outside 1..NDP_MAX_NEIGH: -2, nothing enqueued.  The fused step, the prefetch form and the tick stay
 * single-neighbour; the derivatives of the summed prediction are ndp_downwash_multi_vjp_device / ndp_downwash_multi_jvp_device below.
 * ndp_downwash_multi*: the controller's prediction, f_out[B][N+1][3] fp32 = sum over k (fp32) of ndp_downwash_device's value for neighbour
 *   other_index[i][k]: the network at (other - ego_ref)[0:6], slot k open iff index >= 0 and (ego_xy NULL or |other[o_k] node 0 xy -
 *   ego_xy[i]|^2 < r_horiz^2).  Device form: d_other [rows][N+1][other_stride] and other_stride (10 or 6, else -13) as ndp_step_device_ex;
 *   host form: other[B][N+1][10].  One launch; the weights are moved on chip once per workgroup and reused by the K slots.
 * ndp_plant_force_multi*: the force on the plant, f[v] = sum over k (fp64, products and sums individually rounded) of scale * (double)net(x[o_k]
 *   - x[v]) = the sum of K ndp_plant_force results; a slot with o < 0 or o >= B contributes exactly 0 and is never read; other_index NULL:
 *   nobody has a neighbour (zeros, no weights needed).  d_xy as ndp_plant_force_device. */
#define NDP_MAX_NEIGH 8
int ndp_downwash_multi_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index, int K, const void *d_ego_ref,
                              const void *d_ego_xy, void *d_f_out, void *stream);
int ndp_downwash_multi(ndp_handle *h, const double *other, const int32_t *other_index, int K, const double *ego_ref, const double *ego_xy,
                       float *f_out);
int ndp_plant_force_multi_device(ndp_handle *h, const void *d_x, const void *d_other_index, int K, int gate, double scale, void *d_f,
                                 void *d_xy, void *stream);
int ndp_plant_force_multi(ndp_handle *h, const double *x, const int32_t *other_index, int K, int gate, double scale, double *f);
/* ndp_rollout_formation_multi_device: ndp_rollout_formation_device with d_other_index int32[B][K].  Per tick k: reference window at t0 +
 *   k*dt_tick -> the summed plant force (ndp_plant_force_multi_device at plant_scale, which also writes the ego xy) -> with NDP_FORM_COMPENSATE
 *   the summed prediction (ndp_downwash_multi_device: d_other = d_ego_ref = this tick's reference windows of the whole batch, d_ego_xy = the
 *   plant's xy when NDP_FORM_GATE is set) into the handle's force buffer and the control step with that force as d_f (ndp_step_device's
 *   external-force step); without it the plain step -> plant step with the plant force.  Logs and -8 / -2 refusals as
 *   ndp_rollout_formation_device, and -2 for K outside 1..NDP_MAX_NEIGH (checked even when d_other_index is NULL: pass 1); d_other_index
 *   NULL: ndp_rollout_device's states.  One stream, nothing is synchronised. */
int ndp_rollout_formation_multi_device(ndp_handle *h, int ticks, double t0, double dt_tick, int substeps, const void *d_other_index, int K,
                                       int flags, double plant_scale, void *d_x, void *d_log, void *d_log_u, void *d_log_f,
                                       void *d_worst_status, void *stream);
/* Reverse mode of ndp_downwash_multi_device as that call evaluates the force: ndp_downwash_vjp_device with d_other_index int32[B][K]
 * (required).  The per-slot rules are the forward's: each slot behind its own gate (the same strict expression), index < 0 = empty, the same
 * index in two slots counts twice, other_stride 6 or 10, d_ego_xy NULL = open.  d_gf [B][N+1][3] fp64 is the gradient of the SUMMED force and
 * is shared by the K slots of a row.  Every slot's forward is recomputed with the step's own arithmetic (its ReLU masks are the forward's).
 * One launch over the B K (N+1) virtual rows (instance, slot, node): a 32-row tile with no open row -- a closed or empty slot's -- costs its
 * gate only.  Outputs, each NULL = not computed, not both NULL:
 *   d_gz [B][K][N+1][6] fp64 : per slot; d_gz[i][k] is bit-equal to what ndp_downwash_vjp_device writes for other_index[:, k] -- 0 on closed
 *                               and empty slots, NaN on the open slots of a row whose d_gf is not finite
 *   d_gw [NDP_MLP_NPARAM] fp32, OVERWRITTEN: the sum over all (row, slot), accumulated in registers across the launch, one partial-sum pass
 *                               and one fixed-order reduction, no atomics: two calls are bit-identical.  A row whose d_gf is not finite adds
 *                               nothing: the result is bit-equal to the call with that row's d_gf zeroed.  NOT promised bit-equal to the sum
 *                               of K ndp_downwash_vjp_device results (the order of summation differs).
 * At K = 1 both outputs are bit-equal to ndp_downwash_vjp_device's.  Nothing of the engine's state is written.  The partial sums use the
 * SAME workspace as ndp_downwash_vjp_device (allocated by ndp_create, so the call may be captured into a graph; its size caps the
 * workgroups, the rest is a grid-stride loop): calls of either kind on one handle must be ordered against each other -- the same stream, or
 * streams ordered by events.  -1: NULL handle (or d_other / d_ego_ref missing); -6: weights never set; -2 with a reason in ndp_last_error,
 * nothing launched: K outside 1..NDP_MAX_NEIGH, d_other_index NULL, other_stride not 6 or 10, d_gf NULL, no output asked for. */
int ndp_downwash_multi_vjp_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index, int K,
                                  const void *d_ego_ref, const void *d_ego_xy, const void *d_gf, void *d_gz, void *d_gw, void *stream);
/* Forward mode of ndp_downwash_multi_device: ndp_downwash_jvp_device with d_other_index int32[B][K] (required), the mirror of the call
 * above.  Directions, T = n_tan, not both NULL:
 *   d_tz [B][T][K][N+1][6] fp64 : per slot, the direction of (other[o_k] - ego_ref)[..., 0:6], NULL = 0
 *   d_tw [T][NDP_MLP_NPARAM] fp32 : the direction of the weights (shared by the slots), NULL = 0
 * Outputs:
 *   d_df [B][T][N+1][3] fp64, required: the fp64 sum IN SLOT ORDER of the slots' (double) tangents, the first open slot's value taken as it
 *                             is, closed slots adding nothing: bit-equal to that sum of K ndp_downwash_jvp_device results (d_tz[:, :, k],
 *                             the same d_tw); exactly 0 where no slot is open.  The lane that owns a row accumulates it in d_df itself.
 *   d_f_check [B][N+1][3] fp32, optional: the recomputed summed force, bit-equal to ndp_downwash_multi_device's output.
 * T directions in one call give what T calls give, bit for bit; K = 1 is bit-equal to ndp_downwash_jvp_device.  No atomics, no workspace,
 * nothing of the engine's state written: calls need no ordering against each other.  Refusals as above, and -2 for n_tan outside
 * 1..NDP_JVP_MAX_TANGENTS, no tangent given, d_df NULL. */
int ndp_downwash_multi_jvp_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index, int K,
                                  const void *d_ego_ref, const void *d_ego_xy, int n_tan, const void *d_tz, const void *d_tw, void *d_df,
                                  void *d_f_check, void *stream);

/* ---- The derivatives of the downwash force ON THE PLANT (ndp_plant_force_device / ndp_plant_force_multi_device): the link between the
 * vehicles' actual states and the force f that ndp_plant_step_device / ndp_plant_rollout_device take as an input, whose gradient d_gf those
 * calls return.  The derivative is that of the arithmetic ndp_plant_force_multi_device performs: per slot z = fp32 of the fp64 difference
 * (x[o] - x[v])[0:6], the network, scale * (double)net, summed in fp64 in slot order.  The rounding of z to fp32 counts as the identity; the
 * gate (strict, per slot, the forward's expression) is piecewise constant and contributes nothing; the ReLU masks are the forward's,
 * recomputed with the step's own arithmetic.  d_x [B][10] fp64; d_other_index int32[B] (single forms) or [B][K] (multi forms, K outside
 * 1..NDP_MAX_NEIGH: -2); a slot with o < 0 or o >= B is empty and never read; d_other_index NULL: nobody has a neighbour -- exact zeros in
 * every output, no network pass, no weights needed.  The single-neighbour forms are the K = 1 case, bit for bit.
 *
 * Reverse mode.  d_gf [B][3] fp64 (required) is the gradient of the SUMMED force, shared by a vehicle's K slots; each open slot's upstream is
 * fp32(scale * d_gf[v][c]), the product formed in fp64 and rounded once.  Outputs, each NULL = not computed, not both NULL:
 *   d_gz [B][K][6] fp64 : the gradient per NETWORK INPUT ROW (as ndp_downwash*_vjp_device return it), 0 on closed and empty slots.  The
 *                         scatter onto the states is the caller's: + d_gz[v][k] to x[o_k][0:6], - d_gz[v][k] to x[v][0:6] (torch:
 *                         plant_force does it).  With windows other[o][n] = x[o], ego_ref[v][n] = x[v], ego_xy = x[v][0:2] and the upstream
 *                         scale * d_gf[v] at node 0, d_gz[v][k] is bit-equal to node 0 of ndp_downwash_multi_vjp_device's d_gz.
 *   d_gw [NDP_MLP_NPARAM] fp32, OVERWRITTEN: accumulated in registers across the launch, one partial-sum pass and one fixed-order
 *                         reduction, no atomics: two calls are bit-identical.
 * A vehicle whose d_gf row is not finite adds nothing to d_gw and has NaN in the d_gz of its open slots; so does a slot whose six inputs
 * are not all finite.  Nothing of the engine's state is written.  The partial sums use the SAME workspace as ndp_downwash_vjp_device (its
 * size caps the workgroups, the rest is a grid-stride loop): calls of these kinds on one handle must be ordered against each other -- the
 * same stream, or streams ordered by events.
 *
 * Forward mode, T = n_tan directions (1..NDP_JVP_MAX_TANGENTS), not both NULL:
 *   d_tx [B][T][10] fp64 : directions of the STATES.  The kernel gathers: a slot's input direction is the fp64 difference tx[o][t][i] -
 *                          tx[v][t][i], i < 6, then handled as ndp_downwash_multi_jvp_device handles its d_tz -- no scatter is needed.
 *   d_tw [T][NDP_MLP_NPARAM] fp32 : directions of the weights.
 * Outputs:
 *   d_df [B][T][3] fp64, required: the fp64 sum in slot order of scale * (double)tangent, the product and each sum individually rounded, the
 *                          first open slot's value taken as it is; exactly 0 where no slot is open.
 *   d_f_check [B][3] fp64, optional: the recomputed force, bit-equal to ndp_plant_force_multi_device's.
 * T directions in one call equal T calls bit for bit.  No atomics, no workspace, nothing of the engine's state written.
 *
 * -1: NULL handle or d_x; -6: weights never set and an index given; -2 with a reason in ndp_last_error, nothing enqueued, outputs untouched:
 * K outside 1..NDP_MAX_NEIGH, d_gf NULL, no output asked for, n_tan out of range, no tangent given, d_df NULL. */
int ndp_plant_force_vjp_device(ndp_handle *h, const void *d_x, const void *d_other_index, int gate, double scale, const void *d_gf,
                               void *d_gz, void *d_gw, void *stream);
int ndp_plant_force_multi_vjp_device(ndp_handle *h, const void *d_x, const void *d_other_index, int K, int gate, double scale,
                                     const void *d_gf, void *d_gz, void *d_gw, void *stream);
int ndp_plant_force_jvp_device(ndp_handle *h, const void *d_x, const void *d_other_index, int gate, double scale, int n_tan,
                               const void *d_tx, const void *d_tw, void *d_df, void *d_f_check, void *stream);
int ndp_plant_force_multi_jvp_device(ndp_handle *h, const void *d_x, const void *d_other_index, int K, int gate, double scale, int n_tan,
                                     const void *d_tx, const void *d_tw, void *d_df, void *d_f_check, void *stream);

/* ---- Training the downwash network on the device (nn_train.py:129-157 with --SN): one full-batch Adam step followed by the spectral-norm
 * cap on every weight matrix, in ONE launch of four workgroups (one per layer) behind the weight gradient of ndp_downwash_vjp_device /
 * ndp_downwash_multi_vjp_device.  No host value changes between two steps (the step counter lives in device memory), so steps can be
 * enqueued back to back or captured into a graph.
 *
 * ndp_mlp_spectral_norms_device: d_sigma[l] (fp64 [4]) = the largest singular value of the weight matrix of layer l + 1 of d_w (fp32
 *   [NDP_MLP_NPARAM], blob order of ndp_set_mlp_weights; biases are not part of it).  Per layer: the Gram matrix on the smaller side (6x6,
 *   64x64, 64x64, 3x3) in fp64 on the f64 matrix instruction (products of fp32 values are exact there), Householder tridiagonalisation in
 *   LDS, then 8 rounds of 256-way multisection on Sturm counts from a Gershgorin bound: a direct method whose accuracy does not depend on
 *   the gaps between singular values (relative error of the order of 64 x 2^-53), every loop with a compile-time trip count.  An all-zero
 *   matrix gives exactly 0.  The handle's weights are not read or written.
 * ndp_mlp_spectral_norms: the same for a host blob; synchronises.
 * ndp_mlp_adam_sn_device: one optimiser step.  d_w, d_m, d_v fp32 [NDP_MLP_NPARAM] (parameters and Adam's two moments, updated in place),
 *   d_g fp32 [NDP_MLP_NPARAM] (the gradient, exactly what the VJP calls write as d_gw), d_step int64 [1] (steps taken so far).  All-zero
 *   d_m, d_v, d_step are a fresh optimiser.  With t = step + 1, torch.optim.Adam's defaults (no weight decay, no amsgrad):
 *       m = beta1 m + (1 - beta1) g,  v = beta2 v + (1 - beta2) g^2,  p = p - lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *   in fp64 from the fp32 inputs, every operation rounded on its own (no fused multiply-add); m, v and p are each rounded to fp32 once, in
 *   that order, and the p update reads the STORED m and v: a step is a pure function of the stored state.  fp32 subnormals are kept.  Then, per layer, sigma of the updated weight matrix as above and,
 *   if sn_cap > 0 and sigma > sn_cap, every weight of the layer becomes fp32(w * (sn_cap / sigma)), factor and product in fp64 (the
 *   reference's fp32 `param / s * SN` rounds twice: at most 1.5 ulp apart).  Biases are never scaled (nn_train.py:153).  sn_cap <= 0: no
 *   layer is scaled.
 *   Non-finite gradient: if any of the NDP_MLP_NPARAM values of d_g is NaN or infinite the call changes nothing -- d_w, d_m, d_v and
 *   d_step stay bit for bit -- and d_info[0] = 1 (every workgroup scans the whole gradient and decides alike).
 *   d_step is advanced by the kernel, once per step that was not skipped: every workgroup reads it at entry and the last one to finish
 *   (an agent-scope ticket in a workspace of the handle, which that workgroup resets) writes step + 1.
 *   d_sigma fp64 [4], NULL allowed: the norms AFTER the call -- of a layer that was scaled, the norm of the scaled (rounded) matrix,
 *     computed again; after a skipped step, the norms of the unchanged weights.
 *   d_info int32 [4], NULL allowed: [0] 1 if the step was skipped, else 0; [1] bitmask of the layers that were scaled (bit l = layer l + 1);
 *     [2], [3] reserved, written as 0.
 *   install != 0: behind the update, on the same stream, what ndp_set_mlp_weights_device(h, d_w, stream) does -- also after a skipped step.
 *   The ticket lives in one workspace of the handle (allocated by ndp_create, so the call may be captured): calls on one handle must be
 *   ordered against each other -- the same stream, or streams ordered by events.
 *   -1: NULL handle or a NULL required pointer (d_w, d_g, d_m, d_v, d_step); -2 with a reason in ndp_last_error: lr not finite, a beta
 *   outside [0, 1), eps <= 0 (or NaN), sn_cap NaN.  Nothing is launched on -1 or -2. */
int ndp_mlp_spectral_norms_device(ndp_handle *h, const void *d_w, void *d_sigma, void *stream);
int ndp_mlp_spectral_norms(ndp_handle *h, const float *blob, double *sigma4);
int ndp_mlp_adam_sn_device(ndp_handle *h, void *d_w, const void *d_g, void *d_m, void *d_v, void *d_step, double lr, double beta1,
                           double beta2, double eps, double sn_cap, void *d_sigma, void *d_info, int install, void *stream);

/* ---- The network on sample rows, and its fit (nn_train.py:99-108,131,142-147: x_train [n,6], y_train [n,3] cast to float32, nn.MSELoss,
 * loss.backward(); nn_test.py / plot_pred_one_line: the network on plain grid rows).  No window, no gate, no engine batch shape: the data
 * set is whatever the caller holds in device memory.
 *   d_z [R][6] fp32 : the network's input rows, the caller's (other - ego)[0:6] already in float32;  d_y [R][3] fp32 : the labels;
 *   d_rw [R] fp32   : per-row weights, NULL = every weight 1;
 *   d_index int32 [M] : output / batch row m uses data row index[m]; NULL = index[m] = m (then M <= R).  An index < 0 or >= R is an EMPTY
 *     slot: never read, contributes nothing, its d_f row is exactly 0.  An index listed twice counts twice.  Fixed-size mini-batches pad
 *     their tail with -1.
 * The weights are the installed ones (ndp_set_mlp_weights / _device).
 * ndp_mlp_rows_device: d_f [M][3] fp32 = the network's output, each row bit-equal to what ndp_downwash_device returns for the same six
 *   fp32 inputs (a row with a non-finite input: NaN).
 * ndp_mlp_fit_rows_device: with e = f - y in fp32 (one rounding per component),
 *   d_loss fp64 [1] = scale * sum_m rw (e0^2 + e1^2 + e2^2): each square exact in fp64, products with rw and scale and all sums in fp64
 *     (scale = 1 / (3 n) gives nn.MSELoss).  Each workgroup writes a partial sum to a workspace; a reduce in fixed order writes d_loss.
 *   d_gw fp32 [NDP_MLP_NPARAM], blob order, OVERWRITTEN = d loss / d weights: the backward pass of ndp_downwash_vjp_device (the forward
 *     recomputed once in the kernel, its own ReLU masks, the capped ReLU's derivative 0 on both flat branches, exact fp32 products) with
 *     the upstream d4[c] = fp32(2 scale rw e[c]), the factor formed in fp64 and rounded once.  Per-workgroup partials, a fixed-order reduce,
 *     no atomics: two calls give identical bits.  NULL: loss only, none of the backward pass runs.
 *   d_f fp32 [M][3], NULL allowed: the prediction the loss was formed from.
 *   d_info int32 [2], NULL allowed: rows used, rows skipped.  A row is skipped when its z, y, rw, prediction or residual is not finite: it
 *     contributes nothing to the loss or to d_gw.  Every other non-empty row is used (a row with rw = 0 too).  Empty slots are neither.
 *   groups: the number of workgroups (128 rows each per round, a grid-stride loop covers the rest); 0 = the library's choice,
 *     min(ceil(M / 128), NDP_FIT_MAX_GROUPS); 1..NDP_FIT_MAX_GROUPS forces that count.  It changes results through summation order only.
 * The partials live in a workspace of the handle of their own (allocated by ndp_create, so the calls may be captured): fit calls on one
 * handle must be ordered against each other.  Nothing else of the handle is written.
 * -1: NULL handle, d_z NULL, d_y NULL (fit); -6: weights never set; -2 with a reason in ndp_last_error and nothing launched: R < 1, M < 1,
 * R or M >= 2^31, d_index NULL with M > R, groups outside 0..NDP_FIT_MAX_GROUPS, d_loss, d_gw and d_f all NULL (fit), d_f NULL (rows). */
#define NDP_FIT_MAX_GROUPS 256
int ndp_mlp_rows_device(ndp_handle *h, const void *d_z, const void *d_index, int64_t R, int64_t M, void *d_f, void *stream);
int ndp_mlp_fit_rows_device(ndp_handle *h, const void *d_z, const void *d_y, const void *d_rw, const void *d_index, int64_t R, int64_t M,
                            double scale, int groups, void *d_loss, void *d_gw, void *d_f, void *d_info, void *stream);

/* ---- Peer windows: the neighbour exchange across GPUs as publish / subscribe over xGMI.
 * Replaces the PredXU topic between processes: the publisher is nmpc_node.py:116-133,229-230 (`nmpc_x_ref`, 21x10 float64, a NEW
 * message every control tick), the subscriber ndp_nmpc_leader_node.py:40,60-76 (consumes the latest one).  One process per GPU:
 * the publisher allocates its window buffer with ndp_peer_alloc and sends the 64-byte handle to the subscriber's process once
 * (any channel: torch.distributed object collectives, a socket); the subscriber maps it with ndp_peer_open.  Every control tick
 * each rank then calls ndp_peer_publish_device in front of its control-step launch (a copy launch + a one-wave launch): it writes
 * this tick's windows into one of the two slots of its own buffer, publishes the tick number (an epoch word, system scope) and
 * waits for the neighbour's epoch of the same tick; the control-step kernel launched next reads the neighbour's slot straight out of the
 * publisher's HBM (peer access over xGMI) -- no collective, no host round trip.  Writer -> reader ordering, slot reuse (the
 * reader's acknowledgement), bounded waits and their counters: csrc/peer_epoch.hpp.
 *   ndp_peer_layout : bytes of a buffer whose slots hold n_doubles each ([B][N+1][10] windows: n = B*(N+1)*10), the offset
 *                     of slot 0 and the slot stride (bytes).  The first 512 bytes are protocol words.
 *   ndp_peer_alloc  : zeroed device memory on `device` -> *ptr and its IPC handle (64 bytes).  Fine-grained (coherent between
 *                     agents while kernels run); ordinary device memory if the runtime refuses or NDP_PEER_COARSE=1 is set.
 *   ndp_peer_open   : maps another process's buffer into this process for use on `device` -> *ptr.  The mapped range is
 *                     remembered: neighbour windows (`other`) that lie inside it are read with system-scope loads by every
 *                     kernel of this library, so that they are fetched from the owner's memory, not from a stale cache line.
 *   ndp_peer_publish_device : the per-tick launch described above.  d_src: this rank's windows of the tick (n_doubles, device
 *                     memory); own_buf / nb_buf: this rank's buffer and the mapped neighbour buffer (the same pointer with one
 *                     rank); slot = parity of the tick (first tick = 1 -> slot 1, then alternating): the slot whose address
 *                     the caller hands to the control step as `other` (a mismatch with the device-side tick is counted);
 *                     timeout_us bounds each wait.  Capturable into a hipGraph (an even number of ticks per graph).
 *   ndp_peer_stats  : synchronises `device`; out4 = {ticks published, reader-acknowledgement timeouts, neighbour-epoch
 *                     timeouts (the slot was read as it was: stale), slot-parity mismatches}.
 *   ndp_peer_close / ndp_peer_free: undo open / alloc (the mapping keeps the memory alive: a reader whose publisher has
 *                     exited goes on reading the last published windows and counts epoch timeouts).
 * All return 0 or a negative error code. */
int ndp_peer_layout(size_t n_doubles, size_t *buffer_bytes, size_t *slot0_offset, size_t *slot_stride);
int ndp_peer_alloc(int device, size_t bytes, void **ptr, unsigned char *handle64);
int ndp_peer_open(int device, const unsigned char *handle64, void **ptr);
int ndp_peer_publish_device(int device, const void *d_src, size_t n_doubles, void *own_buf, void *nb_buf, int slot,
                            unsigned timeout_us, void *stream);
int ndp_peer_stats(int device, const void *own_buf, unsigned long long *out4);
int ndp_peer_close(int device, void *ptr);
int ndp_peer_free(int device, void *ptr);

/* ---- The neighbour exchange as ONE RCCL all-gather per control tick, issued by the library on a HIP stream of its own.
 * Replaces the same PredXU traffic (nmpc_node.py:116-133,229-230 -> ndp_nmpc_leader_node.py:40,60-76) with the collective the
 * build contract names: every rank contributes the position / velocity columns of its windows ([B_local][N+1][6] fp64, all the
 * gate and the network read, downwash_nn.py:22), every rank receives all of them ([world * B_local][N+1][6]; rank r's leaders
 * read the rows of rank (r+1) % world, or the rows other_index names).  RCCL is bound at run time (rccl_path: the librccl the
 * process already holds, e.g. torch's -- NULL or "" = the loader's search path); one process per GPU, one ndp_xchg per process.
 *   ndp_xchg_unique_id : rank 0 draws the communicator's id (128 bytes) and hands it to the others (any channel)
 *   ndp_xchg_create    : collective -- every rank calls it with the same id; creates the communicator, the exchange stream
 *                        (its own hardware queue) and two events
 *   ndp_xchg_begin     : packs this rank's d_xr ([rows][10] doubles, rows = B_local * (N+1)) and starts the all-gather into
 *                        d_gathered on the exchange stream, ordered behind everything `after_stream` holds so far (NULL: no
 *                        such ordering) and behind `after_event` (NULL: none; e.g. ndp_last_step_event: the last reader of
 *                        d_gathered); returns at once.  The windows are trajectory-generator output (functions of time): the gather of tick i+1 is
 *                        started before tick i's control step is launched and runs beside it (two gathered buffers).
 *   ndp_xchg_end       : `stream` waits on the device for the gather started last; the control step launched next on `stream`
 *                        may read d_gathered.  No host synchronisation anywhere; begin / end / step are capturable together
 *                        (the FIRST ndp_xchg_begin of a given size allocates the send buffer: call it once outside a capture).
 * All return 0 or a negative error code (-20 / -21: RCCL not found / symbols missing, -22: an RCCL call failed, see
 * ndp_xchg_last_error). */
typedef struct ndp_xchg ndp_xchg;
int ndp_xchg_unique_id(const char *rccl_path, unsigned char *id128);
int ndp_xchg_create(int device, int rank, int world, const unsigned char *id128, const char *rccl_path, ndp_xchg **out);
int ndp_xchg_begin(ndp_xchg *x, const void *d_xr, size_t rows, void *d_gathered, void *after_stream, void *after_event);
/* Ordering another stream behind a control step without a packet on the step's own stream: with ndp_track_steps(h, 1) the
 * completion of every control step launched for h marks an event through the dispatch packet's own completion signal
 * (hipExtLaunchKernel); ndp_last_step_event returns the event of the step launched last (valid until four more have been
 * launched).  Typical use: the all-gather of tick i+2 overwrites the gathered buffer tick i read -- it is begun behind tick i's
 * step with ndp_xchg_begin(..., NULL, that event).  (An event recorded on the compute stream instead costs two command-processor
 * packets between consecutive control steps: 38 against 29 us per tick at batch 1024.)  Tracked steps are not graph-capturable. */
int ndp_track_steps(ndp_handle *h, int on);
int ndp_last_step_event(ndp_handle *h, void **event);
int ndp_xchg_end(ndp_xchg *x, void *stream);
/* The two calls of one tick of the pipelined form in one: ndp_xchg_end(x, stream) for the gather begun last (this tick's windows), then
 * ndp_xchg_begin of the NEXT tick's windows behind the last reader of d_gathered_next -- the completion event of the control step
 * launched last for h when its steps are tracked, else (h NULL, or not tracked) everything `stream` holds so far. */
int ndp_xchg_tick(ndp_xchg *x, ndp_handle *h, void *stream, const void *d_xr_next, size_t rows, void *d_gathered_next);
/* ndp_tick with neighbours on other ranks (ndp_tick_config_remote): stage 2 and the exchange in one call -- this tick's window columns
 * of h's reference list packed into the exchange's send buffer and all-gathered into d_gathered ([world * B][N+1][6] doubles, the
 * buffer ndp_tick_config_remote was given), both on `stream` (NULL: the handle's), i.e. behind ndp_tick_advance_device and in front of
 * ndp_tick_step_device by stream order alone.  Replaces, on the reference's side, the publish of PredXU per control period
 * (nmpc_node.py:229-230) and its subscription in the neighbour's node (ndp_nmpc_leader_node.py:40,60-76). */
int ndp_xchg_tick_windows(ndp_xchg *x, ndp_handle *h, void *d_gathered, void *stream);
/* The same tick with the exchange AHEAD of the control steps: a window is a function of time alone, so the list advance of a later tick,
 * its window columns and their all-gather run on the exchange's own stream BESIDE the control steps, into one of TWO or THREE gather
 * buffers the caller cycles through (each [world * B][N+1][6]; ndp_tick_config_remote names any: the step is told which one it reads).
 * Begins and steps pair up in order (step k reads what begin k gathered); at most two begins may be ahead.  Per period, two buffers:
 *     ndp_xchg_tick_step (tick i: estimator if NDP_TICK_ESTIMATE, device-side wait for gather i, control step + command on `stream`)
 *     ndp_xchg_tick_begin(tick i+1: d_t / flags as ndp_tick_advance_device takes them -- THAT period's trajectory time; NULL: no advance)
 * with one begin in front of the first step; three buffers: step(i) then begin(i+2), two begins in front -- the gather then fills a
 * buffer whose last reader is long over and never waits for a control step (38.3 against 34.9 M solves/s on one rank).  Ordering is the library's (events on the device, nothing waits on the host);
 * with ndp_track_steps the gather waits for exactly the control step that read its buffer last.  Needs a list with >= 2 entries per
 * node spacing (the reference: 5), else -17: the serial form above serves.  Same results as the serial form and the one-handle tick. */
int ndp_xchg_tick_begin(ndp_xchg *x, ndp_handle *h, const void *d_t, int flags, void *d_gathered_next);
/* on = 1: a begin's launches on the exchange's stream (event wait, advance + columns, ncclAllGather, event record: ~15 us of host time)
 * are made by a thread the exchange owns; ndp_xchg_tick_begin then only describes them (~2 us) and ndp_xchg_tick_step waits until its
 * tick's have been made.  One host thread's launches are what bounds the remote tick one period ahead; with two the device does.  Errors
 * of that thread surface at the next begin / step.  Switch only with no gather ahead (-14 otherwise); off (the default) = the caller's thread. */
int ndp_xchg_tick_async(ndp_xchg *x, int on);
int ndp_xchg_tick_step(ndp_xchg *x, ndp_handle *h, const void *d_x_odom, const void *d_vz, const void *d_throttle, int flags,
                       void *d_cmd, void *d_u0, const void *d_gathered, void *stream);
const char *ndp_xchg_last_error(const ndp_xchg *x);
int ndp_xchg_destroy(ndp_xchg *x);

/* Test hook: number of doubles of the LDS image dump, and a step that also dumps it (B = 1 use). */
int ndp_debug_lds_doubles(int N);
/* Test hook: where things sit in that dump: out8 = {XI, MB, CB, MB stride, CB stride, image size, first stamp, 0} (doubles). */
int ndp_debug_lds_layout(int N, int *out8);
/* Test hook: one v_mfma_f64_16x16x4_f64 on caller-chosen per-lane operands a[64], b[64], c[4][64]; d has 832 doubles:
 * d[0..255] = result registers [4][64], d[256..319] = a cross-lane checksum (readlane + wave reductions),
 * d[320..383] = one v_mfma_f64_4x4x4_4b_f64 (four blocks) on a, b with accumulator c[0], d[384..639] = a after the row
 * broadcasts of lanes 0, 4, 8, 12 of every 16-lane row (DPP row_newbcast), d[640..831] = a after the row rotations by 4, 8, 12
 * lanes (DPP row_ror). */
int ndp_debug_mfma_probe(const double *a, const double *b, const double *c, double *d);
/* Test hook: the config-5 instructions through their backends.  mode 0: one v_mfma_f32_16x16x4_f32 on a[0][64], b[0][64];
 * mode 1: one v_mfma_f32_16x16x16_bf16 on four packed contraction steps a[4][64], b[4][64]; c[4][64] -> d[0..255];
 * d[256..319] = the four-lane row sum of a[0] (lanes 4 apart inside each 16-lane row). */
int ndp_debug_mfma_probe_f32(const float *a, const float *b, const float *c, float *d, int mode);
/* Profiling hook: enable = 1 makes every instance of the following steps write its 24 phase stamps (shader clock; NDP_NSTAMP in
 * rti_wave.hpp); out (or NULL) receives the [B][24] stamps of the last step before the switch is applied (0-8: the wave program's
 * phases, 9-15: the kernel's -- downwash tile, entry / exit clocks --, 16-23: the one-launch tick's prologue). */
int ndp_debug_stamps(ndp_handle *h, int enable, double *out);
/* Measurement hook: ndp_downwash_device through the LDS-free form of the downwash kernel (weights streamed from L2, at most 192
 * registers per lane: it can be resident on a CU beside the control-step kernel). */
int ndp_debug_downwash_stream_device(ndp_handle *h, const void *d_other, const void *d_ego_ref, const void *d_ego_xy,
                                     void *d_f_out, void *stream);
/* Profiling hook: where the last host-array step spent its time on the CPU, microseconds: out4 = {packing the inputs into the
 * page-locked mirror, enqueueing (launches / copies), waiting for the results, copying them out}. */
int ndp_debug_host_timing(ndp_handle *h, double *out4);
/* ... and what the host path runs on: out3 = {hardware threads of the machine, cores this process may really use (affinity mask and
 * cgroup CPU quota), pack threads the handle started (-1: no host-array step yet)}. */
int ndp_debug_host_info(ndp_handle *h, int32_t *out3);
/* Test hook: which control-step kernels this handle has launched.  mask (or NULL) receives the rows of the library's kernel table
 * (enum RtiId in csrc/rti_table.hpp) launched since the last call, as bit RtiId, and reading clears it; a step captured into a graph
 * counts once, at capture.  out3 (or NULL) = {rows of the table, instances per workgroup, 1 if the downwash network can run inside
 * the control step's launch (else a separate launch first)}. */
int ndp_debug_rti_launched(ndp_handle *h, uint64_t *mask, int32_t *out3);
/* Test hook: how many HIP resources the library holds in this process right now -- device buffers, page-locked host blocks, events
 * and streams of every handle and exchange alive (memory handed to the caller by ndp_peer_alloc is not counted).  Back at its earlier
 * value once whatever was created since has been destroyed: nothing leaked. */
long long ndp_debug_live_resources(void);
int ndp_step_debug(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                   const double *other, const double *ego_xy, double *u0, double *lds_dump);

#ifdef __cplusplus
}
#endif
#endif
