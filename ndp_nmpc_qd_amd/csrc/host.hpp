// host.hpp -- the private host interface of the library's translation units: the handle, the entry-point frame and the host functions
// one unit calls in another.
//   rti_kernels.hip  the control-step kernels (rti_*_kernel), their table k_rti (rows: rti_table.hpp) and its launcher; first in build.UNITS,
//                    by far the longest compile -- no other unit names one of its kernels.  Also mfma_probe*_kernel, mlp_kernel and
//                    tick_pre_kernel with their launchers: they share inlined device functions with the control-step kernels, and apart
//                    from them the compiler specialises those functions (different code for them and for the one-launch ticks)
//   ndp_hip.hip      the handle's runtime: pack threads, create / destroy, every step form (enqueue_step, launch_rti, rti_pick), the
//                    host-array step, timing, the sensitivities, the adjoint / forward-mode entry points, ndp_set_model, the debug hooks
//   downwash.hip     the downwash network's forward entry points, mlp_stream_kernel + the prefetch protocol, ndp_set_mlp_weights,
//                    plant_force_kernel (f4: the downwash force on the plant), mlp_multi_kernel / plant_force_multi_kernel (K neighbours);
//                    one launcher for both force kernels (launch_plant_force), one host-array body per single / K pair (plant_force_host,
//                    downwash_host) over one statement of what they stage in sThr
//   rows.hip         the rows f1 - f4: reference window and list, follower relay, throttle estimator, actuator command, plant, rollouts
//                    (rollout_head: what all three start with; rollout_formation: the body of both formation rollouts)
//   tick.hip         the control tick's host side (ndp_tick*); no kernel: compiled for the host only
//   mlp_vjp.hip      the downwash network's backward pass (ndp_downwash_vjp_device, ndp_downwash_multi_vjp_device: one body, downwash_vjp)
//                    and its weights set from device memory
//   mlp_fit.hip      the downwash network on sample rows: the forward (ndp_mlp_rows_device) and the fit's loss and weight gradient in one
//                    pass (ndp_mlp_fit_rows_device); shares mlp_vjp.hip's device functions (mlp_vjp_dev.hpp) and the text of its rounds
//                    (mlp_vjp_back.inc, mlp_vjp_part.inc)
//   mlp_jvp.hip      the downwash network's forward mode (ndp_downwash_jvp_device, ndp_downwash_multi_jvp_device: one body, downwash_jvp)
//   mlp_train.hip    the downwash network's optimiser step: Adam + spectral-norm cap in one launch (ndp_mlp_adam_sn_device), the layers'
//                    spectral norms (ndp_mlp_spectral_norms*)
//   plant_deriv.hip  the plant over a given input sequence and its derivatives (ndp_plant_rollout_device, ndp_plant_rollout_vjp_device,
//                    ndp_plant_rollout_jvp_device); a tick's arithmetic is plant_dyn.hpp's, shared with rows.hip's plant_kernel; the
//                    ticks / substeps refusals of these and of closed_loop.hip's calls (plant_seq_check).  The plant's three numbers
//                    every launcher of it passes: plant_num, below
//   plant_force_deriv.hip  the derivatives of the downwash force on the plant (ndp_plant_force_vjp_device, ndp_plant_force_jvp_device and
//                    their multi forms); hosts mlp_vjp.hip's backward pass (mlp_vjp_dev.hpp, mlp_vjp_back.inc, mlp_vjp_part.inc) and
//                    mlp_jvp.hip's direction (mlp_jvp_dev.hpp, mlp_jvp_direction.inc) behind a row loader of its own
//   closed_loop.hip  the closed loop over given windows in one call per direction (ndp_closed_loop_device, ndp_closed_loop_vjp_device,
//                    ndp_closed_loop_jvp_device): the step, its adjoint and its forward mode are the existing kernels, launched unchanged;
//                    the three link kernels between them live here.  Host side: ClView hands out tick k's slices and tape slot,
//                    cl_deriv_begin is what the derivative calls do before they enqueue.  Also the formation's form, with the force on
//                    the plant made inside the loop (ndp_closed_loop_formation_config / _device / _vjp_device,
//                    ndp_plant_force_scatter_device): the reverse link's lane body is closed_loop_rev_lane.inc, shared by both link kernels
//   exchange.hip     peer-mapped windows (ndp_peer_*), the RCCL exchange (ndp_xchg_*) and the remote tick one control period ahead
// A kernel sits with the host code that launches it; device code that two units' kernels inline is a header (mlp_tile.hpp, ref_point.hpp,
// tick_wave.hpp, mlp_vjp_dev.hpp, mlp_jvp_dev.hpp, plant_dyn.hpp, plant_adj.hpp, plant_tan.hpp), and so are the argument blocks the host fills (kern_args.hpp).
// The functions declared below are NDP_HIDDEN: the library exports the C-ABI of include/ndp_nmpc.h and nothing more.
// Ownership: whatever the handle or an exchange got from the HIP runtime -- device and page-locked memory, events, streams -- is a member
// of a hip_own.hpp type (DevBuf, PinnedBuf, Event, Stream) and is released by that member's destructor; every raw pointer, hipEvent_t or
// hipStream_t is a view into an owner's block or the caller's.  A new workspace is one such member and an ensure() at its first use.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "wave_gfx950.hpp"   // defines the device qualifiers, must precede rti_wave.hpp
#include "cfg_params.hpp"
#include "kern_args.hpp"
#include "rti_table.hpp"
#include "hip_own.hpp"

#define NDP_HIDDEN __attribute__((visibility("hidden")))

using namespace ndp;

struct ndp_handle {
    // the handle's stream, and the downwash prefetch's (ensure_prefetch).  Declared first: members are destroyed in reverse order, the
    // streams after every buffer and event
    Stream stream, aux;
    ndp_cfg cfg;
    RtiParams P;
    int lds_per_wave = 0;      // doubles
    int waves = 4;             // instances per workgroup
    int n_simd = 1024;         // SIMDs of the device (4 per CU)
    // bit RtiId of every control-step kernel launched since ndp_debug_rti_launched last read it (launch_kern; relaxed: a test hook)
    mutable std::atomic<uint64_t> rti_launched{0};
    bool use_queue = false;    // interior-point solves through the work list: producer + consumer launch per step (QueueArgs)
    // cfg.work_queue = 0 at (N, n_rti) = (20, 1), batch >= 2 instances per SIMD: the list is switched by what the steps do (queue_policy)
    bool queue_auto = false;
    PinnedBuf<unsigned long long> hIpm;      // page-locked [2]: the device's monotonic counts (interior-point instances, steps executed),
                                             // copied behind every QP_WINDOW-th launch
    unsigned long long ipm_seen = 0, steps_seen = 0;   // the snapshot the last decision was taken on
    unsigned queue_launches = 0;             // launches since the last copy was enqueued
    // Views, not owners.  Into dOut: su0 | dStatus | dIters (the small outputs), then the persistent iterate dX | dU.  Into dIn: sx0, sxr,
    // sur, sf, sother, sego (staging of the f1-f4 host entry points).  dRingU: behind dRingX in its allocation.  lastStatus / lastIters:
    // where the last step wrote them (dStatus / dIters or a slot's output mirror).  tick_remote and HostSlot::dump are the caller's.
    double *dX = nullptr, *dU = nullptr;
    double *sx0 = nullptr, *sxr = nullptr, *sur = nullptr, *sother = nullptr, *sego = nullptr, *su0 = nullptr;
    float *sf = nullptr;
    int *dStatus = nullptr, *dIters = nullptr;
    const int *lastStatus = nullptr, *lastIters = nullptr;
    double *dRingU = nullptr;
    // persistent device state
    DevBuf<float> dForce, dFrag;
    DevBuf<double> dKC;        // constants block of the LDS image (fill_kc)
    DevBuf<int> dTables;       // per-lane index tables of the Riccati sweep (fill_tables)
    DevBuf<signed char> dAct;      // [B][act_pitch(N)] QP_AUTO's active sets, kept between control steps (RtiIo::act); emptied by reset / set_iterate
    // ndp_sens_enable: initial-state sensitivities of every step's QP (rti_sens_kernel): level 0 off, 1 du0/dx0, 2 also dU/dx0 and dX/dx0
    int sens_level = 0;
    DevBuf<double> dSensU0, dSensU, dSensX;   // [B][4][10], [B][N][4][10], [B][N+1][10][10] (the last two: level 2)
    // ndp_sens_params_enable: du0/dxr [B][4][N+1][10], du0/dur [B][4][N][4], du0/df [B][4][N+1][3] (rti_psens_kernel); null: off
    DevBuf<double> dPSensXr, dPSensUr, dPSensF;
    // ndp_step_vjp_device's workspace (first call): the tape's iterate X | U, then u0 [B][4]; status | iterations [B] each; kept sets
    DevBuf<double> dVjp;
    DevBuf<int> dVjpSt;
    DevBuf<signed char> dVjpAct;
    // ndp_closed_loop_vjp_device's workspace (first call), what one tick hands the next: gu0 [B][4] | gx_p [B][10] | the step's gx0 [B][10] |
    // the step's gmodel row [B][16] (closed_loop.hip)
    DevBuf<double> dClWs;
    // ndp_closed_loop_formation_config: one allocation, int32: the index [B][K] | the reverse lists' offset [B+1] | edge [form_edges]
    // (closed_loop.hip: ClGather); null: not configured
    DevBuf<int> dFormIndex;
    int form_K = 0, form_edges = 0;
    // ndp_closed_loop_formation_vjp_device's workspace (first call; the largest K: sized for NDP_MAX_NEIGH): gF [B][3] | g_z [B][8][6] |
    // the weight gradient's fp64 accumulator [NDP_MLP_NPARAM], then a tick's fp32 g_w [NDP_MLP_NPARAM]
    DevBuf<double> dFormWs;
    // mlp_vjp.hip: layers 2 and 3 transposed, one fp32 record per matrix instruction of the backward pass (FRT_TOTAL floats, written with
    // dFrag by both ndp_set_mlp_weights forms); ndp_downwash_vjp_device's per-workgroup partial weight gradients [mlp_vjp_groups][NDP_MLP_NPARAM]
    // (ndp_downwash_multi_vjp_device shares them: it never launches more workgroups than that)
    DevBuf<float> dFragT, dGwPart;
    // ndp_mlp_fit_rows_device's partials, a workspace of its own (its size does not follow the batch shape): gradients
    // [NDP_FIT_MAX_GROUPS][NDP_MLP_NPARAM] fp32 | losses [NDP_FIT_MAX_GROUPS] fp64 | rows used, skipped [NDP_FIT_MAX_GROUPS][2] int32
    DevBuf<float> dFitPart;
    // mlp_train.hip: word 0 = the ticket of ndp_mlp_adam_sn_device's four workgroups (0 between launches), then 4 doubles and a blob's
    // floats: the staging of the host form ndp_mlp_spectral_norms (TRAIN_WS_BYTES)
    DevBuf<unsigned long long> dTrain;
    DevBuf<double> dThr;       // hover-throttle estimator state, SoA [8][B]
    DevBuf<double> dStamps;    // [B][NDP_NSTAMP] whole-batch phase stamps (ndp_debug_stamps)
    DevBuf<double> dTraj;      // f1: the trajectories and the tick's caches (layout: TrajView)
    int traj_seg = 0;
    DevBuf<double> dRingX;     // f1: the reference's sliding list of reference points, phase-major (RingGeom), one allocation (first use): X, then dRingU
    unsigned long long list_n = 0;                 // absolute index of the list's oldest entry = control ticks since the list was built
    int segc_par = 0;                              // which copy of the one-launch tick's segment cache the NEXT tick reads (tick_cache_store)
    int list_step = 5;
    // ndp_tick: the node's control tick on the device (rti_kernel<..., TICK>; other shapes: tick_pre_kernel + the control step)
    DevBuf<int> dTickIndex;          // [B] neighbour instance of every vehicle (< 0: none), or null: no vehicle has one
    DevBuf<double> dTickThrust;      // [B] the thrust command of the previous tick (what hover_throttle_callback reads off body_rate_cmd)
    bool tick_gate = true;           // gate the downwash on |neighbour window node 0 xy - ego odometry xy| < r_horiz (ndp_nmpc_leader_node.py:65-74)
    const double *tick_remote = nullptr;   // ndp_tick_config_remote: the neighbours' windows are rows of the CALLER's buffer (an exchange's gathered /
    int tick_remote_stride = 6;            // peer-mapped windows, [rows][N+1][stride]) instead of this handle's own list
    struct TickSlot { bool busy = false, want_u0 = false; } tslot[2];
    DevBuf<double> dRelay;     // follower relay: [B][4] = filtered offset xyz + initialised flag
    DevBuf<double> sThr;       // staging of the f1-f4 host entry points: 11 B doubles
    // downwash one tick ahead on a second stream (aux; LateArgs): force slots, protocol words, the stream's fork / join events
    DevBuf<float> dForceAB[2];
    DevBuf<unsigned long long> dProto;
    Event evFork, evJoin;
    unsigned prefetch_timeout_us = 100000, pf_groups_rti = 1, pf_ntiles = 1;
    DevBuf<unsigned> dQctr;    // work list: entry count | B instance ids
    DevBuf<int> dQids;
    bool have_mlp = false;
    // Host-pointer entry points.  ONE block holds every input of a step (x0 | xr | ur | f | other | ego_xy, each 256-byte
    // aligned) and one its outputs (u0 | status | iters | X | U).  Two slots of page-locked host mirrors of both (HostSlot,
    // allocated at the first host step): the caller's arrays are packed into a slot's input mirror by the handle's pack threads,
    // the kernel reads that mirror over PCIe and writes u0 / status / iterations (and, when asked, a copy of the new iterate)
    // into the slot's output mirror itself -- one launch and one wait per step, no DMA operation, at every batch size (measured,
    // batch 1024: 106 us per step with two steps in flight against 121 us with one H2D copy per step and 147-157 us with the
    // block copied in chunks as it is packed: every asynchronous copy operation costs ~30 us of latency on this platform).
    // With two slots the packing of step i+1 runs while step i's kernel does (ndp_step_begin / ndp_step_end).
    // The persistent iterate dX | dU always lives in HBM.  dIn / dOut: device-side staging of the f1-f4 host entry points
    // (views sx0 ..) and the small outputs of device-pointer steps.
    DevBuf<unsigned char> dIn, dOut;
    size_t off_x0 = 0, off_xr = 0, off_ur = 0, off_f = 0, off_other = 0, off_ego = 0, in_bytes = 0;
    size_t off_u0 = 0, off_st = 0, off_it = 0, out_bytes = 0, out_all = 0;
    DevBuf<double> sdbg;       // the LDS dump of ndp_step_debug
    struct HostSlot {
        PinnedBuf<unsigned char> hIn, hOut;
        Event evOut;                                         // the step that uses the slot has completed
        bool busy = false, want_iter = false;
        double *dump = nullptr;
    } slot[2];
    bool slots_ready = false;
    // ndp_track_steps: the completion of every control step marks an event WITHOUT a packet of its own (the dispatch packet's
    // completion signal, hipExtLaunchKernel) -- what another stream orders itself behind (ndp_xchg_begin's after_event)
    bool track_steps = false;
    bool last_step_tracked = false;   // does stepDone[step_seq & 3] belong to the control step launched LAST?
    bool track_pending = false;       // a tracked step on a caller's stream has not been waited for (wait_all)
    Event stepDone[4];
    unsigned step_seq = 0;
    double host_us[4] = {0, 0, 0, 0};   // last host step: packing | enqueue | wait for the results | copy-out  (ndp_debug_host_timing)
    int host_cores = 0, pack_threads = 0;   // what ensure_slots found and started (ndp_debug_host_info)
    int slot_head = 0, slot_tail = 0, slots_busy = 0;   // begin fills slot_head, end drains slot_tail
    std::unique_ptr<struct PackPool> pool;
    // the last foreign stream a *_device call enqueued on: the getters wait for it (hipEvent)
    Event evLast;
    bool ev_pending = false;
    // timing
    int timing = 0;            // 0 off, n > 0: bracket every n-th launch of each kernel with HIP events
    int64_t launch_no[2] = {0, 0};
    bool timing_open = false;
    struct Ev { Event a, b; int kind = 0; };
    std::vector<Ev> events;
    std::mutex mu;
    std::string err;
};

#define NDP_HIP(h, call)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                  \
            return -(int)e_ - 1000;                                                        \
        }                                                                                  \
    } while (0)

static inline RingGeom ring_geom(const ndp_handle *h) { return RingGeom{h->list_step, h->cfg.N + 1}; }

enum { FRT_TOTAL = 2 * 128 * 64 };   // floats of dFragT: 128 records of 64 lanes per layer (mlp_vjp.hip: fragt_source)
// workgroups of mlp_vjp_kernel = rows of dGwPart: one per 128 rows (four 32-row tiles), at most 256 (then a grid-stride loop) -- a function
// of the batch shape only
enum { VJ_MAX_GROUPS = 256 };
static inline int mlp_vjp_groups(const ndp_handle *h)
{
    const int ntiles = (h->cfg.batch * (h->cfg.N + 1) + 31) / 32, ngroups = (ntiles + 3) / 4;
    return ngroups < VJ_MAX_GROUPS ? ngroups : VJ_MAX_GROUPS;
}

enum { FIT_WS_BYTES = NDP_FIT_MAX_GROUPS * (17859 * 4 + 8 + 2 * 4) };   // dFitPart
enum { TRAIN_WS_BYTES = 64 + 4 * 8 + 17859 * 4 };   // dTrain: ticket (64 bytes of its own) | sigma [4] fp64 | blob [NDP_MLP_NPARAM] fp32

enum { TICK_ESTIMATE = NDP_TICK_ESTIMATE, TICK_WANT_U0 = NDP_TICK_WANT_U0, TICK_T_UNIFORM = NDP_TICK_T_UNIFORM };

// ---- file-local helpers several units need
static inline size_t nxs(const ndp_handle *h) { return (size_t)h->cfg.batch * (h->cfg.N + 1) * NX; }
static inline size_t nus(const ndp_handle *h) { return (size_t)h->cfg.batch * h->cfg.N * NU; }
static inline size_t nfs(const ndp_handle *h) { return (size_t)h->cfg.batch * (h->cfg.N + 1) * 3; }
static inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
static inline size_t act_bytes(const ndp_handle *h) { return (size_t)h->cfg.batch * (size_t)act_pitch(h->cfg.N); }
// The trajectory block dTraj (ndp_ref_set_trajectory), one allocation of `doubles`, in this order: coefficients [B][S][28] (x, y, z: 8
// each, yaw: 4) | time_cum [B][S+1] | time_seg [B][S] | final_pt [B][3] | the one-launch tick's segment cache [B][SEGC_PER] (empty =
// NaNs: tick_early) | the segment hints int[B] (ref_point) | the cache's second copy [B][SEGC_PER] (tick_cache_store).  base = null:
// the size only.
struct TrajView {
    double *coeff, *tcum, *tseg, *fpt, *segc[2];
    int *hint;
    size_t doubles;
};
static inline TrajView traj_view(double *base, size_t B, size_t S)
{
    TrajView v;
    size_t o = 0;
    auto part = [&](size_t n) { double *p = base ? base + o : nullptr; o += n; return p; };
    v.coeff = part(B * S * 28); v.tcum = part(B * (S + 1)); v.tseg = part(B * S); v.fpt = part(B * 3);
    v.segc[0] = part(B * SEGC_PER); v.hint = reinterpret_cast<int *>(part((B * 4 + 7) / 8)); v.segc[1] = part(B * SEGC_PER);
    v.doubles = o;
    return v;
}
static inline TrajView traj_view(const ndp_handle *h) { return traj_view(h->dTraj, (size_t)h->cfg.batch, (size_t)h->traj_seg); }
// the step's iteration words (RtiIo::iters) -> the caller's interior-point iteration counts
static inline void copy_ipm_iters(int32_t *dst, const int32_t *src, size_t n)
{
    for (size_t i = 0; i < n; ++i) dst[i] = src[i] & ITERS_IPM_MASK;
}

// the numbers every launch of the plant takes (plant_kernel, PlantSeq, ClPlant): the substep dt / substeps, 1 / mass, g
struct PlantNum { double h, inv_mass, g; };
static inline PlantNum plant_num(const ndp_handle *h, double dt, int substeps) { return PlantNum{dt / substeps, 1.0 / h->cfg.mass, h->cfg.gravity}; }

struct Neigh {                 // neighbour windows of a step (device pointers)
    const double *other = nullptr;
    int stride = NX;           // doubles per node: 10 or 6
    const int *index = nullptr;
    const double *ego_xy = nullptr;
    size_t pitch = 0;          // doubles between rows of `other`; 0 = dense, (N+1) stride
    size_t ego_pitch = 0;      // doubles between instances of ego_xy; 0 = dense, 2
};

struct StepOut {               // where a step's status / iteration counts go and whether the new iterate is mirrored (device-accessible
    int *status = nullptr;     // pointers; null = the handle's HBM block / no mirror): the host-array step of small batches points
    int *iters = nullptr;      // them into a page-locked host block
    double *Xm = nullptr, *Um = nullptr;
    hipEvent_t done = nullptr; // marked by the step's last launch through its own dispatch packet (no event packet behind it), or null
    size_t xr_pitch = 0, ur_pitch = 0;   // doubles between the instances' reference windows; 0 = dense arrays (see BatchPtrs)
    double *cmd = nullptr;               // ndp_tick: the actuator command written by the control step itself (BatchPtrs::cmd) ...
    const double *kthr = nullptr;        // ... from k_throttle[B]
    double *thrust_keep = nullptr;
    bool f_f64 = false;                  // d_f holds doubles (ndp_step_ex_f64)
    const TickArgs *tick = nullptr;      // the launch is a whole control tick (rti_kernel<..., TICK>): list advance + estimator inside
};

// What the derivative kernels that recompute a recorded step share (rti_vjp_kernel, rti_wvjp_kernel, rti_jvp_kernel).  Their entries take
// the step's inputs and the tape it started from, never written (the recompute advances a copy: two calls on one tape give the same result),
// and optionally return the recomputed u0 and status for the caller to check against the recorded ones.
struct Tape {
    const void *x0, *xr, *ur, *f, *X_lin, *U_lin, *act_lin;
    void *u0_check, *status_check;
};

enum RecomputeId { RC_WVJP, RC_JVP, RC_VJP, RC_MJVP };   // the derivative kernels that recompute a recorded step (rti_kernels.hip: recompute_kernel)

// ---- host functions one unit calls in another (no locking, no sync: the caller holds h->mu).  C linkage like the entry points they
// sit beside; hidden, so not exported.
extern "C" {
// rti_kernels.hip.  launch_kern: one launch of row `id`, the caller checks hipGetLastError; rti_set_lds: the dynamic LDS of the table's
// plain rows and the recompute kernels (sens false) or of its sensitivity rows
NDP_HIDDEN bool queue_shape(const ndp_handle *h);
NDP_HIDDEN void launch_kern(const ndp_handle *h, RtiId id, hipStream_t s, KernArgs &ka, SensArgs &sa, hipEvent_t start = nullptr,
                            hipEvent_t stop = nullptr);
NDP_HIDDEN const void *recompute_kernel(RecomputeId id, bool n20);
NDP_HIDDEN hipError_t rti_set_lds(bool sens, int lds_bytes, const char **what);
NDP_HIDDEN hipError_t mlp_prepare(void);
NDP_HIDDEN int launch_mlp(ndp_handle *h, const Neigh &nb, const double *d_ego, float *d_f, hipStream_t s, size_t ego_pitch = 0);
NDP_HIDDEN void launch_tick_pre(const TickPre &a, hipStream_t s);
// ndp_hip.hip
NDP_HIDDEN int sens_refuse(ndp_handle *h, const char *what);
NDP_HIDDEN int note_stream(ndp_handle *h, hipStream_t s);
NDP_HIDDEN int set_device(ndp_handle *h);
NDP_HIDDEN int wait_all(ndp_handle *h);
NDP_HIDDEN int begin_timing(ndp_handle *h, hipStream_t s, int kind, bool defer = false);
NDP_HIDDEN int end_timing(ndp_handle *h, hipStream_t s);
NDP_HIDDEN bool can_fuse(const ndp_handle *h);
NDP_HIDDEN int launch_rti(ndp_handle *h, const double *d_x0, const double *d_xr, const double *d_ur, const float *d_f, double *d_u0,
                          double *d_dbg, hipStream_t s, const Neigh *nb = nullptr, const StepOut *so = nullptr, bool prefetched = false);
NDP_HIDDEN int enqueue_step(ndp_handle *h, const double *d_x0, const double *d_xr, const double *d_ur, const float *d_f, const Neigh &nb,
                            double *d_u0, double *d_dbg, hipStream_t s, const StepOut *so = nullptr);
NDP_HIDDEN int ensure_slots(ndp_handle *h);
NDP_HIDDEN int recompute_workspace(ndp_handle *h);
NDP_HIDDEN int recompute_on_workspace(ndp_handle *h, hipStream_t s, const Tape &t, const void *fn20, const void *fn0, void *a1, void *a2);
// downwash.hip.  launch_plant_force: K = 0 the single form, d_index int32[B]; else K neighbours per vehicle, d_index int32[B][K]
// (check_neigh: -2 unless 1 <= K <= NDP_MAX_NEIGH; the launchers do not check)
NDP_HIDDEN int launch_plant_force(ndp_handle *h, const double *d_x, const int *d_index, int K, int gate, double scale, double *d_f,
                                  double *d_xy, hipStream_t s);
NDP_HIDDEN hipError_t mlp_multi_prepare(void);
NDP_HIDDEN int check_neigh(ndp_handle *h, const char *who, int K);
NDP_HIDDEN int launch_mlp_multi(ndp_handle *h, const double *d_other, int other_stride, const int *d_index, int K, const double *d_ego,
                                const double *d_ego_xy, float *d_f, hipStream_t s);
// rows.hip
NDP_HIDDEN ThrCfg thr_cfg(const ndp_handle *h);
NDP_HIDDEN RefCfg ref_cfg(const ndp_handle *h, double toff);
NDP_HIDDEN void launch_throttle_reset(const ndp_handle *h);
NDP_HIDDEN int launch_list_window(ndp_handle *h, double *d_xr, double *d_ur, hipStream_t s);
// tick.hip
NDP_HIDDEN int ensure_tick(ndp_handle *h);
NDP_HIDDEN int tick_step_enqueue(ndp_handle *h, hipStream_t s, const double *x_odom, double *cmd, double *u0, const double *windows,
                                 unsigned long long pos);
// mlp_vjp.hip
NDP_HIDDEN void make_fragments_t(const float *blob, float *frt);
NDP_HIDDEN hipError_t mlp_vjp_prepare(void);
// mlp_fit.hip
NDP_HIDDEN hipError_t mlp_fit_prepare(void);
// plant_force_deriv.hip
NDP_HIDDEN hipError_t plant_force_deriv_prepare(void);
NDP_HIDDEN int launch_plant_force_vjp(ndp_handle *h, const char *who, const void *d_x, const void *d_index, int K, int gate, double scale,
                                      const void *d_gf, void *d_gz, void *d_gw, hipStream_t s);
// plant_deriv.hip.  The refusals of every call that takes `ticks` ticks of `substeps` substeps (closed_loop.hip's too): -2 with the reason
NDP_HIDDEN int plant_seq_check(ndp_handle *h, const char *who, int ticks, int substeps);
// exchange.hip
NDP_HIDDEN int peer_mapped(const void *p);
NDP_HIDDEN void launch_pack_pv_list(const double *base, size_t pitch, int np1, double *pv, size_t B, hipStream_t s);
}  // extern "C"
// ndp_hip.hip (C++ linkage: it returns a string)
NDP_HIDDEN std::string recompute_refusal(const ndp_cfg &c, const char *noun, const Tape &t, const char *own);
// tick.hip (C++ linkage: it returns a TickPre)
NDP_HIDDEN TickPre tick_pre(const ndp_handle *h, bool adv, const double *t, double t_all, bool est, const double *x_odom, const double *vz,
                            const double *throttle, double *pv = nullptr);

// The frame of a handle's entry point: h->mu is held for the whole call.  In this order: -1 for a null handle or missing arguments
// (args false), -2 while sensitivities are on if the entry point does not compute them (refuse: its name), then the device is
// selected and the stream resolved (null: the handle's own).  rc != 0: the call returns it.
struct Entry {
    ndp_handle *h;
    std::unique_lock<std::mutex> lk;
    hipStream_t s = nullptr;
    int rc = -1;
    Entry(ndp_handle *h_, bool args, void *stream = nullptr, const char *refuse = nullptr) : h(h_)
    {
        if (!h) return;
        lk = std::unique_lock<std::mutex>(h->mu);
        s = stream ? (hipStream_t)stream : h->stream;
        if (refuse && h->sens_level) rc = sens_refuse(h, refuse);
        else if (args) rc = set_device(h);
    }
    // the end of a form that enqueues on a caller's stream: the getters wait for that stream too
    int noted(int r) { return r ? r : note_stream(h, s); }
    // the end of a host-array form, behind its copies out: everything on the handle's stream has completed
    int synced(int r)
    {
        if (r) return r;
        NDP_HIP(h, hipStreamSynchronize(h->stream));
        return 0;
    }
};

