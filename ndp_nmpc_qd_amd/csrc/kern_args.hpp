// kern_args.hpp -- argument blocks of the rows, the tick and the control step that more than one translation unit uses (the host fills
// them, the kernels read them).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

#include <type_traits>

#include "wave_gfx950.hpp"   // defines the device qualifiers, must precede rti_wave.hpp
#include "rti_wave.hpp"      // RtiParams

namespace ndp {

struct ThrCfg { double a1, a2, hm, g, R, Q0, Q1, mass; };

// layout of the reference list in HBM (see the f1 list kernels, rows.hip)
struct RingGeom {
    int step, np1;                 // list entries per node spacing; N + 1
    __host__ __device__ int ring() const { return step * (np1 - 1) + 1; }
    __host__ __device__ size_t px() const { return (size_t)step * 2 * np1 * 10; }     // doubles per vehicle, x ring
    __host__ __device__ size_t pu() const { return (size_t)step * 2 * np1 * 4; }
    __host__ __device__ size_t slot(unsigned long long j) const { return (size_t)(j % step) * 2 * np1 + (size_t)((j / step) % np1); }
};

struct RefCfg { int B, N, n_seg; double dt, mass, g, toff; };   // toff: added to every vehicle's node-0 time (rollouts)

struct TickPre {
    RefCfg cf;
    const double *coeff, *tcum, *tseg, *fpt;
    int *seg_hint;                     // [B] the segment each vehicle's last point lay in (ref_point)
    const double *t;                   // [B] trajectory time of the tick, or null: t_all for every vehicle
    double t_all;
    int advance;                       // 0: the list is not advanced
    unsigned long long j_new;          // absolute index of the entry the new point becomes
    RingGeom rg;
    double *rx, *ru;
    ThrCfg thr;
    double *st;                        // estimator state, SoA [8][B]
    const double *vz;                  // vz of vehicle b at vz[b * vz_pitch]: a [B] array (pitch 1) or column 5 of the odometry rows (pitch 10)
    size_t vz_pitch;
    const double *throttle;            // [B]: the thrust command sent last tick (caller's array, or the one the control step kept)
    int est;                           // run the estimator this tick
    // ndp_xchg_tick_begin: the advanced window's position / velocity columns -> pv[b][N+1][6] in the same launch (one launch less on a
    // path that is bound by the host's launches); the window starts at list slot pv_slot, its node N is the point made here
    double *pv = nullptr;
    size_t pv_slot = 0;
};

// ------------------------------------------------------------------------------------------ the control step's argument blocks
struct BatchPtrs {
    const double *kc;
    const int *tables;      // host-built index tables (fill_tables)
    const double *x0, *xr, *ur;
    const float *f;
    double *X, *U, *u0;
    int *status, *iters;
    double *Xm, *Um;        // mirror of the new iterate ([B][N+1][10] | [B][N][4], page-locked host memory) or null
    double *dbg;
    double *stamps;         // [B][NDP_NSTAMP] phase stamps of every instance (ndp_debug_stamps), or null
    size_t xr_pitch, ur_pitch;   // doubles from one instance's reference window to the next: (N+1) 10 / 4 N for dense [B][N+1][10] / [B][N][4]
                                 // arrays; RingGeom::px / pu when the windows are read straight out of the reference list (ndp_tick)
    size_t x0_pitch;             // doubles from one instance's x0 to the next (10)
    // ndp_tick: the actuator command written beside u0 (RtiIo::cmd): cmd[B][4], k_throttle[B] (the estimator's state row), the thrust
    // kept for the next estimator update [B]; null cmd = a plain control step
    double *cmd;
    const double *kthr;
    double *thrust_keep;
    double cmd_mass;
    int f_f64;                   // 1: f holds doubles, [B][N+1][3] (ndp_step_ex_f64)
    signed char *act;            // [B][act_pitch(N)] the instances' kept active sets (RtiIo::act), or null: no warm start of the QP's active set
};

struct MlpArgs {            // fused downwash (null frag = not fused)
    const float *frag;
    const double *other;    // neighbour windows: row (instance) r starts at other + r * (N+1) * other_stride, node k at + k * other_stride
    const double *ego_xy;   // [B][2] or null (gate always open)
    float *force_out;       // [B][N+1][3] copy of the predicted force for callers
    double r2;
    int other_stride;       // doubles per node of `other`: 10 (a full reference window) or 6 (positions + velocities only, what the MLP reads)
    const int *other_index; // [B] row of `other` that holds instance i's neighbour (multi-GPU: a row of the gathered buffer);
                            // < 0 = no neighbour (force 0: the plain NMPC followers of a formation); null = row i
    int other_sys;          // 1: `other` is another process's / GPU's memory mapped through ndp_peer_open -- read it with system-scope loads
    size_t other_pitch;     // doubles from one row of `other` to the next: (N+1) other_stride when dense; RingGeom::px for windows in the list
    size_t ego_pitch;       // doubles from one instance's ego xy to the next: 2 ([B][2]), or 10 when the gate reads the odometry rows x0[B][10]
};

// Work list of instances whose QP needs the interior-point loop (batches with more instances than SIMDs).  An
// interior-point solve costs ~18 Riccati sweeps against 1 for the early exit, so with several instances per SIMD one such
// instance per workgroup leaves the other three SIMDs of its CU idle for most of the launch.  Instead the step is split:
//   producer launch  (QMODE 1): every wave runs the cheap part of its own instance; an instance whose equality-constrained
//                               minimiser is not inside the box is appended to the list (one atomic per such instance)
//                               and NOT touched otherwise;
//   consumer launch  (QMODE 2): wave j solves list entry j from scratch with the interior-point loop; waves past the end
//                               of the list exit at once -- the listed instances are spread evenly over all SIMDs.
// The list counter is zeroed by a one-wave launch behind the consumer (queue_reset_kernel).  (Round 3 first let the consumer do
// it -- every consumer workgroup counted itself with an atomic, the last one reset -- and paid for it: agent-scope atomics on one
// address are served at the memory side at 30-60 ns each and serialise, 61 us at batch 4096 where the memset node it replaced had
// cost 4.6 us.)  (An in-kernel queue -- finished waves popping
// other instances' solves -- was built first: as a second inlined copy of the unrolled step it wrecked the register
// allocation of both copies, as a called function it lost the scalar registers; either way 2.3x slower than this.)
struct QueueArgs {
    unsigned *count;        // entries of ids
    int *ids;               // [B]
    unsigned long long *ipm_total;   // [0] monotonic: instances that needed the interior-point loop (in place: counted by the kernel; work
                                     // list: added up by the reset launch); [1] monotonic: control steps executed (one count per launch) --
                                     // the pair the handle's automatic work-list rule looks at (queue_policy)
};

// Downwash predicted one tick ahead by mlp_stream_kernel on a second stream (ndp_downwash_prefetch_device), consumed by the
// control-step launch of the tick (ndp_step_device_prefetched).  Two chains of launches that order themselves on the device:
//   second stream : prefetch_gate_kernel (one wave: number m = previous + 1; waits until control step m - 2, the last reader of
//                   force slot m & 1, holds its values; publishes m in PF_CUR_M) -> mlp_stream_kernel (reads m with a plain load --
//                   it was written by the launch before it in its own stream; every wave writes its 32 rows of slot m & 1 with
//                   write-through stores and then its tile's epoch word := m)
//   main stream   : control step t = (completed control-step groups) / groups + 1 (plain load: only control steps, in this
//                   stream, advance it); waits late (after its cost phase) for the one or two tile epochs that cover its rows
//                   to reach t, loads its forces past the L2, and counts itself done-reading (WaveGfx950::late_count):
//                   PF_RTI_C1 + g  workgroups counted into group g = workgroup index mod groups, PF_RTI_C2 groups completed --
//                   launch t has read its slot completely at t * groups.
// The usual case costs the control step nothing at agent scope: prefetch_done_kernel, behind every downwash launch in its stream,
// publishes PF_MLP_DONE = m; a control step that finds PF_MLP_DONE >= t when it STARTS (plain load, fresh after the launch
// boundary) knows its slot was in memory before it began and reads it with ordinary cached loads.  Only a control step that
// started before its prediction was complete takes the epoch path.
// No word is shared by many waves at agent scope: the eight XCDs' L2s are not coherent with each other, agent-scope loads and
// atomics are served at the memory side and serialise per address (30-60 ns each: 1024 waves on one flag word cost 7 us per wave,
// one counting atomic per wave 18 us per launch).  Every word has its own 4 KB (PF_STRIDE words: its own memory channel).
// Nothing is baked into a launch, so captured launches replay correctly.  PF_MISSED: control-step waves whose wait timed out
// (zero force, status 5); PF_GATE_TIMEOUT: gate waits that timed out.
enum { PF_GROUPS = 8, PF_STRIDE = 512, PF_CUR_M = 0, PF_RTI_C1 = 1 * PF_STRIDE, PF_RTI_C2 = 9 * PF_STRIDE,
       PF_MISSED = 10 * PF_STRIDE, PF_GATE_TIMEOUT = 11 * PF_STRIDE, PF_MLP_DONE = 12 * PF_STRIDE, PF_SLOW = 13 * PF_STRIDE, PF_EPOCH = 14 * PF_STRIDE /* [2][ntiles] */ };
struct LateArgs {
    unsigned long long *proto;     // null = not a prefetched-force launch
    const float *F[2];             // the two force slots, [B][N+1][3] each
    unsigned timeout_us;
    unsigned groups_rti, ntiles;
};
__device__ __host__ inline unsigned pf_group_size(unsigned n, unsigned groups, unsigned g) { return n / groups + (g < n % groups ? 1u : 0u); }

// ndp_tick in ONE launch (rti_kernel<..., TICK = true>): what tick_pre_kernel does -- the reference list's newest entry, which is node
// N of this tick's window, and the hover-throttle estimator's update -- done by the control step's own wave in front of its work, so
// that a control tick is a single dispatch.  (As a launch of its own that part cost 7-8.5 us + a 4.5 us gap per tick in the kernel
// trace against 24.8 us for the control step: a third of the tick for 112 bytes per vehicle.)
enum { SEGC_SLOT = 32, SEGC_PER = 72 };      // doubles per slot / per vehicle of the tick's segment cache (tick_early)
struct TickArgs {
    const double *coeff, *tcum, *tseg, *fpt;   // the trajectories (ndp_ref_set_trajectory)
    const double *segc;                        // [B][SEGC_PER] the vehicles' current / next segment records (see tick_early): the copy this launch READS
    double *segc_wr;                           // ... and the copy it WRITES (every vehicle's record, re-filled or carried over): the next tick's `segc`
    int n_seg;
    const double *t;                           // [B] trajectory time of the tick, or null: t_all for every vehicle
    double t_all;
    int advance;                               // 0: the list is not advanced in this tick
    double toff, mass, g;                      // T_horizon; flatness constants
    unsigned long long j_new;                  // absolute index of the list entry the new point becomes
    size_t new_slot;                           // rg.slot(j_new), from the host (two 64-bit divisions otherwise, in front of the barrier)
    RingGeom rg;
    double *rx, *ru;
    ThrCfg thr;                                // estimator
    double *st;
    const double *vz;
    size_t vz_pitch;
    const double *throttle;
    int est;
};

struct KernArgs {
    RtiParams P;
    BatchPtrs bp;
    int B, lds_per_wave;
    MlpArgs ma;
    QueueArgs qa;
    LateArgs la;
    TickArgs ta;            // read by the TICK instantiations only
};
// rti_sens_kernel's outputs (ndp_sens_enable): [B][4][10] always, [B][N][4][10] and [B][N+1][10][10] at level 2 (else null)
struct SensArgs {
    double *du0 = nullptr, *dU = nullptr, *dX = nullptr;
    int level = 0;
};
// rti_psens_kernel's further outputs (ndp_sens_params_enable): [B][4][N+1][10], [B][4][N][4], [B][4][N+1][3]
struct PSensArgs {
    double *dxr = nullptr, *dur = nullptr, *df = nullptr;
};
static_assert(offsetof(KernArgs, P) == 0, "WaveGfx950::late_params reads the parameter block at the start of the argument segment");
static_assert(std::is_standard_layout<KernArgs>::value && std::is_trivially_copyable<KernArgs>::value,
              "KernargLate addresses members of the one kernel argument by offsetof");

// the derivative kernels' own blocks (rti_kernels.hip: rti_vjp_kernel / rti_wvjp_kernel, rti_jvp_kernel)
struct VjpArgs {
    const double *gu0, *gX, *gU;
    double *gx0, *gxr, *gur, *gf;
};
struct JvpArgs {
    const double *tx0, *txr, *tur, *tf;
    double *du0, *dX, *dU;
    int T;
};

}  // namespace ndp
