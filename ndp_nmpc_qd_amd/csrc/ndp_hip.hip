// ndp_hip.hip -- gfx950 kernels + the C-ABI of include/ndp_nmpc.h.
//
// Kernels
//   rti_kernel  : one wavefront per OCP instance runs the whole SQP-RTI step (rti_wave.hpp) out of its
//                 LDS slice; 4 waves (= 4 instances) per 256-thread workgroup, one per SIMD of a CU.
//                 FUSED: the downwash MLP tile (mlp_tile) runs in front of linearise inside the same launch.
//                 QMODE 1 / 2: producer / consumer of the work list (instances whose QP needs the interior point).
//   mlp_kernel  : DownwashNN.update + r_horiz gate for all (instance, horizon row) pairs; the four
//                 layers are chained through v_mfma_f32_32x32x2_f32 accumulators (no LDS round trip).
//   mlp_stream_kernel + prefetch_gate_kernel / prefetch_done_kernel : the downwash of the NEXT tick on a second stream, LDS-free
//                 (weights out of L2), ordered against the control step by per-tile epochs (LateArgs / PF_* words).
//   (peer_publish_kernel / peer_epoch_kernel and the RCCL exchange's pack kernels live in exchange.hip; host.hpp: which unit owns what)
//   ref_window_kernel, ref_list_*_kernel, throttle / actuator / plant kernels : the rows either side of the step (f1, f3, f4).
// The iterate (X, U) of a handle lives in HBM and stays there between steps; host-array steps (ndp_step / ndp_step_begin)
// read their inputs from, and mirror their outputs to, page-locked host slots over PCIe (zero-copy) -- see step_begin_locked.
// There is no CPU fallback: every entry point fails (<0) if HIP is unusable.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <sched.h>
#include <stdio.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "wave_gfx950.hpp"   // defines the device qualifiers, must precede rti_wave.hpp
#include "cfg_params.hpp"
#include "cond_qp.hpp"
#include "host.hpp"
#include "mlp_common.hpp"

namespace ndp {

// ------------------------------------------------------------------------------------------ RTI kernel
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

typedef __attribute__((address_space(3))) float *lds_f32;
typedef const __attribute__((address_space(3))) float *lds_cf32;
__device__ __forceinline__ void stage_fragments(const float *__restrict__ fr, lds_f32 dst, int tid, int nthreads);
__device__ __forceinline__ void mlp_tile(lds_cf32 fr, const float zb[3], int lane, float o[3]);
__device__ __forceinline__ bool gate_open(const double *other_inst, const double *ego_xy_inst, double r2);

__device__ __forceinline__ void bind_instance(RtiIo &io, const BatchPtrs &bp, int inst, int N)
{
    const size_t nx = (size_t)(N + 1) * NX, nu = (size_t)N * NU, nf = (size_t)(N + 1) * 3;
    io.x0 = bp.x0 + (size_t)inst * bp.x0_pitch;
    io.xr = bp.xr + inst * bp.xr_pitch;
    io.ur = bp.ur + inst * bp.ur_pitch;
    io.f = bp.f ? bp.f + inst * nf * (bp.f_f64 ? 2 : 1) : nullptr;
    io.f_is_f64 = bp.f_f64;
    io.X = bp.X + inst * nx;
    io.U = bp.U + inst * nu;
    io.Xm = bp.Xm ? bp.Xm + inst * nx : nullptr;
    io.Um = bp.Xm ? bp.Um + inst * nu : nullptr;
    io.u0 = bp.u0 + (size_t)inst * NU;
    io.status = bp.status + inst;
    io.iters = bp.iters + inst;
    io.dbg = bp.dbg;
    io.f_in_lds = 0;
    io.kc = bp.kc;
    io.tables = bp.tables;
    io.stamps = bp.stamps ? bp.stamps + (size_t)inst * NDP_NSTAMP : nullptr;
    io.act = bp.act ? bp.act + (size_t)inst * act_pitch(N) : nullptr;
    if (NDP_RARELY(bp.cmd != nullptr)) {
        io.cmd = bp.cmd + (size_t)inst * NU;
        io.thrust_keep = bp.thrust_keep + inst;
        io.kthr = bp.kthr[inst];            // (requested here, used at the step's very end)
        io.cmd_mass = bp.cmd_mass;
    }
}

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
// what tick_new_point works on, all of it requested at the kernel's very top (tick_early): the time, and the lane's share of the
// vehicle's two cached segment records (see tick_early)
typedef double tick_d2 __attribute__((ext_vector_type(2)));
// h0 / h1: (time_cum[i], time_cum[i + 1]), (time_seg[i], i) of slot 0 / 1; ca / cn: the lane's 8 coefficients in slot 0 / 1; tf: (end of the
// trajectory, the lane's component of final_pt)
struct TickEarly { double tv; tick_d2 h0[2], h1[2], ca[4], cn[4], tf; int v; double own, ownc; };   // own / ownc: word `lane` / constant `lane` of the EGO's record (carried over)
__device__ __forceinline__ TickEarly tick_early(const TickArgs &ta, int inst, int orow, int lane);
__device__ __forceinline__ double tick_new_point(const TickArgs &ta, const TickEarly &te, int inst, int lane, bool store, double xv[10],
                                                 double uv[4], double nbv[6], int &refill, double &cfill, double *stamps);
__device__ __forceinline__ void tick_arrived(TickEarly &te);
__device__ __forceinline__ void tick_cache_store(const TickArgs &ta, const TickEarly &te, int inst, int lane, int refill, double fill, double cfill);
__device__ __forceinline__ double tick_estimator(const TickArgs &ta, int inst, int B, int lane);

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

// Arguments a kernel needs LATE (the tick's estimator constants, the list's geometry for the new entry's store, the trajectory arrays
// of the rare slow path), fetched where they are used.  Read as ordinary members of `ka` the compiler requests every argument at the
// kernel's top and keeps it in scalar registers until its use: the tick kernels ran out of them (160 spills to / 740 reloads from
// vector-register lanes against 19 / 82 in the plain step -- with one wave per SIMD every one of those is time on the clock).  The
// pointer goes through an empty asm so that the loads cannot move up; they hit the scalar cache (the block was touched at the top).
struct KernargLate {
    const __attribute__((address_space(4))) unsigned *kp;
    __device__ __forceinline__ KernargLate()
    {
        kp = (const __attribute__((address_space(4))) unsigned *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
    }
    template <class T> __device__ __forceinline__ T get(unsigned off) const
    {
        static_assert(sizeof(T) % 4 == 0 && std::is_trivially_copyable<T>::value, "plain words only");
        unsigned w[sizeof(T) / 4];
#pragma unroll
        for (unsigned i = 0; i < sizeof(T) / 4; ++i) w[i] = kp[off / 4 + i];
        T t;
        __builtin_memcpy(&t, w, sizeof(T));
        return t;
    }
};
static_assert(offsetof(KernArgs, P) == 0, "WaveGfx950::late_params reads the parameter block at the start of the argument segment");
static_assert(std::is_standard_layout<KernArgs>::value && std::is_trivially_copyable<KernArgs>::value,
              "KernargLate addresses members of the one kernel argument by offsetof");
#define NDP_TA_LATE(L, f) ((L).template get<decltype(TickArgs::f)>((unsigned)(offsetof(KernArgs, ta) + offsetof(TickArgs, f))))
// (A pointer fetched this way has lost what the compiler knows of pointers in the argument block -- that they point to global memory --
// and is dereferenced with FLAT instructions, which also count as LDS operations and turn the waits behind them into full drains:
// fine on the rare paths; the common one goes through gptr.)
template <class T> using gptr = __attribute__((address_space(1))) T *;

// FUSED: the wave first predicts its own instance's disturbance force (gate + MLP over the N+1 <= 32 horizon rows,
// one 32x32 f32 MFMA tile) and leaves it in the LDS staging slot the RTI program reads f from -- no second
// launch and no trip of f through HBM.
// QMODE: 0 = the whole step in place; 1 / 2 = producer / consumer of the interior-point work list (see QueueArgs); 3 = in place, the
// lean program (RtiWave's LEAN: no stiff sweeps) -- the late-force step that shares the SIMDs with the next tick's downwash launch.
#ifndef NDP_RTI_ATTR       // kernel-development hook: extra attributes of rti_kernel (e.g. a register cap for occupancy studies)
#define NDP_RTI_ATTR
#endif
// TICK: the launch is a whole control tick of ndp_tick (see TickArgs): the wave makes its window's newest node -- and its neighbour's --
// itself and runs the estimator; instantiated for the reference configuration's in-place and producer forms only.
// The control step's statements are shared by rti_kernel and rti_sens_kernel through rti_kernel_body.inc (see there).
template <int NSLOT, int WAVES, bool FUSED, int NC = 0, int PREC = 0, int NRC = (NC ? 1 : 0), int QMODE = 0, bool TICK = false>
__global__ __launch_bounds__(64 * WAVES) NDP_RTI_ATTR void rti_kernel(KernArgs ka)
{
    constexpr bool SENS = false, PSENS = false;
    const SensArgs sa{};
    const PSensArgs pa{};
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ unsigned wg_done;     // prefetched-force launches: the workgroup's waves that hold their force values (see LateArgs)
#include "rti_kernel_body.inc"
}

// The control step with its initial-state sensitivities (ndp_sens_enable): three-slot shapes (N <= 27), qp_precision 0, one RTI iteration,
// in place or the work list's producer / consumer; the level (1 or 2) is a run-time uniform of SensArgs.
template <int WAVES, bool FUSED, int NC, int QMODE>
__global__ __launch_bounds__(64 * WAVES) void rti_sens_kernel(KernArgs ka, SensArgs sa)
{
    constexpr int NSLOT = 3, PREC = 0, NRC = NC ? 1 : 0;
    constexpr bool TICK = false, SENS = true, PSENS = false;
    const PSensArgs pa{};
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ unsigned wg_done;
#include "rti_kernel_body.inc"
}

// ... and also with its parameter sensitivities (ndp_sens_params_enable): du0/dxr, du0/dur, du0/df of the same QP, behind the x0 ones
// (level >= 1), for the same shapes but the unfused run-time horizon (k_rti: that instantiation came out with a scratch frame).
template <int WAVES, bool FUSED, int NC, int QMODE>
__global__ __launch_bounds__(64 * WAVES) void rti_psens_kernel(KernArgs ka, SensArgs sa, PSensArgs pa)
{
    constexpr int NSLOT = 3, PREC = 0, NRC = NC ? 1 : 0;
    constexpr bool TICK = false, SENS = true, PSENS = true;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ unsigned wg_done;
#include "rti_kernel_body.inc"
}

// What the three kernels below share in front of their own Io: the wave's instance (a ragged last workgroup: its spare waves leave), its
// views of the batch and its LDS, and the step's program.  Text, not a function (see rti_kernel_body.inc): a shared function changed all
// six kernels' code, and so did issuing the step's first loads in front of the Io instead of behind it, so that call stays with each kernel.
#define NDP_RECOMPUTE_PROLOGUE                                                                     \
    extern __shared__ __attribute__((aligned(16))) double smem[];                                  \
    const RtiParams &P = ka.P;                                                                     \
    const int waves = (int)(blockDim.x >> 6), wave = (int)(threadIdx.x >> 6);                      \
    const int inst = __builtin_amdgcn_readfirstlane((int)blockIdx.x * waves + wave);               \
    if (inst >= ka.B) return;                                                                      \
    const int N = NC ? NC : P.N;                                                                   \
    RtiIo io;                                                                                      \
    bind_instance(io, ka.bp, inst, N);                                                             \
    const int lpw = NC ? ((lds_doubles(NC) + 1) & ~1) : ka.lds_per_wave;                           \
    WaveGfx950::lds_ptr lds = (WaveGfx950::lds_ptr)(smem + (size_t)wave * lpw);                    \
    using Prog = RtiWave<WaveGfx950, 3, NC, true, NC ? 1 : 0>;

// The adjoint of the control step (ndp_step_vjp_device, RtiWave::vjp_out): the step's own program, recomputed from a caller's tape, then
// the adjoint of its last QP contracted with the caller's upstream gradients.  The tape (the iterate and kept set before the step) has been
// copied into the handle's VJP workspace by the host, so the recompute advances that copy: the kernel writes nothing but the workspace and
// its outputs.  Three slots (N <= 27), qp_precision 0, one RTI iteration, in place; the force read from global memory (fp32, or none).
// Instances per workgroup: blockDim.x / 64 (the handle's).  Not a row of k_rti: its own launcher (ndp_step_vjp_device).
struct VjpArgs {
    const double *gu0, *gX, *gU;
    double *gx0, *gxr, *gur, *gf;
};
template <int NC>
__global__ __launch_bounds__(256) void rti_vjp_kernel(KernArgs ka, VjpArgs va)
{
    NDP_RECOMPUTE_PROLOGUE
    const size_t i = (size_t)inst, nx = (size_t)(N + 1) * NX, nu = (size_t)N * NU, nf = (size_t)(N + 1) * 3;
    const VjpIo vo{va.gu0 ? va.gu0 + i * NU : nullptr, va.gX ? va.gX + i * nx : nullptr, va.gU ? va.gU + i * nu : nullptr,
                   va.gx0 ? va.gx0 + i * NX : nullptr, va.gxr ? va.gxr + i * nx : nullptr, va.gur ? va.gur + i * nu : nullptr,
                   va.gf ? va.gf + i * nf : nullptr};
    typename Prog::InBuf inb;
    double x0v;
    Prog::issue_first(P, io, inb, x0v);
    Prog::template run<false, true, false, false, true>(P, io, lds, inb, x0v, nullptr, nullptr, &vo);
}

// The same adjoint with the gradient in the cost weights and the mass beside it (ndp_step_vjp_model_device, RtiWave::vjp_out<true>):
// gmodel [B][16] = dL/dQd [10] | dL/dRd [4] | dL/dmass | 0, one row per instance (the caller sums over the batch: no atomic, two calls are
// bit-identical).  Kernels of their own, so that rti_vjp_kernel stays the code it was.
template <int NC>
__global__ __launch_bounds__(256) void rti_wvjp_kernel(KernArgs ka, VjpArgs va, double *gmodel)
{
    NDP_RECOMPUTE_PROLOGUE
    const size_t i = (size_t)inst, nx = (size_t)(N + 1) * NX, nu = (size_t)N * NU, nf = (size_t)(N + 1) * 3;
    const VjpIo vo{va.gu0 ? va.gu0 + i * NU : nullptr, va.gX ? va.gX + i * nx : nullptr, va.gU ? va.gU + i * nu : nullptr,
                   va.gx0 ? va.gx0 + i * NX : nullptr, va.gxr ? va.gxr + i * nx : nullptr, va.gur ? va.gur + i * nu : nullptr,
                   va.gf ? va.gf + i * nf : nullptr};
    typename Prog::InBuf inb;
    double x0v;
    Prog::issue_first(P, io, inb, x0v);
    Prog::template run<false, true, false, false, true, true>(P, io, lds, inb, x0v, nullptr, nullptr, &vo, gmodel + i * 16);
}

// The forward-mode derivative of the control step (ndp_step_jvp_device, RtiWave::jvp_out): the recompute of rti_vjp_kernel -- the same
// workspace, the same tape rules -- then one Riccati sweep per direction over the blocks the step left, n_tan directions per call.  The
// tangents and outputs are instance-major: instance i's T directions lie together.  Not a row of k_rti: ndp_step_jvp_device launches it.
struct JvpArgs {
    const double *tx0, *txr, *tur, *tf;
    double *du0, *dX, *dU;
    int T;
};
template <int NC>
__global__ __launch_bounds__(256) void rti_jvp_kernel(KernArgs ka, JvpArgs ja)
{
    NDP_RECOMPUTE_PROLOGUE
    const size_t i = (size_t)inst * (size_t)ja.T, nx = (size_t)(N + 1) * NX, nu = (size_t)N * NU, nf = (size_t)(N + 1) * 3;
    const JvpIo jo{ja.tx0 ? ja.tx0 + i * NX : nullptr, ja.txr ? ja.txr + i * nx : nullptr, ja.tur ? ja.tur + i * nu : nullptr,
                   ja.tf ? ja.tf + i * nf : nullptr, ja.du0 ? ja.du0 + i * NU : nullptr, ja.dX ? ja.dX + i * nx : nullptr,
                   ja.dU ? ja.dU + i * nu : nullptr, ja.T};
    typename Prog::InBuf inb;
    double x0v;
    Prog::issue_first(P, io, inb, x0v);
    Prog::template run<false, true, false, false, false, false, true>(P, io, lds, inb, x0v, nullptr, nullptr, nullptr, nullptr, &jo);
}

#undef NDP_RECOMPUTE_PROLOGUE

// test hook: one v_mfma_f64_16x16x4_f64 / v_mfma_f64_4x4x4_4b_f64 with caller-chosen per-lane operands (pins the register maps)
__global__ void mfma_probe_kernel(const double *a, const double *b, const double *c, double *d)
{
    const int l = (int)threadIdx.x;
    WaveGfx950::vd4 acc;
    for (int r = 0; r < 4; ++r) acc.r[r] = c[r * 64 + l];
    acc = WaveGfx950::mfma(a[l], b[l], acc);
    for (int r = 0; r < 4; ++r) d[r * 64 + l] = acc.r[r];
    d[256 + l] = WaveGfx950::readlane(a[l], 37) + WaveGfx950::wave_sum(b[l]) + WaveGfx950::wave_min(a[l]) + WaveGfx950::wave_max(a[l]);
    // the four-block v_mfma_f64_4x4x4_4b_f64 on the same operands (accumulator: c's first register) and the four row broadcasts
    d[320 + l] = WaveGfx950::mfma4(a[l], b[l], c[l]);
    d[384 + l] = WaveGfx950::rowb<0>(a[l]);
    d[448 + l] = WaveGfx950::rowb<1>(a[l]);
    d[512 + l] = WaveGfx950::rowb<2>(a[l]);
    d[576 + l] = WaveGfx950::rowb<3>(a[l]);
    // the row rotations that bring the packed -Lam^-1 of a stage to block 3 (rti_wave.hpp: linv_get)
    d[640 + l] = WaveGfx950::rowror4<1>(a[l]);
    d[704 + l] = WaveGfx950::rowror4<2>(a[l]);
    d[768 + l] = WaveGfx950::rowror4<3>(a[l]);
}

// test hook: one v_mfma_f32_16x16x4_f32 (mode 0) or one v_mfma_f32_16x16x16_bf16 (mode 1: four packed contraction steps)
// through the config-5 backends, caller-chosen per-lane operands a[4][64], b[4][64] (mode 0 uses row 0), c[4][64] -> d[4][64]
__global__ void mfma_probe32_kernel(const float *a, const float *b, const float *c, float *d, int mode)
{
    const int l = (int)threadIdx.x;
    WaveGfx950F32::md4 acc;
    for (int r = 0; r < 4; ++r) acc.r[r] = c[r * 64 + l];
    if (mode == 0) acc = WaveGfx950F32::mfma(a[l], b[l], acc);
    else {
        float av[4], bv[4];
        for (int i = 0; i < 4; ++i) { av[i] = a[i * 64 + l]; bv[i] = b[i * 64 + l]; }
        acc = WaveGfx950BF16::mfma_k(av, bv, 4, acc);
    }
    for (int r = 0; r < 4; ++r) d[r * 64 + l] = acc.r[r];
    // the row sum of the config-5 layout: lanes 4 apart inside a 16-lane row
    double x = (double)a[l];
    x = x + WaveGfx950F32::csum1(x);
    x = x + WaveGfx950F32::csum2(x);
    d[256 + l] = (float)x;
}

// behind the work list's consumer launch: the list is empty again for the next step's producer
__global__ void queue_reset_kernel(unsigned *count, unsigned long long *ipm_total)
{
    if (threadIdx.x == 0) {
        *ipm_total += *count;
        *count = 0u;
    }
}

// ------------------------------------------------------------------------------------------ MLP kernel
// nn_net.py:7-18: Linear(6,128) ReLU Linear(128,64) ReLU Linear(64,128) ReLU Linear(128,3), fp32.
// One wave = 32 horizon rows (columns of the MFMA tile); activations stay transposed [feature][row] in
// the accumulators: the 32x32 f32 accumulator holds feature (r&3)+8(r>>2)+4(lane>>5) of row lane&31 in
// register r, which is exactly the B-operand shape of the next layer's 32x32x2 step when that step
// contracts the feature pair {f0(r), f0(r)+4}.  The weights are pre-permuted on the host into that
// "fragment order" (one 64-float record per MFMA), so A operands are coalesced 256-byte loads.
// Fragment blob (built on the host by make_fragments, parked in LDS during the MLP phase), in float units:
//   FR_L1  12 x 64 f32     layer-1 A operands for v_mfma_f32_32x32x2_f32 (K = 6 inputs)
//   FR_B1/B2/B3, FR_W4 ([128 features][4]: w0 w1 w2 0), FR_B4
//   FR_HF  layers 2 and 3 as fp16 pairs: 32 records (16 per layer) x 2 splits (hi, lo * 2^11) x 64 lanes x 8 halves
// The blob is moved by LDS-DMA in 1-KB pieces (one global_load_lds_dwordx4 per wave): its size is a multiple of 256 floats.
enum { FR_L1 = 0, FR_B1 = FR_L1 + 12 * 64, FR_B2 = FR_B1 + 128, FR_B3 = FR_B2 + 64, FR_W4 = FR_B3 + 128,
       FR_B4 = FR_W4 + 4 * 128, FR_HF = FR_B4 + 4, FR_REC = 2 * 64 * 8 / 2 /* floats per record */,
       FR_USED = FR_HF + 32 * FR_REC,
       // (a multiple of 8 pieces: every wave of a 1- / 2- / 4- / 8-wave workgroup moves the SAME number of them -- see stage_fragments)
       FR_CHUNKS = (FR_USED + 2047) / 2048 * 8, FR_TOTAL = FR_CHUNKS * 256 };
static_assert(FR_HF % 4 == 0 && FR_W4 % 4 == 0, "16-byte alignment of the LDS image");
static_assert(FR_L1 == frag::L1 && FR_B1 == frag::B1 && FR_B2 == frag::B2 && FR_B3 == frag::B3 && FR_W4 == frag::W4 && FR_B4 == frag::B4 &&
              FR_HF == frag::HF && FR_REC == frag::REC && FR_TOTAL == frag::TOTAL, "mlp_common.hpp: frag:: restates this enum for mlp_vjp.hip");

// The four layers for one 32-row tile held by one wave.  zb[s] = input feature 2s + (lane>>5) of row lane&31;
// returns the three outputs of row lane&31 in o[] (both half-waves hold the full sums).

// The workgroup copies the fragment blob (FR_TOTAL floats, L2-resident) into LDS by LDS-DMA: each wave issues one
// global_load_lds_dwordx4 per 1-KB piece (64 lanes x 16 B, lane-linear destination), nothing passes through VGPRs and
// all pieces are in flight at once; the caller's __syncthreads() (which waits vmcnt(0)) retires them.  Through
// registers (global_load_dwordx4 + ds_write_b128 per thread and pass) the same copy took 7.5k cycles per workgroup.
// Streaming the weights per wave straight from L2 instead made 1024 waves fetch the same lines in lockstep (channel
// hot-spotting: the MLP tile took 33k cycles at B = 1024 against 25k alone).
__device__ __forceinline__ void stage_fragments(const float *__restrict__ fr, lds_f32 dst, int tid, int nthreads)
{
    // the wave index is uniform: keep the piece loop scalar (derived from threadIdx it would run under an exec mask), a
    // compile-time number of rounds with a uniform guard on the last one
    // The number of pieces per wave must not depend on the wave: with a guarded last round the compiler cannot count the transfers
    // in flight and makes the NEXT wait of the wave -- whatever it is for -- a wait for all of them (s_waitcnt vmcnt(0)); the one-launch
    // tick's polynomial work, meant to run under the transfer, then started behind it (+2 600 cycles per tick).
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nw = nthreads >> 6;
#pragma unroll
    for (int i = 0; i < FR_CHUNKS; ++i) {
        if (i * nw >= FR_CHUNKS) break;
        const int c = wave + i * nw;
        if ((i + 1) * nw <= FR_CHUNKS || c < FR_CHUNKS)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(fr + c * 256 + lane * 4),
                                             (__attribute__((address_space(3))) void *)(dst + c * 256), 16, 0, 0);
    }
}

__device__ __forceinline__ void load_w(lds_cf32 fr, int rec, int lane, Split2 &w)
{
    const __attribute__((address_space(3))) h16x8 *p = (const __attribute__((address_space(3))) h16x8 *)(fr + FR_HF) + rec * 128 + lane;
    w.hi = p[0]; w.lo = p[64];
}

// The four layers for one 32-row tile held by one wave.  zb[s] = input feature 2s + (lane>>5) of row lane&31;
// returns the three outputs of row lane&31 in o[] (both half-waves hold the full sums).
// Measured (scripts/ubench/mfma_f16_valu_overlap.hip, profiles/r02_ubench_mfma_f16_valu_overlap.txt): a wave's f32 VALU work is
// NOT hidden behind its own v_mfma_f32_32x32x16_f16 -- 35 cycles per instruction alone, 35 + 6 + 2.5 per v_fma_f32 issued
// behind it -- so a software-pipelined form of this tile (conversions of one layer issued between the matrix instructions
// of the next) ran no faster than this layer-by-layer form (9.46 k against 9.18 k cycles); what counts is the instruction
// count.  No scheduling fences here: the compiler's own order is 0.84 k cycles shorter than a fenced one.
// Activations stay transposed [feature][row] in the accumulators.  Registers 8s..8s+7 of a 32x32 accumulator,
// converted to fp16 pairs, ARE the B operand of k-step s of the next layer (feature 16s + 8(j>>2) + 4(lane>>5) + (j&3) in
// element j); the weights are stored in that k order.
__device__ __forceinline__ void mlp_tile(lds_cf32 fr, const float zb[3], int lane, float o[3])
{
    typedef float f4_t __attribute__((ext_vector_type(4)));
    const int h = lane >> 5;
    Split2 x1[4][2], x2[2][2];
    f16_t h3[4];
    float bc[16];
    // layer 1 (6 -> 128): exact f32 MFMA, K = 2 per instruction
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) {
#pragma unroll
        for (int r = 0; r < 16; ++r) bc[r] = fr[FR_B1 + ot * 32 + f0(r) + 4 * h];
        f16_t acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bc[r];        // the bias rides in the accumulator
#pragma unroll
        for (int s = 0; s < 3; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[FR_L1 + (ot * 3 + s) * 64 + lane], zb[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = relu_cap(acc[r]);
        split2(acc, 0, x1[ot][0]);
        split2(acc, 1, x1[ot][1]);
    }
    // layers 2 (128 -> 64) and 3 (64 -> 128) as one stream of 32 weight records, the next record requested before
    // the current record's six MFMAs issue
    Split2 wc, wn;
    load_w(fr, 0, lane, wc);
    f16_t acc, accl;
#pragma unroll
    for (int rec = 0; rec < 32; ++rec) {
        const bool l2 = rec < 16;
        const int q = l2 ? rec : rec - 16;
        const int ot = l2 ? q / 8 : q / 4, it = l2 ? (q / 2) % 4 : (q / 2) % 2, s = q % 2;
        const bool first = l2 ? (q % 8 == 0) : (q % 4 == 0), last = l2 ? (q % 8 == 7) : (q % 4 == 3);
        if (rec + 1 < 32) load_w(fr, rec + 1, lane, wn);
        if (first) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[r] = fr[(l2 ? FR_B2 : FR_B3) + ot * 32 + f0(r) + 4 * h];   // the bias rides in the accumulator
                accl[r] = 0.0f;
            }
        }
#ifdef NDP_DEV_HALF_TILE        // (measurement only: half of the tile's matrix instructions, wrong forces -- what a tile shared by two waves would cost at best)
        if (!(rec & 1))
#endif
        mm3(wc, l2 ? x1[it][s] : x2[it][s], acc, accl);
        if (last) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = fmaf(accl[r], NDP_LO_INV, acc[r]);
                acc[r] = l2 ? relu_cap(v) : fmaxf(v, 0.0f);
            }
            if (l2) { split2(acc, 0, x2[ot][0]); split2(acc, 1, x2[ot][1]); }
            else h3[ot] = acc;
        }
        wc = wn;
    }
    // last layer (128 -> 3) on the VALU in f32: each half-wave owns 64 of the 128 features of its row; weights come as
    // one 16-byte record per feature, the records of the next 16 features requested before the current ones are used
    const __attribute__((address_space(3))) f4_t *w4 = (const __attribute__((address_space(3))) f4_t *)(fr + FR_W4);
    f4_t qc[16], qn[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) qc[r] = w4[f0(r) + 4 * h];
    o[0] = o[1] = o[2] = 0.0f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        if (it + 1 < 4) {
#pragma unroll
            for (int r = 0; r < 16; ++r) qn[r] = w4[(it + 1) * 32 + f0(r) + 4 * h];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = fmaf(qc[r][c], h3[it][r], o[c]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) qc[r] = qn[r];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = o[c] + __shfl_xor(o[c], 32, 64) + fr[FR_B4 + c];
}

// Standalone form (DownwashNN.update for arbitrary row counts): one 32-row tile per wave, no tile loop --
// a loop would make every weight load loop-invariant and the compiler then tries to keep 17k weights in registers.
__global__ __launch_bounds__(256) void mlp_kernel(const float *__restrict__ fr, const double *__restrict__ other,
                                                  const double *__restrict__ ego, const double *__restrict__ ego_xy,
                                                  float *__restrict__ fout, int rows, int np1, double r2,
                                                  int other_stride, const int *__restrict__ other_index, int other_sys,
                                                  size_t other_pitch, size_t ego_pitch, size_t ego_xy_pitch)     // doubles per row of other / per instance of ego, ego_xy (see MlpArgs)
{
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ntiles = (rows + 31) / 32;
    const int tile = (int)blockIdx.x * 4 + wave;
    lds_f32 wl = (lds_f32)wsm;
    stage_fragments(fr, wl, (int)threadIdx.x, 256);
    __syncthreads();
    if (tile >= ntiles) return;
    const int row = tile * 32 + j;
    const bool valid = row < rows;
    const int rowc = valid ? row : rows - 1;
    const int inst = rowc / np1, k = rowc - inst * np1;
    const int orow = other_index ? other_index[inst] : inst;          // see MlpArgs
    const double *oth = other + (size_t)(orow < 0 ? 0 : orow) * other_pitch;
    bool open = valid && orow >= 0;
    if (ego_xy) {
        const double oxy[2] = {ld_other(oth, other_sys), ld_other(oth + 1, other_sys)};
        open = open && gate_open(oxy, ego_xy + (size_t)inst * ego_xy_pitch, r2);
    }
    // downwash_nn.py:22-23: (other - ego)[:, 0:6] in fp64, cast to fp32
    float zb[3], o[3];
#pragma unroll
    for (int s = 0; s < 3; ++s)
        zb[s] = (float)(ld_other(oth + (size_t)k * other_stride + 2 * s + h, other_sys) - ego[(size_t)inst * ego_pitch + (size_t)k * NX + 2 * s + h]);
    mlp_tile(wl, zb, lane, o);
    if (valid && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) fout[(size_t)row * 3 + c] = open ? o[c] : 0.0f;   // :75-76 zeros when gated off
    }
}

// ---- LDS-free form of the tile (measurement: downwash of the NEXT tick in a second stream beside the control-step kernel, which
// holds all of a CU's LDS and 320 of its 512 registers per lane).  The weight records come straight from global memory (L2),
// NPRE records requested ahead; biases, first- and last-layer weights likewise.  Same arithmetic, same fragment blob.
typedef const float *__restrict__ g_cf32;
__device__ __forceinline__ void load_w_g(g_cf32 fr, int rec, int lane, Split2 &w)
{
    const h16x8 *p = reinterpret_cast<const h16x8 *>(fr + FR_HF) + rec * 128 + lane;
    w.hi = p[0]; w.lo = p[64];
}

__device__ __forceinline__ void mlp_tile_stream(g_cf32 fr, const float zb[3], int lane, float o[3])
{
    typedef float f4_t __attribute__((ext_vector_type(4)));
    constexpr int NPRE = 2;
    const int h = lane >> 5;
    Split2 wq[NPRE];
#pragma unroll
    for (int i = 0; i < NPRE; ++i) load_w_g(fr, i, lane, wq[i]);        // in flight under layer 1
    Split2 x1[4][2], x2[2][2];
    const f4_t *w4 = reinterpret_cast<const f4_t *>(fr + FR_W4);
    o[0] = o[1] = o[2] = 0.0f;
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) {
        f16_t acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = fr[FR_B1 + ot * 32 + f0(r) + 4 * h];
#pragma unroll
        for (int s = 0; s < 3; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[FR_L1 + (ot * 3 + s) * 64 + lane], zb[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = relu_cap(acc[r]);
        split2(acc, 0, x1[ot][0]);
        split2(acc, 1, x1[ot][1]);
        __builtin_amdgcn_sched_barrier(0);     // keep the phases apart: left alone the scheduler hoists every later load up front (254 registers)
    }
    f16_t acc, accl;
#pragma unroll
    for (int rec = 0; rec < 32; ++rec) {
        const bool l2 = rec < 16;
        const int q = l2 ? rec : rec - 16;
        const int ot = l2 ? q / 8 : q / 4, it = l2 ? (q / 2) % 4 : (q / 2) % 2, s = q % 2;
        const bool first = l2 ? (q % 8 == 0) : (q % 4 == 0), last = l2 ? (q % 8 == 7) : (q % 4 == 3);
        const Split2 wc = wq[rec % NPRE];
        if (rec + NPRE < 32) load_w_g(fr, rec + NPRE, lane, wq[rec % NPRE]);
        if (first) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[r] = fr[(l2 ? FR_B2 : FR_B3) + ot * 32 + f0(r) + 4 * h];
                accl[r] = 0.0f;
            }
        }
        mm3(wc, l2 ? x1[it][s] : x2[it][s], acc, accl);
        if (last) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = fmaf(accl[r], NDP_LO_INV, acc[r]);
                acc[r] = l2 ? relu_cap(v) : fmaxf(v, 0.0f);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (l2) { split2(acc, 0, x2[ot][0]); split2(acc, 1, x2[ot][1]); }
            else {      // last layer (128 -> 3) on this output tile at once: its 32 hidden features need not stay live
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const f4_t qv = w4[ot * 32 + f0(r) + 4 * h];
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c] = fmaf(qv[c], acc[r], o[c]);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = o[c] + __shfl_xor(o[c], 32, 64) + fr[FR_B4 + c];
}

// one wave = one 32-row tile, four per workgroup, no LDS and no barrier, ~180 registers per lane (control step: 320 -- the two fit on
// a SIMD together; ensure_prefetch checks it).  proto != null: launch m of the prefetch protocol (see LateArgs).
__global__ __launch_bounds__(256)
void mlp_stream_kernel(const float *__restrict__ fr, const double *__restrict__ other, const double *__restrict__ ego,
                       const double *__restrict__ ego_xy, float *__restrict__ fout, float *__restrict__ fout1, int rows, int np1, double r2,
                       int other_stride, const int *__restrict__ other_index, unsigned long long *proto, int other_sys)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ntiles = (rows + 31) / 32;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= ntiles) return;
    unsigned long long m = 0;
    if (proto) {
        m = proto[PF_CUR_M];                        // written by the gate launch in front of this one (plain load)
        if (m & 1) fout = fout1;
    }
    const int row = tile * 32 + j;
    const bool valid = row < rows;
    const int rowc = valid ? row : rows - 1;
    const int inst = rowc / np1, k = rowc - inst * np1;
    const int orow = other_index ? other_index[inst] : inst;
    const double *oth = other + (size_t)(orow < 0 ? 0 : orow) * np1 * other_stride;
    bool open = valid && orow >= 0;
    if (ego_xy) {
        const double oxy[2] = {ld_other(oth, other_sys), ld_other(oth + 1, other_sys)};
        open = open && gate_open(oxy, ego_xy + inst * 2, r2);
    }
    float zb[3], o[3];
#pragma unroll
    for (int s = 0; s < 3; ++s)
        zb[s] = (float)(ld_other(oth + (size_t)k * other_stride + 2 * s + h, other_sys) - ego[(size_t)rowc * NX + 2 * s + h]);
    mlp_tile_stream(fr, zb, lane, o);
    if (!proto) {
        if (valid && h == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) fout[(size_t)row * 3 + c] = open ? o[c] : 0.0f;
        }
        return;
    }
    // the rows go out past this XCD's L2 (agent-scope stores: the reader runs on other XCDs, now), then -- once they are complete --
    // the tile's epoch word
    if (valid && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            __hip_atomic_store(reinterpret_cast<unsigned *>(fout) + (size_t)row * 3 + c, __float_as_uint(open ? o[c] : 0.0f),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // The rows were written THROUGH to memory (sc1 stores): what is needed before the epoch word goes out is their COMPLETION, i.e.
    // s_waitcnt vmcnt(0) -- stores of one wave to different addresses / channels may complete out of order.  Not an agent-scope
    // release: its buffer_wbl2 writes back the XCD's whole L2, the control step's dirty iterate included (one per wave, 672 per
    // launch, made the control step beside it 50 % slower).  And not a workgroup-scope release fence alone: on gfx950 it emits NO
    // vmcnt wait (the ISA had the three row stores followed directly by the epoch store) -- the wait is spelled out;
    // the fence stays as the compiler-level barrier.  scripts/isa_audit.py checks the instruction is there.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0)
        __hip_atomic_store(proto + PF_EPOCH + (m & 1) * (unsigned)ntiles + tile, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wave, in front of downwash launch m on the second stream: takes the number, waits until the control step that read force
// slot m & 1 last (number m - 2) holds its values, publishes the number for the launch behind it.  A single wave polling gently
// costs nothing (waves of the downwash kernel polling on every CU kept registers the next control-step workgroups needed).
__global__ void prefetch_gate_kernel(unsigned long long *proto, unsigned timeout_us, unsigned groups_rti)
{
    if (threadIdx.x != 0) return;
    const unsigned long long m = proto[PF_CUR_M] + 1;
    if (m > 2) {
        const unsigned long long want = (m - 2) * groups_rti;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(proto + PF_RTI_C2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
            __builtin_amdgcn_s_sleep(16);
            if (__builtin_amdgcn_s_memrealtime() - t0 > 100ull * timeout_us) {
                atomicAdd(reinterpret_cast<int *>(proto + PF_GATE_TIMEOUT), 1);
                break;
            }
        }
    }
    proto[PF_CUR_M] = m;
}

// behind downwash launch m in its stream: that launch is complete
__global__ void prefetch_done_kernel(unsigned long long *proto)
{
    if (threadIdx.x == 0) __hip_atomic_store(proto + PF_MLP_DONE, proto[PF_CUR_M], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// host: blob (W1 b1 W2 b2 W3 b3 W4 b4, row-major [out][in]) -> fragment order
static uint16_t f16_rn(float x)
{   // round-to-nearest-even f32 -> fp16 bits, subnormals included (the weights and their residuals are finite and small)
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t ax = u & 0x7FFFFFFFu;
    if (ax >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);               // >= 65536: inf (never for these data)
    if (ax < 0x33000000u) return sign;                                       // < 2^-25: 0
    const int e = (int)(ax >> 23) - 127;
    uint32_t m = (ax & 0x7FFFFFu) | 0x800000u;                               // 24-bit significand
    const int shift = e < -14 ? 13 + (-14 - e) : 13;                         // bits to drop (subnormal: more)
    const uint32_t keep = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    uint32_t r = keep + ((rem > half || (rem == half && (keep & 1u))) ? 1u : 0u);
    // normal: r has the hidden bit at position 10; adding the exponent field lets a mantissa carry roll into it
    const uint32_t bits = e < -14 ? r : (uint32_t)((e + 15 - 1) << 10) + r;
    return (uint16_t)(sign | bits);
}
static float f16_f32(uint16_t b)
{
    const uint32_t sign = (uint32_t)(b & 0x8000u) << 16, ex = (b >> 10) & 0x1Fu, mant = b & 0x3FFu;
    float x;
    if (ex == 0) {
        x = (float)mant * 5.9604644775390625e-08f;                           // 2^-24
        uint32_t u; memcpy(&u, &x, 4); u |= sign; memcpy(&x, &u, 4);
        return x;
    }
    const uint32_t u = sign | ((ex + 112u) << 23) | (mant << 13);
    memcpy(&x, &u, 4);
    return x;
}

static void make_fragments(const float *blob, std::vector<float> &fr)
{
    const float *W1 = blob, *b1 = W1 + 128 * 6, *W2 = b1 + 128, *b2 = W2 + 64 * 128;
    const float *W3 = b2 + 64, *b3 = W3 + 128 * 64, *W4 = b3 + 128, *b4 = W4 + 3 * 128;
    fr.assign(FR_TOTAL, 0.0f);
    for (int ot = 0; ot < 4; ++ot)
        for (int s = 0; s < 3; ++s)
            for (int l = 0; l < 64; ++l) fr[FR_L1 + (ot * 3 + s) * 64 + l] = W1[(ot * 32 + (l & 31)) * 6 + 2 * s + (l >> 5)];
    for (int i = 0; i < 128; ++i) fr[FR_B1 + i] = b1[i];
    for (int i = 0; i < 64; ++i) fr[FR_B2 + i] = b2[i];
    for (int i = 0; i < 128; ++i) fr[FR_B3 + i] = b3[i];
    for (int f = 0; f < 128; ++f)
        for (int c = 0; c < 3; ++c) fr[FR_W4 + f * 4 + c] = W4[c * 128 + f];
    for (int i = 0; i < 3; ++i) fr[FR_B4 + i] = b4[i];
    // layers 2, 3: record = (out tile, in tile, k-step); lane (r = l&31, h = l>>5) element j holds
    // W[ot*32 + r][it*32 + 16 s + 8 (j>>2) + 4 h + (j&3)] split into hi + lo / 2^11
    uint16_t *hf = reinterpret_cast<uint16_t *>(fr.data() + FR_HF);
    for (int rec = 0; rec < 32; ++rec) {
        const bool l2 = rec < 16;
        const int q = l2 ? rec : rec - 16;
        const int ot = l2 ? q / 8 : q / 4, it = l2 ? (q / 2) % 4 : (q / 2) % 2, s = q % 2;
        const float *W = l2 ? W2 : W3;
        const int nin = l2 ? 128 : 64;
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
                const int kin = it * 32 + 16 * s + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3);
                const float w = W[(ot * 32 + (l & 31)) * nin + kin];
                const uint16_t hi = f16_rn(w);
                const float r1 = w - f16_f32(hi);
                const uint16_t lo = f16_rn(r1 * NDP_LO_SCALE);
                uint16_t *rp = hf + (size_t)rec * 2 * 512;
                rp[0 * 512 + l * 8 + j] = hi;
                rp[1 * 512 + l * 8 + j] = lo;
            }
    }
}

// ------------------------------------------------------------------------------------------ f3 kernels
// Hover-throttle estimator (2-state Kalman filter on [f_collect, k_throttle] + Tustin differentiator), one thread
// per vehicle.  Elementwise and HBM-bound: state is SoA ([8][B] doubles) so every access is a coalesced 512-B wave
// load/store; 152 algorithmic bytes per vehicle and tick.  Operation order follows the reference's numpy
// expressions (hover_throttle_estimator.py:38-51) so results agree to rounding.

// Streaming (non-temporal) accesses of the rows' kernels: outputs nobody reads again in the same launch, inputs read once.  With plain
// stores ref_window_kernel ran at 0.45 of the HBM roof although its loads + arithmetic alone take 75 us and its arithmetic + stores
// alone 111 us of the 187 (knock-out builds, round 5): the 616 MB of window rows went through L2 as ordinary dirty lines and every
// wave's dependent load rounds queued behind them.  `nt`: 137 us (0.62).
typedef double nt_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_stream(double2 *p, const double2 &v)
{
    const nt_d2 t = {v.x, v.y};
    __builtin_nontemporal_store(t, reinterpret_cast<nt_d2 *>(p));
}
__device__ __forceinline__ void st_stream(double *p, double v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ double2 ld_stream(const double2 *p)
{
    const nt_d2 t = __builtin_nontemporal_load(reinterpret_cast<const nt_d2 *>(p));
    return make_double2(t.x, t.y);
}

// one estimator update of vehicle v (state SoA [8][S]); returns k_throttle
__device__ __forceinline__ double throttle_update_one(const ThrCfg &c, double *__restrict__ st, size_t S, int v, double vzv, double th)
{
    const double az = nc_add(nc_mul(c.a1, st[7 * S + v]), nc_mul(c.a2, vzv - st[6 * S + v]));   // differentiator.py:21
    st[6 * S + v] = vzv;
    st[7 * S + v] = az;
    double x1 = st[1 * S + v];
    if (0.1 < th && th < 1.0) {                                            // hover_throttle_estimator.py:40
        const double z = az + c.g;
        const double P11 = st[5 * S + v];
        // numpy evaluates these products without fused multiply-add: keep individually rounded operations
        const double p01 = nc_mul(th, P11), p10 = nc_mul(P11, th);
        const double p00 = nc_add(nc_mul(p01, th), c.Q0), p11 = nc_add(P11, c.Q1);
        const double inv = 1.0 / nc_add(nc_mul(nc_mul(c.hm, p00), c.hm), c.R);
        const double K0 = nc_mul(nc_mul(p00, c.hm), inv), K1 = nc_mul(nc_mul(p10, c.hm), inv);
        const double x0p = nc_mul(th, x1);
        const double innov = z - nc_mul(c.hm, x0p);
        st[0 * S + v] = nc_add(x0p, nc_mul(K0, innov));
        x1 = nc_add(x1, nc_mul(K1, innov));
        st[1 * S + v] = x1;
        const double i00 = 1.0 - nc_mul(K0, c.hm), i10 = -nc_mul(K1, c.hm);
        st[2 * S + v] = nc_mul(i00, p00);
        st[3 * S + v] = nc_mul(i00, p01);
        st[4 * S + v] = nc_add(nc_mul(i10, p00), p10);
        st[5 * S + v] = nc_add(nc_mul(i10, p01), p11);
    }
    return x1;
}

__global__ __launch_bounds__(256) void throttle_kernel(ThrCfg c, double *__restrict__ st, const double *__restrict__ vz,
                                                       const double *__restrict__ throttle, double *__restrict__ k_out, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    k_out[v] = throttle_update_one(c, st, (size_t)B, v, vz[v], throttle[v]);
}

__global__ __launch_bounds__(256) void throttle_reset_kernel(double *st, double k_init, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    const size_t S = (size_t)B;
    st[0 * S + v] = 0.0; st[1 * S + v] = k_init;
    st[2 * S + v] = 1.0; st[3 * S + v] = 0.0; st[4 * S + v] = 0.0; st[5 * S + v] = 1.0;
    st[6 * S + v] = 0.0; st[7 * S + v] = 0.0;
}

// nmpc_u_2_att_tgt (nmpc_node.py:273-283): body rates pass through, thrust = c * mass / k_throttle (0 if k == 0)
__device__ __forceinline__ double thrust_cmd(double c, double mass, double k) { return k != 0.0 ? nc_mul(c, mass) / k : 0.0; }
__global__ __launch_bounds__(256) void actuator_kernel(const double *__restrict__ u0, const double *__restrict__ k,
                                                       double *__restrict__ cmd, double mass, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    const double2 a = reinterpret_cast<const double2 *>(u0)[2 * v], b = reinterpret_cast<const double2 *>(u0)[2 * v + 1];
    const double kk = k[v];
    double2 o0 = a, o1 = b;
    o1.y = thrust_cmd(b.y, mass, kk);
    reinterpret_cast<double2 *>(cmd)[2 * v] = o0;
    reinterpret_cast<double2 *>(cmd)[2 * v + 1] = o1;
}

// ------------------------------------------------------------------------------------------ f2 kernels
// AlphaFilter per instance and axis (alpha_filter.py:19; individually rounded like the Python expression)
__global__ __launch_bounds__(256) void relay_formation_kernel(double alpha, double *__restrict__ st, const double *__restrict__ form, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    const bool init = st[v * 4 + 3] != 0.0;
    const double oma = 1.0 - alpha;
    for (int a = 0; a < 3; ++a) {
        const double u = form[v * 3 + a];
        const double y = init ? st[v * 4 + a] : u;
        st[v * 4 + a] = nc_add(nc_mul(alpha, y), nc_mul(oma, u));
    }
    st[v * 4 + 3] = 1.0;
}

// follower reference = leader window with the filtered offset added to the positions.  HBM-bound: 3360 B per instance at N = 20.
// A dense copy in 16-byte pieces (piece p: row p / 5, doubles 2 (p % 5) and + 1 of it), the offset added to pieces 0 (x, y) and 1 (z):
// every instruction of a wave covers 1 KB of contiguous memory on both sides, the output streams (st_stream).  As one thread per ROW
// -- five pieces at an 80-byte lane stride -- each instruction touched 40 lines a fifth each: 195 us for 262 144 windows (0.58 of the
// roof); that form with streaming loads / stores: 685 us, every partial line fetched again by each of its five instructions.
enum { RELAY_UNROLL = 4 };
__global__ __launch_bounds__(256) void relay_reference_kernel(const double *__restrict__ st, const double *__restrict__ xr_lead,
                                                              double *__restrict__ xr_out, int rows, int np1)
{
    const size_t total = (size_t)rows * 5;
    const size_t p0 = (size_t)blockIdx.x * (256 * RELAY_UNROLL) + threadIdx.x;
    const double2 *src = reinterpret_cast<const double2 *>(xr_lead);
    double2 *dst = reinterpret_cast<double2 *>(xr_out);
    double2 v[RELAY_UNROLL], o[RELAY_UNROLL];
#pragma unroll
    for (int j = 0; j < RELAY_UNROLL; ++j) {
        const size_t p = p0 + (size_t)j * 256, pc = p < total ? p : total - 1;
        const int r = (int)(pc / 5), c = (int)(pc - (size_t)r * 5), inst = r / np1;
        v[j] = src[pc];
        o[j] = make_double2(0.0, 0.0);
        if (c == 0) o[j] = *reinterpret_cast<const double2 *>(st + (size_t)inst * 4);        // (ox, oy)
        else if (c == 1) o[j].x = st[(size_t)inst * 4 + 2];                                   // (oz, -)
    }
#pragma unroll
    for (int j = 0; j < RELAY_UNROLL; ++j) {
        const size_t p = p0 + (size_t)j * 256;
        const int c = (int)(p % 5);
        double2 w = v[j];
        if (c == 0) { w.x += o[j].x; w.y += o[j].y; }
        else if (c == 1) w.x += o[j].x;
        if (p < total) st_stream(dst + p, w);
    }
}

// ------------------------------------------------------------------------------------------ f4 kernel
// plant: the OCP's own dynamics (nmpc_body_rate_ctl.py:147-158 + f/mass), RK4 substeps, quaternion renormalised
__device__ __forceinline__ void plant_f(const double *x, const double *u, const double *acc, double *d)
{
    const double qw = x[6], qx = x[7], qy = x[8], qz = x[9];
    d[0] = x[3]; d[1] = x[4]; d[2] = x[5];
    d[3] = 2.0 * (qx * qz + qw * qy) * u[3] + acc[0];
    d[4] = 2.0 * (qy * qz - qw * qx) * u[3] + acc[1];
    d[5] = (1.0 - 2.0 * qx * qx - 2.0 * qy * qy) * u[3] + acc[2];
    d[6] = (-u[0] * qx - u[1] * qy - u[2] * qz) * 0.5;
    d[7] = (u[0] * qw + u[2] * qy - u[1] * qz) * 0.5;
    d[8] = (u[1] * qw - u[2] * qx + u[0] * qz) * 0.5;
    d[9] = (u[2] * qw + u[1] * qx - u[0] * qy) * 0.5;
}

__global__ __launch_bounds__(256) void plant_kernel(double *__restrict__ x, const double *__restrict__ u, const double *__restrict__ f,
                                                    double h, int sub, double inv_mass, double g, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    double xv[10], uv[4], acc[3] = {0.0, 0.0, -g};
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double2 t = reinterpret_cast<const double2 *>(x)[(size_t)v * 5 + i];
        xv[2 * i] = t.x; xv[2 * i + 1] = t.y;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double2 t = reinterpret_cast<const double2 *>(u)[(size_t)v * 2 + i];
        uv[2 * i] = t.x; uv[2 * i + 1] = t.y;
    }
    if (f) { acc[0] = f[v * 3] * inv_mass; acc[1] = f[v * 3 + 1] * inv_mass; acc[2] = f[v * 3 + 2] * inv_mass - g; }
    for (int s = 0; s < sub; ++s) {
        double k1[10], k2[10], k3[10], k4[10], xs[10];
        plant_f(xv, uv, acc, k1);
#pragma unroll
        for (int i = 0; i < 10; ++i) xs[i] = xv[i] + 0.5 * h * k1[i];
        plant_f(xs, uv, acc, k2);
#pragma unroll
        for (int i = 0; i < 10; ++i) xs[i] = xv[i] + 0.5 * h * k2[i];
        plant_f(xs, uv, acc, k3);
#pragma unroll
        for (int i = 0; i < 10; ++i) xs[i] = xv[i] + h * k3[i];
        plant_f(xs, uv, acc, k4);
#pragma unroll
        for (int i = 0; i < 10; ++i) xv[i] += h / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
    }
    const double n = sqrt(xv[6] * xv[6] + xv[7] * xv[7] + xv[8] * xv[8] + xv[9] * xv[9]);
#pragma unroll
    for (int i = 6; i < 10; ++i) xv[i] /= n;
#pragma unroll
    for (int i = 0; i < 5; ++i) reinterpret_cast<double2 *>(x)[(size_t)v * 5 + i] = make_double2(xv[2 * i], xv[2 * i + 1]);
}

// ------------------------------------------------------------------------------------------ f1 kernel
// Reference window generation (the step before the path): per vehicle a piecewise polynomial trajectory
// (TrajCoefficients.msg) is evaluated at the N+1 node times t + k*dt and pushed through the differential-flatness map;
// what NMPCRefPublisher.get_nmpc_pts returns (pt_pub/pt_publisher.py:79-103, base_pt_publisher.py:81-133,
// diff_flatness :188-248, traj_full_pt_2_x_u :115-146).  One thread per (vehicle, node): reads its segment's 28
// coefficients (224 contiguous bytes, shared by the neighbouring nodes of the vehicle), writes 80 + 32 contiguous bytes.

// Value and first ND - 1 derivatives of sum_i c[i] s^i at s by repeated synthetic division (the Taylor shift): pass k divides the
// previous pass's quotient by (x - s) once more and leaves p^(k)(s) / k! -- NC_ - 1 - k fused multiply-adds, 22 for the four values of
// a septic against 43 when every derivative is a Horner pass of its own with the factors i (i-1) .. applied on the way
// (get_poly_params + _get_output_value, base_pt_publisher.py:102-133, polym_optimizer.py:104-139, evaluate every power, factor and
// term separately: ~160 multiplies and adds per reference point).  out[k] = p^(k)(s) / k!.
// Measured (round 3): folding factors and 1 / tseg^d into per-derivative coefficient blocks on the host (1 operation per
// coefficient, but 85 instead of 28 loads per point) made the kernel SLOWER: the loads cost more than the arithmetic saved.
template <int NC_, int ND>
__device__ __forceinline__ void taylor_shift(const double *__restrict__ c, double s, double out[ND])
{
    double b[NC_];
#pragma unroll
    for (int i = 0; i < NC_; ++i) b[i] = c[i];
#pragma unroll
    for (int k = 0; k < ND; ++k) {
#pragma unroll
        for (int i = NC_ - 2; i >= k; --i) b[i] = fma(b[i + 1], s, b[i]);
        out[k] = b[k];
    }
}

// ---- one reference point, in three pieces shared by every kernel that makes one (so that they all make the SAME point, bit for bit:
// the control step that computes its window's newest node itself -- rti_kernel<..., TICK> -- must agree with the list kernels):
//   seg_locate   which polynomial segment holds trajectory time t (base_pt_publisher.py:93-100)
//   traj_chain   one of the 14 polynomial values of a trajectory point: p / v / a / j of one axis, yaw, yaw rate (:102-133)
//   flatness_xu  the differential-flatness map of the point (pt_publisher.py:188-248) and the x / u packing (:115-146)
// seg_hint (or null): the vehicle's segment at its previous point -- control ticks move forward 20 ms at a time, so it is nearly always
// still the one: two loads confirm it instead of a search over time_cum.  Returns -1 past the end of the trajectory.
__device__ __forceinline__ int seg_locate(int n_seg, const double *__restrict__ tc, double t, int hint)
{
    if (t >= tc[n_seg]) return -1;                        // base_pt_publisher.py:93-94: hover at final_pt after the end
    int idx = hint < 0 ? 0 : (hint >= n_seg ? n_seg - 1 : hint);
    if ((idx == 0 || !(tc[idx] > t)) && tc[idx + 1] > t) return idx;
    // :100: first i with time_cum[i] > t, minus one -- time_cum ascends, so that is (entries of 0 .. n_seg-1 not above t) - 1.
    // Counted eight independent loads at a time: a search loop is a chain of dependent global loads, ~0.6 us each.
    idx = 0;
    for (int i = 0; i < n_seg; i += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = tc[i + j < n_seg ? i + j : n_seg];
#pragma unroll
        for (int j = 0; j < 8; ++j) idx += (i + j < n_seg && !(v[j] > t)) ? 1 : 0;
    }
    return idx > 0 ? idx - 1 : 0;
}

// value number c of a trajectory point at normalised segment time s; its = 1 / time_seg: c = 3 d + axis (d = derivative 0..3,
// axis 0..2) for c < 12, c = 12: yaw, c = 13: yaw rate.  ca = the value's own polynomial: chain_base(c) doubles into the segment's
// record of 28 coefficients, x(8) y(8) z(8) yaw(4).
__device__ __forceinline__ int chain_base(int c) { return c >= 12 ? 24 : 8 * (c % 3); }
// p, v, a, j of one axis (ca: its 8 coefficients) / yaw, yaw rate (ca: the 4 yaw coefficients): derivative d carries d! / time_seg^d
__device__ __forceinline__ void traj_axis(const double *__restrict__ ca, double s, double its, double out[4])
{
#pragma clang fp contract(off)
    double tl[4];
    taylor_shift<8, 4>(ca, s, tl);
    const double its2 = its * its;
    out[0] = tl[0]; out[1] = tl[1] * its; out[2] = tl[2] * (2.0 * its2); out[3] = tl[3] * (6.0 * (its2 * its));
}
__device__ __forceinline__ void traj_yaw(const double *__restrict__ ca, double s, double its, double out[2])
{
#pragma clang fp contract(off)
    double tl[2];
    taylor_shift<4, 2>(ca, s, tl);
    out[0] = tl[0]; out[1] = tl[1] * its;
}
__device__ __forceinline__ double traj_chain(const double *__restrict__ ca, int c, double s, double its)
{
    if (c >= 12) {
        double y[2];
        traj_yaw(ca, s, its, y);
        return c == 12 ? y[0] : y[1];
    }
    double v[4];
    traj_axis(ca, s, its, v);
    const int d = c / 3;
    return d == 0 ? v[0] : (d == 1 ? v[1] : (d == 2 ? v[2] : v[3]));
}

// ---- f64 helpers of the flatness map.  An IEEE divide or square root is a ~30-instruction dependent chain on gfx950 and the map
// has four and three of them, one behind the other, plus a library sincos (~150 instructions with its large-argument path): measured
// in the one-launch tick, where a single wave runs the map with nothing to overlap it, ~4 000 cycles of a 7 300-cycle prologue; in the
// list / window kernels the same chains are why "HBM-bound" kernels sat at 0.4 of the HBM roof.  These are seed + Newton forms
// (v_rcp_f64 / v_rsq_f64: 2^-26 relative or better; two steps -> ~1e-16, not correctly rounded) and a Cody-Waite sincos with the
// fdlibm kernel polynomials (|error| < 1 ulp for |x| < 1e5) -- deterministic, shared by every kernel that makes a reference point.
__device__ __forceinline__ double rcp_n(double a)
{
    double r = __builtin_amdgcn_rcp(a);
    r = fma(fma(-a, r, 1.0), r, r);
    r = fma(fma(-a, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ double rsqrt_n(double a)
{
#pragma clang fp contract(off)
    double y = __builtin_amdgcn_rsq(a);
    y = fma(y * 0.5, fma(-a * y, y, 1.0), y);
    y = fma(y * 0.5, fma(-a * y, y, 1.0), y);
    return y;
}
__device__ __forceinline__ void sincos_n(double x, double *sn, double *cs)
{
#pragma clang fp contract(off)
    const double k = rint(x * 6.36619772367581382433e-01);            // x * 2 / pi
    double r = fma(-k, 1.57079632673412561417e+00, x);                // pi / 2 in three pieces (fdlibm e_rem_pio2: pio2_1, pio2_2, pio2_3)
    r = fma(-k, 6.07710050630396597660e-11, r);
    r = fma(-k, 2.02226624871116645580e-21, r);
    const double z = r * r;
    // fdlibm k_sin / k_cos on |r| <= pi / 4
    const double ps = fma(z, fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08), 2.75573137070700676789e-06),
                                        -1.98412698298579493134e-04), 8.33333333332248946124e-03), -1.66666666666666324348e-01);
    const double s0 = fma(z * r, ps, r);
    const double pc = fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09), -2.75573143513906633035e-07),
                                        2.48015872894767294178e-05), -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    const double c0 = fma(z * z, pc, fma(-0.5, z, 1.0));
    const int q = (int)k & 3;
    const double s1 = (q & 1) ? c0 : s0, c1 = (q & 1) ? s0 : c0;
    *sn = (q & 2) ? -s1 : s1;
    *cs = ((q + 1) & 2) ? -c1 : c1;
}

// Every product-sum below is written out (fma where one is wanted, contraction off otherwise): the compiler's own choice of which
// multiplies to fuse depends on the surrounding code, and two kernels must not differ in the last bit of a reference point.
__device__ __forceinline__ void flatness_xu(double mass, double g, const double pvaj[12], double yaw, double yawd, double xv[10], double uv[4])
{
#pragma clang fp contract(off)
    const double td[3] = {pvaj[6], pvaj[7], pvaj[8] + g};
    const double tn2 = fma(td[0], td[0], fma(td[1], td[1], td[2] * td[2]));
    const double rtn = rsqrt_n(tn2), tn = tn2 * rtn;
    const double zb[3] = {td[0] * rtn, td[1] * rtn, td[2] * rtn};
    double sy, cy;
    sincos_n(yaw, &sy, &cy);
    // z_b x x_c with x_c = [cos yaw, sin yaw, 0]
    const double zx[3] = {-(zb[2] * sy), zb[2] * cy, fma(zb[0], sy, -(zb[1] * cy))};
    const double rnzx = rsqrt_n(fma(zx[0], zx[0], fma(zx[1], zx[1], zx[2] * zx[2])));
    const double yb[3] = {zx[0] * rnzx, zx[1] * rnzx, zx[2] * rnzx};
    const double xb[3] = {fma(yb[1], zb[2], -(yb[2] * zb[1])), fma(yb[2], zb[0], -(yb[0] * zb[2])), fma(yb[0], zb[1], -(yb[1] * zb[0]))};
    const double zj = fma(zb[0], pvaj[9], fma(zb[1], pvaj[10], zb[2] * pvaj[11]));
    double ho[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) ho[i] = rtn * fma(-zj, zb[i], pvaj[9 + i]);      // mass / u1 = 1 / |t_des|
    const double wp = -fma(ho[0], yb[0], fma(ho[1], yb[1], ho[2] * yb[2]));
    const double wq = fma(ho[0], xb[0], fma(ho[1], xb[1], ho[2] * xb[2]));
    const double wr = yawd * zb[2];
    // tf.transformations.quaternion_from_matrix on [x_b y_b z_b] (ROS geometry; restated): R[i][0..2] = xb[i], yb[i], zb[i]
    const double R[3][3] = {{xb[0], yb[0], zb[0]}, {xb[1], yb[1], zb[1]}, {xb[2], yb[2], zb[2]}};
    // (q[3] = w; i = index of the largest diagonal entry, j = i + 1, k = i + 2 mod 3.  Written with selects over the three cases:
    // dynamically indexed local arrays live in scratch memory on this target.)
    double q0, q1, q2, q3, tt = R[0][0] + R[1][1] + R[2][2] + 1.0;
    if (tt > 1.0) {
        q3 = tt; q2 = R[1][0] - R[0][1]; q1 = R[0][2] - R[2][0]; q0 = R[2][1] - R[1][2];
    } else {
        const bool c1 = R[1][1] > R[0][0];
        const bool c2 = R[2][2] > (c1 ? R[1][1] : R[0][0]);
        // case (i, j, k) = (0,1,2), (1,2,0), (2,0,1)
        const double t0 = R[0][0] - (R[1][1] + R[2][2]) + 1.0, t1 = R[1][1] - (R[2][2] + R[0][0]) + 1.0, t2 = R[2][2] - (R[0][0] + R[1][1]) + 1.0;
        const double s01 = R[0][1] + R[1][0], s12 = R[1][2] + R[2][1], s20 = R[2][0] + R[0][2];
        const double d21 = R[2][1] - R[1][2], d02 = R[0][2] - R[2][0], d10 = R[1][0] - R[0][1];
        tt = c2 ? t2 : (c1 ? t1 : t0);
        q0 = c2 ? s20 : (c1 ? s01 : t0);       // q[i] = tt, q[j] = R[i][j] + R[j][i], q[k] = R[k][i] + R[i][k]
        q1 = c2 ? s12 : (c1 ? t1 : s01);
        q2 = c2 ? t2 : (c1 ? s12 : s20);
        q3 = c2 ? d10 : (c1 ? d02 : d21);      // q[3] = R[k][j] - R[j][k]
    }
    const double qs = 0.5 * rsqrt_n(tt);
    // [qw, qx, qy, qz] (pt_publisher.py:237-240, :115-128); u = [p, q, r, collective_force / mass] (:138-145)
    xv[0] = pvaj[0]; xv[1] = pvaj[1]; xv[2] = pvaj[2]; xv[3] = pvaj[3]; xv[4] = pvaj[4]; xv[5] = pvaj[5];
    xv[6] = q3 * qs; xv[7] = q0 * qs; xv[8] = q1 * qs; xv[9] = q2 * qs;
    uv[0] = wp; uv[1] = wq; uv[2] = wr; uv[3] = tn;            // collective_force / mass = (|t_des| mass) / mass (:138-145)
}

// One reference point: trajectory of vehicle b at trajectory time t -> x[10] = [p, v, qw, qx, qy, qz], u[4] = [wx, wy, wz, c]
// (get_traj_pt, base_pt_publisher.py:81-133; diff_flatness, pt_publisher.py:188-248; traj_full_pt_2_x_u, :115-146)
__device__ __forceinline__ void ref_point(const RefCfg &cf, const double *__restrict__ coeff, const double *__restrict__ tcum,
                                          const double *__restrict__ tseg, const double *__restrict__ fpt, int b, double t,
                                          double xv[10], double uv[4], int *__restrict__ seg_hint = nullptr)
{
    const double *tc = tcum + (size_t)b * (cf.n_seg + 1);
    double pvaj[12], yaw = 0.0, yawd = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) pvaj[i] = 0.0;
    const int idx = seg_locate(cf.n_seg, tc, t, seg_hint ? seg_hint[b] : 0);
    if (idx < 0) {
        for (int i = 0; i < 3; ++i) pvaj[i] = fpt[(size_t)b * 3 + i];
    } else {
        if (seg_hint) seg_hint[b] = idx;
        const double its = rcp_n(tseg[(size_t)b * cf.n_seg + idx]);
        // the record as 14 16-byte loads (it starts at a multiple of 224 bytes): the load unit's time per instruction does not depend
        // on the width, and these rows are bound by the number of load instructions (see ref_window_kernel)
        double rec[28];
        {
            const double2 *r2 = reinterpret_cast<const double2 *>(coeff + ((size_t)b * cf.n_seg + idx) * 28);
#pragma unroll
            for (int i = 0; i < 14; ++i) { const double2 v = r2[i]; rec[2 * i] = v.x; rec[2 * i + 1] = v.y; }
        }
        double s;
        {
#pragma clang fp contract(off)
            s = (t - tc[idx]) * its;                      // :102-103
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double v[4];
            traj_axis(rec + 8 * a, s, its, v);
            pvaj[a] = v[0]; pvaj[3 + a] = v[1]; pvaj[6 + a] = v[2]; pvaj[9 + a] = v[3];
        }
        double y[2];
        traj_yaw(rec + 24, s, its, y);
        yaw = y[0]; yawd = y[1];
    }
    flatness_xu(cf.mass, cf.g, pvaj, yaw, yawd, xv, uv);
}

#define REF_ROWS 64     // rows (vehicle, node) per workgroup = one wave: small batches spread over all CUs
// What binds it (round 5, knock-out builds at 262 144 windows, 187 us as it stood): loads + arithmetic alone 75 us, arithmetic + stores
// alone 111 us (5.5 TB/s of writes: the device's fill ceiling), loads + stores WITHOUT the arithmetic 168 us -- the two memory phases
// did not overlap across waves: the 616 MB of output went through L2 as ordinary dirty lines and the dependent load rounds of the
// other waves (time -> segment -> coefficients) queued behind them.  Streaming stores (st_stream): 127-137 us, 0.62-0.68 of the roof.
// Not what binds it, each measured: the number of load instructions (coefficients as 14 16-byte loads: +2.6 %; from the scalar
// cache instead, a timing experiment: nothing), the number of dependent rounds (a branch-free scan that merges two of the three rounds
// but requests six more time_cum entries: 13 % SLOWER), occupancy (64 registers for 8 waves spills and is slower).  ONE 5 KB staging
// buffer used twice (x rows, then u rows): 7 KB per wave had capped a CU at 22 workgroups.
__global__ __launch_bounds__(REF_ROWS)
void ref_window_kernel(RefCfg cf, const double *__restrict__ coeff, const double *__restrict__ tcum,
                       const double *__restrict__ tseg, const double *__restrict__ fpt,
                       const double *__restrict__ tq, double *__restrict__ xr, double *__restrict__ ur)
{
    // Each lane produces 80 + 32 contiguous bytes; written directly that is a 16-byte store at an 80-byte lane stride
    // (one fifth of every cache line per instruction).  The wave's rows are contiguous in xr (and, minus the node-N
    // rows, in ur), so the outputs are transposed through LDS and leave as dense 1024-byte wave stores.
    __shared__ __attribute__((aligned(16))) double sx[REF_ROWS * 10];
    const int lane = (int)threadIdx.x;
    const int row0 = (int)blockIdx.x * REF_ROWS;
    const int np1 = cf.N + 1, nrows = cf.B * np1;
    const int row = row0 + lane < nrows ? row0 + lane : nrows - 1;      // tail lanes recompute the last row, never store
    const int b = row / np1, k = row - b * np1;
    const double t = (tq ? tq[b] : 0.0) + cf.toff + k * cf.dt;
    double xv[10], uv[4];
    ref_point(cf, coeff, tcum, tseg, fpt, b, t, xv, uv);
#pragma unroll
    for (int i = 0; i < 5; ++i) reinterpret_cast<double2 *>(sx)[lane * 5 + i] = make_double2(xv[2 * i], xv[2 * i + 1]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const int rows_here = nrows - row0 < REF_ROWS ? nrows - row0 : REF_ROWS;
    // 16 bytes per lane and store (rows are 80 / 32 bytes: both arrays stay 16-byte aligned at every row)
    double2 *xg = reinterpret_cast<double2 *>(xr + (size_t)row0 * 10);
    const double2 *s2 = reinterpret_cast<const double2 *>(sx);
    for (int i = lane; i < rows_here * 5; i += REF_ROWS) st_stream(xg + i, s2[i]);
    // ur has no node-N rows: the number of u rows before row (b, k) is b N + k = row - b
    const int ufirst = row0 - row0 / np1;
    const int uslot = (row - b) - ufirst;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();                                        // every lane has read its x pieces: the buffer is free
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (k < cf.N && row0 + lane < nrows) {
        reinterpret_cast<double2 *>(sx)[uslot * 2] = make_double2(uv[0], uv[1]);
        reinterpret_cast<double2 *>(sx)[uslot * 2 + 1] = make_double2(uv[2], uv[3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const int rend = row0 + rows_here;
    const int nu = (rend - rend / np1) - ufirst;                                 // u rows among [row0, rend)
    double2 *ug = reinterpret_cast<double2 *>(ur + (size_t)ufirst * 4);
    for (int i = lane; i < nu * 2; i += REF_ROWS) st_stream(ug + i, s2[i]);
}

// ---- f1, the reference's own bookkeeping: NMPCRefPublisher keeps a list of `ring` = step N + 1 reference points per vehicle,
// ts_nmpc apart (pt_publisher.py:36-38, params/nmpc_params.py:40-43; step = 5); every control tick drops the oldest and appends
// the point at ros_t + T_horizon (:78-97); the controller's window is every step-th entry (:99-103).
// Device layout (round 5): the window of tick n is the list entries with ABSOLUTE index n, n + step, .., n + step N (entry j =
// the j-th point ever put into the list) -- all of one residue class mod step.  So the list is kept PHASE-MAJOR, a short ring of
// N + 1 positions per phase, every entry stored twice, N + 1 positions apart:
//     x ring [B][step][2 (N+1)][10]      u ring [B][step][2 (N+1)][4]
//     entry j -> phase j % step, positions (j / step) % (N+1) and + (N+1)
// and every window is N + 1 CONTIGUOUS x rows (N u rows) starting at position (n / step) % (N+1) of phase n % step: the control
// step reads its reference window -- and a neighbour's -- straight out of the list (instance pitch = RingGeom::px / pu doubles),
// there is no window copy on the control tick's path, and the stand-alone window call is a dense copy.  `n` lives on the host
// (ndp_handle::list_n) and is baked into each launch's arguments.

__device__ __forceinline__ void ring_store(const RingGeom &rg, double *__restrict__ rx, double *__restrict__ ru, int b,
                                           unsigned long long j, const double xv[10], const double uv[4])
{
    const size_t s = rg.slot(j);
    double2 *x0 = reinterpret_cast<double2 *>(rx + (size_t)b * rg.px() + s * 10), *x1 = x0 + (size_t)rg.np1 * 5;
    double2 *u0 = reinterpret_cast<double2 *>(ru + (size_t)b * rg.pu() + s * 4), *u1 = u0 + (size_t)rg.np1 * 2;
#pragma unroll
    for (int c = 0; c < 5; ++c) { const double2 v = make_double2(xv[2 * c], xv[2 * c + 1]); x0[c] = v; x1[c] = v; }
#pragma unroll
    for (int c = 0; c < 2; ++c) { const double2 v = make_double2(uv[2 * c], uv[2 * c + 1]); u0[c] = v; u1[c] = v; }   // (plain: 80- / 32-byte pieces, partial lines -- streamed they cost the list advance a quarter of its rate)
}

// Fills list entries: point i of vehicle b at trajectory time (tq ? tq[b] : 0) + toff + i * tstep becomes entry j0 + i;
// dup0 also makes point 0 entry j0 - 1 (_gen_long_list_w_traj's duplicate, :73-74).
__global__ __launch_bounds__(256) void ref_list_fill_kernel(RefCfg cf, const double *__restrict__ coeff, const double *__restrict__ tcum,
                                                            const double *__restrict__ tseg, const double *__restrict__ fpt,
                                                            const double *__restrict__ tq, double tstep, int npts, unsigned long long j0,
                                                            RingGeom rg, int dup0, double *__restrict__ rx, double *__restrict__ ru)
{
    const int id = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (id >= cf.B * npts) return;
    const int b = id / npts, i = id - b * npts;
    double xv[10], uv[4];
    // one point per vehicle = the per-tick advance: the segment hint applies (it lives behind final_pt, see ndp_ref_set_trajectory)
    int *hint = npts == 1 ? reinterpret_cast<int *>(const_cast<double *>(fpt + (size_t)cf.B * 3 + (size_t)cf.B * SEGC_PER)) : nullptr;
    ref_point(cf, coeff, tcum, tseg, fpt, b, (tq ? tq[b] : 0.0) + cf.toff + i * tstep, xv, uv, hint);
    ring_store(rg, rx, ru, b, j0 + (unsigned long long)i, xv, uv);
    if (dup0 && i == 0) ring_store(rg, rx, ru, b, j0 - 1, xv, uv);
}

// gen_fix_pt_ref (pt_publisher.py:40-55): every entry = the odometry state, u = [0, 0, 0, c_hover]; one thread per stored row
__global__ __launch_bounds__(256) void ref_list_fix_kernel(const double *__restrict__ x_odom, double c_hover, int B, RingGeom rg,
                                                           double *__restrict__ rx, double *__restrict__ ru)
{
    const int per = rg.step * 2 * rg.np1;
    const int id = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (id >= B * per) return;
    const int b = id / per;
    const double2 *s = reinterpret_cast<const double2 *>(x_odom) + (size_t)b * 5;
    double2 *dx = reinterpret_cast<double2 *>(rx) + (size_t)id * 5, *du = reinterpret_cast<double2 *>(ru) + (size_t)id * 2;
#pragma unroll
    for (int c = 0; c < 5; ++c) dx[c] = s[c];
    du[0] = make_double2(0.0, 0.0);
    du[1] = make_double2(0.0, c_hover);
}

// get_nmpc_ref_from_long_list (:99-103) as a stand-alone call: the window of tick n -> xr[B][N+1][10], ur[B][N][4].  Both sides
// are contiguous per vehicle (see RingGeom): a dense copy, 16 bytes per lane -- 5 (N+1) + 2 N pieces per vehicle.
enum { WIN_UNROLL = 4 };      // 16-byte pieces per thread, a block apart: four loads in flight per lane before the first store
__global__ __launch_bounds__(256) void ref_list_window_kernel(const double *__restrict__ rx, const double *__restrict__ ru, RingGeom rg,
                                                              unsigned long long n, int B, double *__restrict__ xr, double *__restrict__ ur)
{
    const int N = rg.np1 - 1, nxp = 5 * rg.np1, per = nxp + 2 * N;
    const size_t total = (size_t)B * per, s = rg.slot(n);
    const size_t id0 = (size_t)blockIdx.x * (256 * WIN_UNROLL) + threadIdx.x;
    double2 v[WIN_UNROLL];
    double2 *dst[WIN_UNROLL];
#pragma unroll
    for (int j = 0; j < WIN_UNROLL; ++j) {
        const size_t id = id0 + (size_t)j * 256;
        const size_t idc = id < total ? id : total - 1;
        const int b = (int)(idc / per), e = (int)(idc - (size_t)b * per);
        const double2 *src = e < nxp ? reinterpret_cast<const double2 *>(rx + (size_t)b * rg.px() + s * 10) + e
                                     : reinterpret_cast<const double2 *>(ru + (size_t)b * rg.pu() + s * 4) + (e - nxp);
        dst[j] = id < total ? (e < nxp ? reinterpret_cast<double2 *>(xr) + (size_t)b * nxp + e
                                       : reinterpret_cast<double2 *>(ur) + (size_t)b * 2 * N + (e - nxp)) : nullptr;
        v[j] = *src;
    }
#pragma unroll
    for (int j = 0; j < WIN_UNROLL; ++j)
        if (dst[j]) st_stream(dst[j], v[j]);
}


// ------------------------------------------------------------------------------------------ the node's control tick (ndp_tick)
// nmpc_node.py:211-231 for every vehicle of the handle, on the device, references resident: per tick the host hands over the
// odometry states (80 B per vehicle) and a few scalars; everything else the tick needs is already in HBM.
//   tick_pre_kernel  (one thread per vehicle): the reference list's advance -- the point at t + T_horizon becomes the list's newest
//                    entry (get_nmpc_pts, pt_publisher.py:79-97), which is also node N of this tick's window -- and the hover-
//                    throttle estimator's update (hover_throttle_callback, nmpc_node.py:251-253) from vz and the thrust command of
//                    the previous tick
//   rti_kernel       the control step: x0 = the odometry rows, xr / ur / the neighbour's window straight out of the list; its last
//                    store is nmpc_u_2_att_tgt (:273-283): [wx, wy, wz, c mass / k_throttle] where the host reads it (RtiIo::cmd),
//                    the thrust kept on the device for the next estimator update.  (A third launch for that -- tick_post_kernel,
//                    the first form -- cost 4.6 us per tick in the trace for 32 bytes per vehicle.)

__global__ __launch_bounds__(64) void tick_pre_kernel(TickPre a)
{
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= a.cf.B) return;
    double vzv = 0.0, th = 0.0;
    if (a.est) { vzv = a.vz[(size_t)b * a.vz_pitch]; th = a.throttle[b]; }      // (requested before the polynomial work)
    if (a.advance) {
        double xv[10], uv[4];
        const int N = a.rg.np1 - 1;
        const double2 *src = reinterpret_cast<const double2 *>(a.rx + (size_t)b * a.rg.px() + a.pv_slot * 10);
        double2 *dst = reinterpret_cast<double2 *>(a.pv) + (size_t)b * a.rg.np1 * 3;
        if (a.pv) {                    // nodes 0 .. N-1 lie in the list since earlier ticks: copied under the polynomial work
#pragma unroll 4
            for (int k = 0; k < N; ++k) {
                const double2 v0 = src[k * 5], v1 = src[k * 5 + 1], v2 = src[k * 5 + 2];
                dst[k * 3] = v0; dst[k * 3 + 1] = v1; dst[k * 3 + 2] = v2;
            }
        }
        ref_point(a.cf, a.coeff, a.tcum, a.tseg, a.fpt, b, (a.t ? a.t[b] : a.t_all) + a.cf.toff, xv, uv, a.seg_hint);
        ring_store(a.rg, a.rx, a.ru, b, a.j_new, xv, uv);
        if (a.pv) {                    // node N: the point itself (not read back)
            dst[N * 3] = make_double2(xv[0], xv[1]); dst[N * 3 + 1] = make_double2(xv[2], xv[3]); dst[N * 3 + 2] = make_double2(xv[4], xv[5]);
        }
    }
    if (a.est) (void)throttle_update_one(a.thr, a.st, (size_t)a.cf.B, b, vzv, th);
}

// ---- the one-launch tick's prologue (rti_kernel<..., TICK>, see TickArgs), one wave per vehicle
// Lanes 0..13 evaluate the 14 polynomial values of the ego's new point (value c on lane c: the same traj_chain a list kernel calls),
// lanes 16..21 the position / velocity values of the neighbour's (orow >= 0); the values are collected with v_readlane and every lane
// runs the flatness map on them (uniform values: as long as one lane's work).  Lanes 0..13 then store the entry into the list (both
// copies), for the ticks to come.  x_new / u_new / nb_new are the same in every lane.
__device__ __forceinline__ double uniform_lane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// A per-vehicle cache of the trajectory's CURRENT and NEXT segment records, 2 x 32 doubles at segc + SEGC_PER v:
//     [0] time_cum[i]  [1] time_cum[i + 1]  [2] time_seg[i]  [3] i  [4 .. 31] the 28 coefficients of segment i
// and behind them [64 + 2 a], [65 + 2 a] = (time_cum[n_seg], final_pt[a]) for the axes a = 0..2 (one 16-byte load per lane)
// Found through the trajectory arrays a point costs two dependent memory round trips (segment index -> record), ~1 700 cycles
// each and nothing in the wave to hide them under; the cache's address depends on the vehicle only, so its loads are the launch's
// first and arrive under the weight transfer.  A vehicle moves on to its next segment every time_seg / 20 ms ticks (and in a batch
// of a thousand some vehicle does in every tick): that is slot 1, valid from the moment slot 0 was; the wave that crosses re-fills
// both slots -- one load per lane, requested in the prologue, stored behind the MLP phase (tick_cache_store), off everybody's
// critical path.  Anything else (the first tick after ndp_ref_set_trajectory -- the cache starts as NaNs --, a jump in time) takes
// seg_locate and the trajectory arrays, and re-fills the cache the same way.
__device__ __forceinline__ TickEarly tick_early(const TickArgs &ta, int inst, int orow, int lane)
{
    TickEarly te;
    const int c = (lane & 15) < 14 ? (lane & 15) : 13, q = (4 + chain_base(c)) >> 1;
    te.v = ((lane >> 4) & 1) && orow >= 0 ? orow : inst;
    // The load unit takes 16 cycles per instruction and wave of 64 (four lanes a cycle, whatever the width), and the four waves of a
    // compute unit share it: as 35 8-byte loads by all 64 lanes these requests alone kept it busy for 2 200 cycles.  Hence 16-byte
    // loads (13 of them) and only the 24 lanes whose values are looked at (lanes 0..13 ego, 16..21 neighbour).
    const tick_d2 *s0 = reinterpret_cast<const tick_d2 *>(ta.segc + (size_t)te.v * SEGC_PER);
    te.tv = ta.t_all;
    if (lane < 24) {
        te.h0[0] = s0[0]; te.h0[1] = s0[1]; te.h1[0] = s0[SEGC_SLOT / 2]; te.h1[1] = s0[SEGC_SLOT / 2 + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = q + (c >= 12 ? (k & 1) : k);
            te.ca[k] = s0[o]; te.cn[k] = s0[SEGC_SLOT / 2 + o];
        }
        te.tf = s0[SEGC_SLOT + (c < 3 ? c : 0)];
    }
    // the ego's whole record, word `lane` (and constant `lane` in lanes 0..5): carried over into the copy the NEXT tick reads
    te.own = ta.segc[(size_t)inst * SEGC_PER + lane];
    te.ownc = ta.segc[(size_t)inst * SEGC_PER + 2 * SEGC_SLOT + (lane < 6 ? lane : 5)];
    if (lane < 24) {
        // (written as a branch: as a select the compiler picks between two ADDRESSES -- the argument's copy parked in scratch memory
        // for it -- and loads through a flat pointer)
        if (ta.t) te.tv = ta.t[te.v];
    }
    return te;
}

// Consume everything tick_early requested, HERE.  While an LDS-DMA transfer (global_load_lds) is in flight the compiler cannot use the
// in-order load counter: the instruction counts as "may touch memory AND LDS", and from its issue to the next full drain every wait of
// the wave -- for whatever value -- is emitted as s_waitcnt vmcnt(0), i.e. a wait for the whole 72-KB weight transfer.  Left to its
// first use inside tick_new_point the cached records therefore "arrived" only when the transfer was complete (6 400 cycles after
// entry; requested at 1 000) and the polynomial work ran BEHIND the transfer instead of under it.  Waiting for them in front of the
// transfer costs the transfer a later start (the records' own latency) and takes the polynomial work off the critical path.
__device__ __forceinline__ void tick_arrived(TickEarly &te)
{
    asm volatile("" : "+v"(te.tv), "+v"(te.h0[0]), "+v"(te.h0[1]), "+v"(te.h1[0]), "+v"(te.h1[1]), "+v"(te.tf), "+v"(te.own), "+v"(te.ownc));
    asm volatile("" : "+v"(te.ca[0]), "+v"(te.ca[1]), "+v"(te.ca[2]), "+v"(te.ca[3]), "+v"(te.cn[0]), "+v"(te.cn[1]), "+v"(te.cn[2]), "+v"(te.cn[3]));
}

// returns (in every lane) the value lane l must store into the ego's cache word l behind the MLP phase, valid if refill != 0
// store: false in the idle waves of a ragged last workgroup (they shadow the last instance for the barriers' sake and must not write)
__device__ __forceinline__ double tick_new_point(const TickArgs &ta, const TickEarly &te, int inst, int lane, bool store, double xv[10],
                                                 double uv[4], double nbv[6], int &refill, double &cfill, double *stamps)
{
    // profiling hook (ndp_debug_stamps): slots 17.. = the prologue's own timeline; each stamp waits for the value it names
    auto stamp_after = [&](int idx, double dep) {
        if (NDP_RARELY(stamps != nullptr)) {
            unsigned long long tk;
            asm volatile("s_nop 0\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tk) : "v"(dep) : "memory");
            if (lane == 0) stamps[idx] = (double)tk;
        }
    };
    const int c = (lane & 15) < 14 ? (lane & 15) : 13;
    const int v = te.v;
    const int S = ta.n_seg;
    const double lo0 = te.h0[0][0], hi0 = te.h0[0][1], ts0 = te.h0[1][0], i0 = te.h0[1][1];
    const double lo1 = te.h1[0][0], hi1 = te.h1[0][1], ts1 = te.h1[1][0], i1 = te.h1[1][1];
    stamp_after(17, lo0 + te.cn[3][1] + te.tf[1]);                    // the cached records are there
    const double t = te.tv + ta.toff;
    stamp_after(18, t);                                               // the time is there
    bool past = t >= te.tf[0];                                        // base_pt_publisher.py:93-94: hover at final_pt after the end
    // (the same tests as seg_locate's: segment 0 also serves times in front of time_cum[0]; a NaN bound -- the empty cache -- fails all three)
    const bool in0 = (i0 == 0.0 || !(lo0 > t)) && hi0 > t, in1 = !in0 && !(lo1 > t) && hi1 > t;
    const bool slow = lane < 24 && !past && !in0 && !in1;            // (lanes 24..63 hold nothing: tick_early)
    int idx = (int)(in0 ? i0 : i1);
    double tcs = in0 ? lo0 : lo1, tsg = in0 ? ts0 : ts1, fp = te.tf[1];
    // (opaque to the optimiser: left visible as "a loaded value or, on the slow path, another load", it parks the cached values in
    // scratch memory to select between ADDRESSES and load through a flat pointer)
    asm volatile("" : "+v"(tcs), "+v"(tsg), "+v"(fp));
    double ca[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ca[i] = in1 ? te.cn[i >> 1][i & 1] : te.ca[i >> 1][i & 1];
    if (slow) {                                                       // (rare; per lane) through the trajectory arrays
        const KernargLate L;
        const double *tc = NDP_TA_LATE(L, tcum) + (size_t)v * (S + 1);
        const int cb = chain_base(c);
        idx = seg_locate(S, tc, t, -1);
        if (idx < 0) {                                                // (an empty cache does not know where the trajectory ends)
            past = true;
            idx = S - 1;
            fp = NDP_TA_LATE(L, fpt)[(size_t)v * 3 + (c < 3 ? c : 0)];
        } else {
            tcs = tc[idx]; tsg = NDP_TA_LATE(L, tseg)[(size_t)v * S + idx];
            const double *r = NDP_TA_LATE(L, coeff) + ((size_t)v * S + idx) * 28 + cb;
#pragma unroll
            for (int i = 0; i < 8; ++i) ca[i] = r[c >= 12 ? (i & 3) : i];
        }
    }
    double val = 0.0;
    if (past) {
        if (c < 3) val = fp;
    } else {
        const double its = rcp_n(tsg);
        double s;
        {
#pragma clang fp contract(off)
            s = (t - tcs) * its;
        }
        val = traj_chain(ca, c, s, its);
    }
    // the ego's cache: re-filled by this wave when its point did not come out of slot 0 (lane 0 belongs to the ego's group)
    refill = __builtin_amdgcn_readlane((in1 || slow) ? 1 : 0, 0);
    double fill = 0.0;
    cfill = te.ownc;
    if (refill) {
        const int ie = __builtin_amdgcn_readlane(idx, 0);
        const int sl = lane >> 5, f = lane & 31, i = ie + sl < S ? ie + sl : S - 1;
        const KernargLate L;
        const double *tce = NDP_TA_LATE(L, tcum) + (size_t)inst * (S + 1), *fpt = NDP_TA_LATE(L, fpt);
        cfill = lane < 6 ? ((lane & 1) ? fpt[(size_t)inst * 3 + (lane >> 1)] : tce[S]) : 0.0;   // (constants of the trajectory; stored by tick_cache_store)
        fill = f == 0 ? tce[i] : (f == 1 ? tce[i + 1] : (f == 2 ? NDP_TA_LATE(L, tseg)[(size_t)inst * S + i] : (f == 3 ? (double)i
                 : NDP_TA_LATE(L, coeff)[((size_t)inst * S + i) * 28 + (f - 4)])));
        if (ie + sl >= S && f == 1) fill = -1.0e300;                  // no segment behind the last one: slot 1 never matches (hi <= any t)
    }
    stamp_after(19, val);                                             // the lane's polynomial value
    double pvaj[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) pvaj[i] = uniform_lane(val, i);
    const double yaw = uniform_lane(val, 12), yawd = uniform_lane(val, 13);
#pragma unroll
    for (int i = 0; i < 6; ++i) nbv[i] = uniform_lane(val, 16 + i);
    stamp_after(20, pvaj[11] + nbv[5] + yawd);                        // collected over the lanes
    // where the entry goes (lane l: element l of x | u): the list's geometry is a late argument, requested HERE so that its fetch passes
    // under the flatness map instead of standing between the map and the barrier (-390 cycles per tick)
    gptr<double> dst;
    size_t mirror;
    {
        const KernargLate L;
        const size_t sl = NDP_TA_LATE(L, new_slot);
        const RingGeom rg = NDP_TA_LATE(L, rg);
        dst = (gptr<double>)(lane < 10 ? NDP_TA_LATE(L, rx) + (size_t)inst * rg.px() + sl * 10 + lane
                                       : NDP_TA_LATE(L, ru) + (size_t)inst * rg.pu() + sl * 4 + (lane - 10));
        mirror = (size_t)rg.np1 * (lane < 10 ? 10 : 4);
    }
    flatness_xu(ta.mass, ta.g, pvaj, yaw, yawd, xv, uv);
    stamp_after(21, xv[9] + uv[0]);                                   // flatness map done
    // the entry, for the windows of the ticks to come: element l of x | u from lane l
    // (v_writelane of the uniform values: written as a chain of selects on the lane id the compiler builds a table in scratch memory)
    int elo = 0, ehi = 0;
#pragma unroll
    for (int i = 0; i < 14; ++i) {
        const double w = i < 10 ? xv[i] : uv[i - 10];
        const int wl = __builtin_amdgcn_readfirstlane(__double2loint(w)), wh = __builtin_amdgcn_readfirstlane(__double2hiint(w));
        asm("v_writelane_b32 %0, %1, %2" : "+v"(elo) : "s"(wl), "n"(i));
        asm("v_writelane_b32 %0, %1, %2" : "+v"(ehi) : "s"(wh), "n"(i));
    }
    const double e = __hiloint2double(ehi, elo);
    if (store && lane < 14) {
        dst[0] = e;
        dst[mirror] = e;
    }
    return fill;
}

// The cache has two copies.  A launch READS one (its own record and its neighbour's, at entry) and WRITES the other -- every vehicle's
// record, every advancing tick: re-filled when the vehicle crossed into its next segment, carried over otherwise -- and the host swaps
// them between ticks.  (With one copy written in place, the neighbour's wave -- another workgroup, possibly another XCD, possibly a later
// round of a batch larger than the device -- could read a record while its owner re-filled it in the same launch: old header, new
// coefficients.  Nothing orders two workgroups of one launch; a kernel boundary orders everything.)
__device__ __forceinline__ void tick_cache_store(const TickArgs &ta, const TickEarly &te, int inst, int lane, int refill, double fill, double cfill)
{
    ta.segc_wr[(size_t)inst * SEGC_PER + lane] = refill ? fill : te.own;
    if (lane < 6) ta.segc_wr[(size_t)inst * SEGC_PER + 2 * SEGC_SLOT + lane] = cfill;
}

// hover_throttle_callback (nmpc_node.py:251-253) of this vehicle, by lane 0; returns k_throttle to every lane
__device__ __forceinline__ double tick_estimator(const TickArgs &ta, int inst, int B, int lane)
{
    double k = 0.0;
    const KernargLate L;
    if (lane == 0) k = throttle_update_one(NDP_TA_LATE(L, thr), NDP_TA_LATE(L, st), (size_t)B, inst, NDP_TA_LATE(L, vz)[(size_t)inst * NDP_TA_LATE(L, vz_pitch)],
                                           NDP_TA_LATE(L, throttle)[inst]);
    return uniform_lane(k, 0);
}

}  // namespace ndp

// ------------------------------------------------------------------------------------------ C-ABI
using namespace ndp;

// RTI_K(...): the rti_kernel instantiation to reference.  -DNDP_DEV_HEADLINE_ONLY (kernel development builds only, never
// the shipped library) collapses every instantiation but the reference configuration's two onto rti_kernel<3, 4, false, 20>, so
// that an experiment on the headline kernel compiles in 20 s instead of 3 min; such a library serves N = 20, n_rti = 1 only.
#ifdef NDP_DEV_HEADLINE_ONLY
template <int NSLOT, int WAVES, bool FUSED, int NC = 0, int PREC = 0, int NRC = (NC ? 1 : 0), int QMODE = 0, bool TICK = false>
#ifndef NDP_DEV_QMODE      // 1: study the work list's producer form (no interior-point code) in place of the in-place kernel
#define NDP_DEV_QMODE 0
#endif
struct RtiK { static constexpr auto fn = rti_kernel<3, (WAVES == 2 && NC == 20 ? 2 : 4), (FUSED && NC == 20 && QMODE == 0), 20, 0, 1, NDP_DEV_QMODE, (TICK && NC == 20 && QMODE == 0)>; };
#define RTI_K(...) (RtiK<__VA_ARGS__>::fn)
template <int WAVES, bool FUSED, int NC, int QMODE>
struct RtiSensK { static constexpr auto fn = rti_sens_kernel<4, (FUSED && NC == 20 && QMODE == 0), 20, NDP_DEV_QMODE>; };
#define RTI_SENS_K(...) (RtiSensK<__VA_ARGS__>::fn)
template <int WAVES, bool FUSED, int NC, int QMODE>
struct RtiPSensK { static constexpr auto fn = rti_psens_kernel<4, (FUSED && NC == 20 && QMODE == 0), 20, NDP_DEV_QMODE>; };
#define RTI_PSENS_K(...) (RtiPSensK<__VA_ARGS__>::fn)
#elif defined(NDP_DEV_COND_ONLY)
// compile / register studies of the condensed study kernels: every instantiation collapses onto rti_kernel<5, 1, false, 0, 5 or 6>
template <int NSLOT, int WAVES, bool FUSED, int NC = 0, int PREC = 0, int NRC = (NC ? 1 : 0), int QMODE = 0, bool TICK = false>
struct RtiK { static constexpr auto fn = rti_kernel<5, 1, false, 0, (PREC == 6 ? 6 : 5)>; };
#define RTI_K(...) (RtiK<__VA_ARGS__>::fn)
template <int WAVES, bool FUSED, int NC, int QMODE>       // (and the sensitivity kernels onto one)
struct RtiSensK { static constexpr auto fn = rti_sens_kernel<4, false, 20, 0>; };
#define RTI_SENS_K(...) (RtiSensK<__VA_ARGS__>::fn)
template <int WAVES, bool FUSED, int NC, int QMODE>
struct RtiPSensK { static constexpr auto fn = rti_psens_kernel<4, false, 20, 0>; };
#define RTI_PSENS_K(...) (RtiPSensK<__VA_ARGS__>::fn)
#elif defined(NDP_DEV_N40_ONLY)
// register studies of config 5's shape (scripts/dev_regs.sh): every instantiation collapses onto rti_kernel<5, 2, false, 40, 0, 2, NDP_DEV_QMODE>
#ifndef NDP_DEV_QMODE
#define NDP_DEV_QMODE 0
#endif
template <int NSLOT, int WAVES, bool FUSED, int NC = 0, int PREC = 0, int NRC = (NC ? 1 : 0), int QMODE = 0, bool TICK = false>
struct RtiK { static constexpr auto fn = rti_kernel<5, 2, false, 40, 0, 2, NDP_DEV_QMODE>; };
#define RTI_K(...) (RtiK<__VA_ARGS__>::fn)
template <int WAVES, bool FUSED, int NC, int QMODE>       // (and the sensitivity kernels onto one)
struct RtiSensK { static constexpr auto fn = rti_sens_kernel<4, false, 20, 0>; };
#define RTI_SENS_K(...) (RtiSensK<__VA_ARGS__>::fn)
template <int WAVES, bool FUSED, int NC, int QMODE>
struct RtiPSensK { static constexpr auto fn = rti_psens_kernel<4, false, 20, 0>; };
#define RTI_PSENS_K(...) (RtiPSensK<__VA_ARGS__>::fn)
#else
#define RTI_K(...) (rti_kernel<__VA_ARGS__>)
// RTI_SENS_K / RTI_PSENS_K(WAVES, FUSED, NC, QMODE): the rti_sens_kernel / rti_psens_kernel instantiation to reference (collapsed like
// RTI_K in development builds)
#define RTI_SENS_K(...) (rti_sens_kernel<__VA_ARGS__>)
#define RTI_PSENS_K(...) (rti_psens_kernel<__VA_ARGS__>)
#endif

// ---- host pack threads.  A host-array step first moves the caller's (pageable) arrays into a page-locked mirror the kernel can
// read; at batch 1024 that is 4.2 MB per step -- 56 us for one core, 26-30 us for eight (measured), against ~100 us for the
// kernel that then pulls them over PCIe.  The mirror is filled by a few persistent threads and the caller, a chunk
// (<= PACK_CHUNK bytes) at a time.
// len bytes as they lie, or -- rows > 0 -- `rows` rows of `len` bytes each taken from rows src_stride bytes apart (the neighbour
// windows: the 6 position / velocity columns of every 10-column row, all the gate and the network read)
struct PackJob { unsigned char *dst; const unsigned char *src; size_t len; size_t rows = 0, src_stride = 0; };
enum : size_t { PACK_CHUNK = (size_t)256 << 10 };
struct PackPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<const PackJob *> jobs{nullptr};
    std::atomic<int> njobs{0}, next{0}, active{0};
    std::unique_ptr<std::atomic<int>[]> done;
    int done_cap = 0;
    uint64_t gen = 0;
    std::atomic<uint64_t> gen_pub{0};   // gen, readable without the lock (the workers' polling phase)
    bool stop = false;
    static void cpu_relax()
    {
#if !defined(__HIP_DEVICE_COMPILE__) && (defined(__x86_64__) || defined(__i386__))
        __asm__ __volatile__("pause");
#endif
    }

    explicit PackPool(int n)
    {
        for (int i = 0; i < n; ++i) th.emplace_back([this] { work(); });
    }
    ~PackPool()
    {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        for (auto &t : th) t.join();
    }
    bool take_one()
    {   // njobs is published last (release) and read first (acquire): a thread that sees a job count sees that list and its flags
        const int n = njobs.load(std::memory_order_acquire);
        if (n == 0) return false;
        const int i = next.fetch_add(1, std::memory_order_acq_rel);
        if (i >= n) return false;
        const PackJob &j = jobs.load(std::memory_order_relaxed)[i];
        if (j.rows == 0) memcpy(j.dst, j.src, j.len);
        else
            for (size_t r = 0; r < j.rows; ++r) memcpy(j.dst + r * j.len, j.src + r * j.src_stride, j.len);
        done[i].store(1, std::memory_order_release);
        return true;
    }
    void drain() { while (take_one()) {} }
    void work()
    {
        uint64_t seen = 0;
        for (;;) {
            // back-to-back steps: the next job list arrives within microseconds -- poll for it a short while (a futex wake-up
            // costs 30-60 us per thread) before going to sleep on the condition variable (a 50 Hz control loop sleeps)
            for (int spin = 0; spin < 20000 && gen_pub.load(std::memory_order_acquire) == seen; ++spin) cpu_relax();
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
                active.fetch_add(1, std::memory_order_acq_rel);   // under the lock: post() cannot miss a worker that saw this generation
            }
            drain();
            active.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
    // hands the job list to the workers; the caller then consumes done[i] in order (wait_job) and must call finish()
    void post(const PackJob *j, int n)
    {
        if (n > done_cap) { done.reset(new std::atomic<int>[n]); done_cap = n; }
        for (int i = 0; i < n; ++i) done[i].store(0, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> lk(mu);
            jobs.store(j, std::memory_order_relaxed);
            next.store(0, std::memory_order_relaxed);
            njobs.store(n, std::memory_order_release);
            ++gen;
            gen_pub.store(gen, std::memory_order_release);
        }
        if (!th.empty() && n > 1) cv.notify_all();
    }
    bool is_done(int i) const { return done[i].load(std::memory_order_acquire) != 0; }
    void wait_job(int i)
    {
        // the caller packs as well while it has nothing to hand to the DMA engine (and does everything when there are no threads)
        while (!is_done(i))
            if (!take_one()) std::this_thread::yield();
    }
    void finish()
    {   // the job list lives on the caller's stack: no worker may still be looking at it when the caller returns
        njobs.store(0, std::memory_order_release);
        while (active.load(std::memory_order_acquire) != 0) std::this_thread::yield();
    }
};

static thread_local std::string g_create_err;

static size_t nxs(const ndp_handle *h) { return (size_t)h->cfg.batch * (h->cfg.N + 1) * NX; }
static size_t nus(const ndp_handle *h) { return (size_t)h->cfg.batch * h->cfg.N * NU; }
static size_t nfs(const ndp_handle *h) { return (size_t)h->cfg.batch * (h->cfg.N + 1) * 3; }
static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
// host cores this process may really use: the affinity mask, cut down to the cgroup's CPU quota (cpu.max: "<quota> <period>" or "max ...")
static int usable_cores()
{
    int n = (int)std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int a = CPU_COUNT(&set); if (a > 0 && a < n) n = a; }
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        double period = 0.0;
        if (fscanf(f, "%31s %lf", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0.0) {
            const int c = (int)(atof(q) / period);
            if (c >= 1 && c < n) n = c;
        }
        fclose(f);
    }
    return n < 1 ? 1 : n;
}
static size_t act_bytes(const ndp_handle *h) { return (size_t)h->cfg.batch * (size_t)act_pitch(h->cfg.N); }
// The trajectory block dTraj (ndp_ref_set_trajectory), one allocation of `doubles`, in this order: coefficients [B][S][28] (x, y, z: 8
// each, yaw: 4) | time_cum [B][S+1] | time_seg [B][S] | final_pt [B][3] | the one-launch tick's segment cache [B][SEGC_PER] (empty =
// NaNs: tick_early) | the segment hints int[B] (ref_point) | the cache's second copy [B][SEGC_PER] (tick_cache_store).  base = null:
// the size only.
struct TrajView {
    double *coeff, *tcum, *tseg, *fpt, *segc[2];
    int *hint;
    size_t doubles;
};
static TrajView traj_view(double *base, size_t B, size_t S)
{
    TrajView v;
    size_t o = 0;
    auto part = [&](size_t n) { double *p = base ? base + o : nullptr; o += n; return p; };
    v.coeff = part(B * S * 28); v.tcum = part(B * (S + 1)); v.tseg = part(B * S); v.fpt = part(B * 3);
    v.segc[0] = part(B * SEGC_PER); v.hint = reinterpret_cast<int *>(part((B * 4 + 7) / 8)); v.segc[1] = part(B * SEGC_PER);
    v.doubles = o;
    return v;
}
static TrajView traj_view(const ndp_handle *h) { return traj_view(h->dTraj, (size_t)h->cfg.batch, (size_t)h->traj_seg); }
// the step's iteration words (RtiIo::iters) -> the caller's interior-point iteration counts
static void copy_ipm_iters(int32_t *dst, const int32_t *src, size_t n)
{
    for (size_t i = 0; i < n; ++i) dst[i] = src[i] & ITERS_IPM_MASK;
}

// entry points that do not run the control step through rti_sens_kernel: refused on a handle with sensitivities on
int sens_refuse(ndp_handle *h, const char *what)
{
    h->err = std::string(what) + ": not available while initial-state sensitivities are enabled (ndp_sens_enable(h, 0) first): "
             "only the in-place and work-list step forms compute them";
    return -2;
}

// the shapes the work-queue form of rti_kernel is instantiated for (compile-time horizon and iteration count)
static bool queue_shape(const ndp_handle *h)
{
    return h->cfg.qp_precision == 0 &&
           ((h->cfg.N == 20 && h->cfg.n_rti == 1 && h->waves == 4) || (h->cfg.N == 40 && h->cfg.n_rti == 2 && h->waves == 2));
}

// Every control-step kernel the library launches, one entry per instantiation (RTI_K / RTI_SENS_K: collapsed in the development
// builds).  rti_pick chooses the entry of a call; ndp_create / ndp_sens_enable give every plain / sensitivity entry its dynamic LDS.
// (The order of the rows is the order the kernels lie in the code object.)
struct RtiKern {
    const void *fn;
    int waves;                 // instances per workgroup: the launch geometry
    bool sens;                 // rti_sens_kernel (KernArgs, SensArgs) or rti_psens_kernel (KernArgs, SensArgs, PSensArgs), else rti_kernel (KernArgs)
};
enum RtiId {
    K3_4, K3_2, K3_1, K5_4, K5_2, K5_1, K3F_4, K3F_2, K3F_1,         // any horizon: 3 / 5 slots, fused downwash; 4, 2, 1 instances per group
    K20, K20F, K20_W2, K20F_W2,                                       // the reference shape (N = 20, one RTI iteration)
    K20_PROD, K20F_PROD, K20_CONS, K20_LATE,                          // ... work-list producer / consumer, late-force step
    K20F_TICK, K20_TICK, K20F_PROD_TICK, K20_PROD_TICK,               // ... one-launch ticks
    KPREC1, KPREC2, KPREC3, KPREC4, KPREC5, KPREC6,                   // precision studies, any horizon, one wave per group
    K40_F32, K40_BF16, K40, K40_PROD, K40_CONS,                       // BASELINE config 5's shape (N = 40, two RTI iterations)
    S20F_PROD, S20_PROD, S20_CONS, S20F, S20, SF_4, S_4, SF_2, S_2,   // sensitivities (three slots)
    P20F_PROD, P20_PROD, P20_CONS, P20F, P20, PF_4, PF_2,              // ... with parameter sensitivities (no unfused run-time horizon)
    RTI_KERNELS
};
static const RtiKern k_rti[] = {
    {(const void *)RTI_K(3, 4, false), 4}, {(const void *)RTI_K(3, 2, false), 2}, {(const void *)RTI_K(3, 1, false), 1},
    {(const void *)RTI_K(5, 4, false), 4}, {(const void *)RTI_K(5, 2, false), 2}, {(const void *)RTI_K(5, 1, false), 1},
    {(const void *)RTI_K(3, 4, true), 4}, {(const void *)RTI_K(3, 2, true), 2}, {(const void *)RTI_K(3, 1, true), 1},
    {(const void *)RTI_K(3, 4, false, 20), 4}, {(const void *)RTI_K(3, 4, true, 20), 4},
    {(const void *)RTI_K(3, 2, false, 20), 2}, {(const void *)RTI_K(3, 2, true, 20), 2},
    {(const void *)RTI_K(3, 4, false, 20, 0, 1, 1), 4}, {(const void *)RTI_K(3, 4, true, 20, 0, 1, 1), 4},
    {(const void *)RTI_K(3, 4, false, 20, 0, 1, 2), 4}, {(const void *)RTI_K(3, 4, false, 20, 0, 1, 3), 4},
    {(const void *)RTI_K(3, 4, true, 20, 0, 1, 0, true), 4}, {(const void *)RTI_K(3, 4, false, 20, 0, 1, 0, true), 4},
    {(const void *)RTI_K(3, 4, true, 20, 0, 1, 1, true), 4}, {(const void *)RTI_K(3, 4, false, 20, 0, 1, 1, true), 4},
    {(const void *)RTI_K(5, 1, false, 0, 1), 1}, {(const void *)RTI_K(5, 1, false, 0, 2), 1}, {(const void *)RTI_K(5, 1, false, 0, 3), 1},
    {(const void *)RTI_K(5, 1, false, 0, 4), 1}, {(const void *)RTI_K(5, 1, false, 0, 5), 1}, {(const void *)RTI_K(5, 1, false, 0, 6), 1},
    {(const void *)RTI_K(5, 2, false, 40, 3, 2), 2}, {(const void *)RTI_K(5, 2, false, 40, 4, 2), 2},
    {(const void *)RTI_K(5, 2, false, 40, 0, 2), 2}, {(const void *)RTI_K(5, 2, false, 40, 0, 2, 1), 2},
    {(const void *)RTI_K(5, 2, false, 40, 0, 2, 2), 2},
    {(const void *)RTI_SENS_K(4, true, 20, 1), 4, true}, {(const void *)RTI_SENS_K(4, false, 20, 1), 4, true},
    {(const void *)RTI_SENS_K(4, false, 20, 2), 4, true},
    {(const void *)RTI_SENS_K(4, true, 20, 0), 4, true}, {(const void *)RTI_SENS_K(4, false, 20, 0), 4, true},
    {(const void *)RTI_SENS_K(4, true, 0, 0), 4, true}, {(const void *)RTI_SENS_K(4, false, 0, 0), 4, true},
    {(const void *)RTI_SENS_K(2, true, 0, 0), 2, true}, {(const void *)RTI_SENS_K(2, false, 0, 0), 2, true},
    {(const void *)RTI_PSENS_K(4, true, 20, 1), 4, true}, {(const void *)RTI_PSENS_K(4, false, 20, 1), 4, true},
    {(const void *)RTI_PSENS_K(4, false, 20, 2), 4, true},
    {(const void *)RTI_PSENS_K(4, true, 20, 0), 4, true}, {(const void *)RTI_PSENS_K(4, false, 20, 0), 4, true},
    {(const void *)RTI_PSENS_K(4, true, 0, 0), 4, true}, {(const void *)RTI_PSENS_K(2, true, 0, 0), 2, true},
};
static_assert(sizeof(k_rti) / sizeof(k_rti[0]) == RTI_KERNELS, "one row per RtiId");
static_assert(RTI_KERNELS <= 64, "ndp_debug_rti_launched reports the rows as bits of one 64-bit mask");

extern "C" {

int ndp_abi_version(void) { return NDP_ABI_VERSION; }
size_t ndp_cfg_size(void) { return sizeof(ndp_cfg); }

int ndp_default_cfg(ndp_cfg *cfg)
{
    if (!cfg) return -1;
    fill_default_cfg(cfg);
    return 0;
}

const char *ndp_last_error(const ndp_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int ndp_debug_lds_doubles(int N) { return lds_doubles(N) + DBG_EXTRA; }

int ndp_debug_lds_layout(int N, int *out8)
{
    if (!out8) return -1;
    lds_layout(N, out8);
    return 0;
}

int ndp_debug_mfma_probe(const double *a, const double *b, const double *c, double *d)
{
    double *da = nullptr, *db = nullptr, *dc = nullptr, *dd = nullptr;
    if (hipMalloc((void **)&da, 64 * 8) != hipSuccess || hipMalloc((void **)&db, 64 * 8) != hipSuccess ||
        hipMalloc((void **)&dc, 256 * 8) != hipSuccess || hipMalloc((void **)&dd, 832 * 8) != hipSuccess)
        return -1;
    (void)hipMemcpy(da, a, 64 * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, b, 64 * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dc, c, 256 * 8, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, 0, da, db, dc, dd);
    const hipError_t e = hipMemcpy(d, dd, 832 * 8, hipMemcpyDeviceToHost);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dc); (void)hipFree(dd);
    return e == hipSuccess ? 0 : -2;
}

int ndp_debug_mfma_probe_f32(const float *a, const float *b, const float *c, float *d, int mode)
{
    float *da = nullptr, *db = nullptr, *dc = nullptr, *dd = nullptr;
    if (hipMalloc((void **)&da, 256 * 4) != hipSuccess || hipMalloc((void **)&db, 256 * 4) != hipSuccess ||
        hipMalloc((void **)&dc, 256 * 4) != hipSuccess || hipMalloc((void **)&dd, 320 * 4) != hipSuccess)
        return -1;
    (void)hipMemcpy(da, a, 256 * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, b, 256 * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(dc, c, 256 * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(mfma_probe32_kernel, dim3(1), dim3(64), 0, 0, da, db, dc, dd, mode);
    const hipError_t e = hipMemcpy(d, dd, 320 * 4, hipMemcpyDeviceToHost);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dc); (void)hipFree(dd);
    return e == hipSuccess ? 0 : -2;
}

int ndp_destroy(ndp_handle *h)
{
    if (!h) return -1;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->ev_pending) (void)hipEventSynchronize(h->evLast);
    for (auto &e : h->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    if (h->evLast) (void)hipEventDestroy(h->evLast);
    if (h->aux) { (void)hipStreamSynchronize(h->aux); (void)hipStreamDestroy(h->aux); }
    for (hipEvent_t e : {h->evFork, h->evJoin, h->stepDone[0], h->stepDone[1], h->stepDone[2], h->stepDone[3]})
        if (e) (void)hipEventDestroy(e);
    h->pool.reset();
    void *ptrs[] = {h->dForceAB[0], h->dForceAB[1], h->dProto, h->dRingX, h->dTraj, h->dTables, h->dStamps, h->dRelay, h->dThr, h->sThr, h->dKC, h->dForce, h->dFrag,
                    h->dIn, h->dOut, h->sdbg, h->dQctr, h->dQids, h->dTickIndex, h->dTickThrust, h->dAct,
                    h->dSensU0, h->dSensU, h->dSensX, h->dPSensXr, h->dPSensUr, h->dPSensF, h->dVjp, h->dVjpSt, h->dVjpAct, h->dFragT, h->dGwPart};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    for (auto &sl : h->slot) {
        if (sl.hIn) (void)hipHostFree(sl.hIn);
        if (sl.hOut) (void)hipHostFree(sl.hOut);
        if (sl.evOut) (void)hipEventDestroy(sl.evOut);
    }
    if (h->hIpm) {                          // (a copy into it may still be queued on a caller's stream)
        (void)hipDeviceSynchronize();
        (void)hipHostFree(h->hIpm);
    }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

// a pin is the weight as_gamma on its input: far below the input weights it holds nothing, yet as_check still writes the input onto
// its bound -- a wrong step with status 0 (NDP_AS_GAMMA_FLOOR in the header).  ndp_create's rule, and ndp_set_model's for a new Rd.
static bool as_gamma_holds(const ndp_cfg &c, const double *Rd)
{
    if (c.as_iter_max <= 0) return true;
    double rd = 0.0;
    for (int i = 0; i < 4; ++i) rd = std::max(rd, std::fabs(c.dt * Rd[i]));
    return std::isfinite(c.as_gamma) && c.as_gamma >= NDP_AS_GAMMA_FLOOR * rd;
}

int ndp_create(const ndp_cfg *cfg, ndp_handle **out)
{
    if (!cfg || !out) { g_create_err = "ndp_create: null argument"; return -1; }
    *out = nullptr;
    if (cfg->batch < 1 || cfg->N < 2 || slots_for(cfg->N) > 5 || cfg->n_rti < 1 || cfg->qp_precision < 0 || cfg->qp_precision > 6 ||
        cfg->work_queue < 0 || cfg->work_queue > 2 || !(cfg->ts_nmpc > 0.0) || cfg->dt < cfg->ts_nmpc) {
        g_create_err = "ndp_create: need batch >= 1, 2 <= N <= 46, n_rti >= 1, qp_precision in 0..6, work_queue in 0..2, 0 < ts_nmpc <= dt";
        return -2;
    }
    if (cfg->qp_precision >= 5 && (cfg->N % 4 != 0 || cfg->N > 40)) {
        g_create_err = "ndp_create: the condensed study (qp_precision 5 / 6) tiles the 4N x 4N Hessian by 16: N must be a multiple of 4, at most 40";
        return -2;
    }
    if (!as_gamma_holds(*cfg, cfg->Rd)) {
        g_create_err = "ndp_create: as_gamma must be finite and at least 1e8 * max(dt * Rd) when as_iter_max > 0 (a weaker pin does not hold "
                       "its input on the bound)";
        return -2;
    }
    if (cfg->ipm_refine > 0 && (slots_for(cfg->N) > 3 || cfg->qp_precision != 0)) {
        // (rounds 4-5 accepted the setting and ignored it -- a getter nobody called said so)
        g_create_err = "ndp_create: ipm_refine > 0 is not served for this shape: the refinement path (stiff sweeps + second solves while a STATE bound's "
                       "barrier term exceeds refine_gamma) lives in the three-slot fp64 kernels only (N <= 27, qp_precision 0); the five-slot kernels "
                       "(N >= 28) sit at the register limit without it.  Set ipm_refine = 0: strongly active state bounds at a tight tolerance then "
                       "end in status 4 (never a silent answer)";
        return -2;
    }
    {   // the reference list holds one point per control period and the window is every (dt / ts_nmpc)-th entry
        // (params/nmpc_params.py:40-43): the ratio has to be a whole number, else ring windows and direct windows disagree
        const double ratio = cfg->dt / cfg->ts_nmpc, nearest = (double)(long long)(ratio + 0.5);
        if (ratio - nearest > 1e-9 || nearest - ratio > 1e-9) {
            g_create_err = "ndp_create: dt must be a whole multiple of ts_nmpc (node spacing = every k-th entry of the reference list)";
            return -2;
        }
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= cfg->device) {
        g_create_err = std::string("ndp_create: no usable HIP device (") + hipGetErrorString(e) + ")";
        return -3;
    }
    ndp_handle *h = new (std::nothrow) ndp_handle;
    if (!h) return -4;
    h->cfg = *cfg;
    h->P = to_params(*cfg);
    h->list_step = (int)(cfg->dt / cfg->ts_nmpc + 0.5);      // params/nmpc_params.py:40-43: every 5th list entry is a node
    h->lds_per_wave = (lds_doubles(cfg->N) + 1) & ~1;   // keep 16-byte alignment per wave slice
    if (cfg->qp_precision >= 5) h->lds_per_wave += (cond_extra_doubles(cfg->N) + 1) & ~1;   // (the condensed study works behind the slice: one wave per workgroup)
    const size_t per_wave_bytes = (size_t)h->lds_per_wave * sizeof(double);
    h->waves = 4;
    while (h->waves > 1 && per_wave_bytes * h->waves > 160 * 1024) h->waves >>= 1;
    if (const char *e = getenv("NDP_DEV_WAVES")) {      // measurement switch: instances per workgroup (2: two workgroups per CU)
        const int w = atoi(e);
        if ((w == 1 || w == 2 || w == 4) && w <= h->waves) h->waves = w;
    }
    auto fail = [&](const char *what, hipError_t err) {
        g_create_err = std::string("ndp_create: ") + what + ": " + hipGetErrorString(err);
        ndp_destroy(h);
        return -5;
    };
    if ((e = hipSetDevice(cfg->device)) != hipSuccess) return fail("hipSetDevice", e);
    {
        hipDeviceProp_t prop;
        if ((e = hipGetDeviceProperties(&prop, cfg->device)) != hipSuccess) return fail("hipGetDeviceProperties", e);
        h->n_simd = 4 * prop.multiProcessorCount;
    }
    // work list: with one instance per SIMD nothing can be re-balanced; with two or more it is switched by what the steps do
    // (queue_policy) -- callers who know their workload set cfg.work_queue = 1 / 2.
    // The N = 40 / 2-iteration shape always takes the list: its producer kernel carries no interior-point code and does not
    // spill, which is worth 17 % even when nothing is listed (the in-place kernel of that shape uses 0.9 KB of scratch per lane)
    if (cfg->work_queue == 1 && !(queue_shape(h) && cfg->qp_mode == NDP_QP_AUTO)) {
        g_create_err = "ndp_create: work_queue = 1 needs qp_mode AUTO, qp_precision 0 and (N, n_rti) = (20, 1) or (40, 2)";
        delete h;
        return -2;
    }
    // reference shape, two or more instances per SIMD, cfg.work_queue = 0: in place to begin with, the list when the steps ask for it
    // (queue_policy)
    h->queue_auto = cfg->work_queue == 0 && queue_shape(h) && cfg->qp_mode == NDP_QP_AUTO && cfg->N == 20 && cfg->batch >= 2 * h->n_simd;
    h->use_queue = cfg->work_queue == 1 || (cfg->work_queue == 0 && queue_shape(h) && cfg->qp_mode == NDP_QP_AUTO && cfg->N == 40);
    if (h->queue_auto) {
        if ((e = hipHostMalloc((void **)&h->hIpm, 64, hipHostMallocDefault)) != hipSuccess) return fail("hipHostMalloc (work-list counter)", e);
        h->hIpm[0] = h->hIpm[1] = 0;
    }
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    if ((e = hipEventCreateWithFlags(&h->evLast, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    const size_t B = cfg->batch;
#define ALLOC(p, n)                                                                      \
    if ((e = hipMalloc((void **)&(p), (n))) != hipSuccess) return fail("hipMalloc " #p, e)
    ALLOC(h->dForce, nfs(h) * 4); ALLOC(h->dFrag, FR_TOTAL * 4); ALLOC(h->dFragT, FRT_TOTAL * 4); ALLOC(h->dGwPart, (size_t)mlp_vjp_groups(h) * NDP_MLP_NPARAM * 4); ALLOC(h->dKC, KC_HOST * 8);
    ALLOC(h->dThr, B * 8 * 8); ALLOC(h->sThr, B * 11 * 8);
    ALLOC(h->dRelay, B * 4 * 8);
    ALLOC(h->dQctr, 256); ALLOC(h->dQids, B * 4);
    ALLOC(h->dAct, B * (size_t)act_pitch(cfg->N));
    (void)hipMemsetAsync(h->dAct, 0, B * (size_t)act_pitch(cfg->N), h->stream);
    (void)hipMemsetAsync(h->dRelay, 0, B * 4 * 8, h->stream);
    (void)hipMemsetAsync(h->dQctr, 0, 256, h->stream);
    {
        double kc[KC_HOST];
        fill_kc(h->P, kc);
        if ((e = hipMemcpyAsync(h->dKC, kc, sizeof(kc), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail("hipMemcpy kc", e);
        ALLOC(h->dTables, TB_WORDS * 4);
        std::vector<int> tb(TB_WORDS);
        fill_tables(cfg->N, tb.data(), (cfg->qp_precision == 3 || cfg->qp_precision == 4) ? 1 : 0);   // the fp32 / bf16 sweeps keep a different column per lane
        if ((e = hipMemcpyAsync(h->dTables, tb.data(), TB_WORDS * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail("hipMemcpy tables", e);
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail("hipStreamSynchronize", e);
    }
    {   // input / output blocks and their views
        size_t o = 0;
        h->off_x0 = o; o += up256(B * NX * 8);
        h->off_xr = o; o += up256(nxs(h) * 8);
        h->off_ur = o; o += up256(nus(h) * 8);
        h->off_f = o; o += up256(nfs(h) * 8);        // (fp32 forces, or fp64 ones: ndp_step_ex_f64)
        h->off_other = o; o += up256(nxs(h) * 8);
        h->off_ego = o; o += up256(B * 2 * 8);
        h->in_bytes = o;
        o = 0;
        h->off_u0 = o; o += up256(B * NU * 8);
        h->off_st = o; o += up256(B * 4);
        h->off_it = o; o += up256(B * 4);
        h->out_bytes = o;
        // the persistent iterate lives right behind the small outputs: u0 | status | iterations | X | U come back to the host
        // in ONE copy when a caller asks for the iterate as well (ndp_step_ex).  All of it is HBM; the page-locked host
        // mirrors of the host-array entry points are allocated by their first call (ensure_slots).
        h->out_all = h->out_bytes + (nxs(h) + nus(h)) * 8;
        ALLOC(h->dIn, h->in_bytes);
        ALLOC(h->dOut, h->out_all);
        h->dX = (double *)(h->dOut + h->out_bytes); h->dU = h->dX + nxs(h);
        h->sx0 = (double *)(h->dIn + h->off_x0); h->sxr = (double *)(h->dIn + h->off_xr); h->sur = (double *)(h->dIn + h->off_ur);
        h->sf = (float *)(h->dIn + h->off_f); h->sother = (double *)(h->dIn + h->off_other); h->sego = (double *)(h->dIn + h->off_ego);
        h->su0 = (double *)(h->dOut + h->off_u0); h->dStatus = (int *)(h->dOut + h->off_st); h->dIters = (int *)(h->dOut + h->off_it);
        h->lastStatus = h->dStatus; h->lastIters = h->dIters;
        ALLOC(h->sdbg, (size_t)(lds_doubles(cfg->N) + DBG_EXTRA) * 8);
    }
#undef ALLOC
    (void)hipMemsetAsync(h->dX, 0, nxs(h) * 8, h->stream);
    (void)hipMemsetAsync(h->dU, 0, nus(h) * 8, h->stream);
    (void)hipMemsetAsync(h->dOut, 0, h->out_bytes, h->stream);
    (void)hipMemsetAsync(h->dForce, 0, nfs(h) * 4, h->stream);
    // allow the big dynamic-LDS launches
    const int lds_bytes = (int)(per_wave_bytes * h->waves);
    if ((e = hipFuncSetAttribute((const void *)mlp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(FR_TOTAL * sizeof(float)))) != hipSuccess)
        return fail("hipFuncSetAttribute(mlp_kernel)", e);
    if ((e = mlp_vjp_prepare()) != hipSuccess) return fail("hipFuncSetAttribute(mlp_vjp_kernel)", e);
    for (const RtiKern &k : k_rti)      // (the sensitivity kernels: ndp_sens_enable)
        if (!k.sens && (e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)) != hipSuccess)
            return fail("hipFuncSetAttribute", e);
    for (const void *fn : {(const void *)rti_wvjp_kernel<20>, (const void *)rti_wvjp_kernel<0>})   // (ndp_step_vjp_model_device)
        if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)) != hipSuccess)
            return fail("hipFuncSetAttribute(rti_wvjp_kernel)", e);
    for (const void *fn : {(const void *)rti_jvp_kernel<20>, (const void *)rti_jvp_kernel<0>})     // (forward mode: ndp_step_jvp_device)
        if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)) != hipSuccess)
            return fail("hipFuncSetAttribute(rti_jvp_kernel)", e);
    for (const void *fn : {(const void *)rti_vjp_kernel<20>, (const void *)rti_vjp_kernel<0>})     // (the adjoint: ndp_step_vjp_device)
        if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)) != hipSuccess)
            return fail("hipFuncSetAttribute(rti_vjp_kernel)", e);
    hipLaunchKernelGGL(throttle_reset_kernel, dim3((cfg->batch + 255) / 256), dim3(256), 0, h->stream, h->dThr, 50.0, cfg->batch);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail("hipStreamSynchronize", e);
    *out = h;
    return 0;
}

int ndp_set_mlp_weights(ndp_handle *h, const float *blob, size_t n)
{
    if (!h || !blob) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (n != NDP_MLP_NPARAM) { h->err = "ndp_set_mlp_weights: expected 17859 floats"; return -2; }
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    std::vector<float> fr;
    make_fragments(blob, fr);
    std::vector<float> frt(FRT_TOTAL);
    make_fragments_t(blob, frt.data());          // the backward pass's records (mlp_vjp.hip)
    NDP_HIP(h, hipMemcpyAsync(h->dFrag, fr.data(), FR_TOTAL * 4, hipMemcpyHostToDevice, h->stream));
    NDP_HIP(h, hipMemcpyAsync(h->dFragT, frt.data(), FRT_TOTAL * 4, hipMemcpyHostToDevice, h->stream));
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    h->have_mlp = true;
    return 0;
}

// ---- enqueue helpers (no locking, no sync) ----
// defer: the caller may hand the pair to the launch itself (hipExtLaunchKernel's start / stop events: the dispatch packet's own
// timestamps, no event packets around the kernel -- an event pair recorded around a launch adds ~2.5 us of dispatch gap to what it
// measures); it records ev.a itself if it cannot.
static int begin_timing(ndp_handle *h, hipStream_t s, int kind, bool defer = false)
{
    h->timing_open = false;
    if (!h->timing || (h->launch_no[kind]++ % h->timing) != 0) return 0;
    h->timing_open = true;
    ndp_handle::Ev ev; ev.kind = kind;
    NDP_HIP(h, hipEventCreate(&ev.a)); NDP_HIP(h, hipEventCreate(&ev.b));
    if (!defer) NDP_HIP(h, hipEventRecord(ev.a, s));
    h->events.push_back(ev);
    return 0;
}
static int end_timing(ndp_handle *h, hipStream_t s)
{
    if (!h->timing_open) return 0;
    NDP_HIP(h, hipEventRecord(h->events.back().b, s));
    return 0;
}

// A *_device call enqueued on a caller's stream: remember it so that the getters (ndp_get_status, ndp_get_iterate, ...)
// wait for that work and not only for the library's own stream.  Streams being captured into a graph are skipped (an
// event recorded there belongs to the graph and cannot be waited on from the host).
int note_stream(ndp_handle *h, hipStream_t s)
{
    if (s == h->stream) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return 0; }
    NDP_HIP(h, hipEventRecord(h->evLast, s));
    h->ev_pending = true;
    return 0;
}
static int wait_all(ndp_handle *h)
{
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    if (h->ev_pending) {
        NDP_HIP(h, hipEventSynchronize(h->evLast));
        h->ev_pending = false;
    }
    if (h->track_pending) {            // tracked control steps on a caller's stream (ndp_xchg_tick_step): the last one's completion event
        if (h->stepDone[h->step_seq & 3]) NDP_HIP(h, hipEventSynchronize(h->stepDone[h->step_seq & 3]));
        h->track_pending = false;
    }
    return 0;
}

int set_device(ndp_handle *h)
{
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    return 0;
}

struct Neigh {                 // neighbour windows of a step (device pointers)
    const double *other = nullptr;
    int stride = NX;           // doubles per node: 10 or 6
    const int *index = nullptr;
    const double *ego_xy = nullptr;
    size_t pitch = 0;          // doubles between rows of `other`; 0 = dense, (N+1) stride
    size_t ego_pitch = 0;      // doubles between instances of ego_xy; 0 = dense, 2
};

static int launch_mlp(ndp_handle *h, const Neigh &nb, const double *d_ego, float *d_f, hipStream_t s, size_t ego_pitch = 0)
{
    if (!h->have_mlp) { h->err = "downwash requested but ndp_set_mlp_weights was never called"; return -6; }
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * np1;
    const int ntiles = (rows + 31) / 32;
    const int grid = (ntiles + 3) / 4;
    int rc = begin_timing(h, s, 1);
    if (rc) return rc;
    hipLaunchKernelGGL(mlp_kernel, dim3(grid), dim3(256), FR_TOTAL * sizeof(float), s, (const float *)h->dFrag, nb.other, d_ego, nb.ego_xy, d_f,
                       rows, np1, h->cfg.r_horiz * h->cfg.r_horiz, nb.stride, nb.index, peer_mapped(nb.other),
                       nb.pitch ? nb.pitch : (size_t)np1 * nb.stride, ego_pitch ? ego_pitch : (size_t)np1 * NX, nb.ego_pitch ? nb.ego_pitch : (size_t)2);
    NDP_HIP(h, hipGetLastError());
    return end_timing(h, s);
}

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

// The automatic work-list rule (cfg.work_queue = 0, reference shape, at least two instances per SIMD).  The list re-balances interior-
// point solves over all SIMDs (+70 % at batch 4096 when a fifth of the instances iterate) but costs a step that lists nothing two more
// launches and a slower producer kernel: 8-15 % (batch 2048: 45.4 against 39.5 us; 16 384: 332 against 309 us).  So the handle starts in
// place and looks at what the steps do: the device keeps two monotonic counts -- instances that went into the interior-point loop (counted
// by the in-place kernel, added up by the list's reset launch) and control steps executed -- and a 16-byte copy of the pair is enqueued
// behind every QP_WINDOW-th launch.  Whenever a snapshot that covers QP_WINDOW more executed steps has LANDED (the host may be many
// launches ahead of the device), the fraction over those steps switches the list on at >= 4 %, off at <= 1.5 %.  Evaluated at launch
// time: a captured graph keeps the form it was captured in.
enum { QP_WINDOW = 8 };
static void queue_policy(ndp_handle *h, hipStream_t s)
{
    if (!h->queue_auto) return;
    const unsigned long long steps_now = ((volatile unsigned long long *)h->hIpm)[1], ipm_now = ((volatile unsigned long long *)h->hIpm)[0];
    if (steps_now >= h->steps_seen + QP_WINDOW && ipm_now >= h->ipm_seen) {
        const double frac = (double)(ipm_now - h->ipm_seen) / ((double)(steps_now - h->steps_seen) * (double)h->cfg.batch);
        if (frac >= 0.04) h->use_queue = true;
        else if (frac <= 0.015) h->use_queue = false;
        h->ipm_seen = ipm_now;
        h->steps_seen = steps_now;
    }
    if (++h->queue_launches < QP_WINDOW) return;
    h->queue_launches = 0;
    if (hipMemcpyAsync(h->hIpm, reinterpret_cast<unsigned long long *>(h->dQctr + 16), 16, hipMemcpyDeviceToHost, s) != hipSuccess) (void)hipGetLastError();
}

// The kernel of one launch of a step.  phase: 0 the in-place step, 1 / 2 the work list's producer / consumer.  (The late-force and tick
// forms have no sensitivity kernel: launch_rti refuses them first.)
static RtiId rti_pick(const ndp_handle *h, bool fused, bool tick, bool prefetched, int phase)
{
    const int N = h->cfg.N, W = h->waves, pr = h->cfg.qp_precision, wi = W == 4 ? 0 : W == 2 ? 1 : 2;
    const bool ref = N == 20 && h->cfg.n_rti == 1;     // the reference configuration (params/nmpc_params.py:9, 1 RTI iteration): compile-time instantiations
    if (pr) {                                          // BASELINE config 5 (unfused; run ndp_downwash first for a force)
        if (pr >= 3 && N == 40 && h->cfg.n_rti == 2 && W == 2) return pr == 3 ? K40_F32 : K40_BF16;   // config 5's own shape: 2 instances per workgroup
        return (RtiId)(KPREC1 + pr - 1);               // any horizon: one wave per workgroup (5 / 6: the condensed study, fp32 / bf16 instruction)
    }
    if (h->sens_level > 0) {
        // (ndp_sens_enable admits three-slot shapes at qp_precision 0, one RTI iteration, 2 or 4 instances per workgroup; work list: N = 20)
        RtiId id;
        if (phase) id = phase == 2 ? S20_CONS : fused ? S20F_PROD : S20_PROD;
        else if (N == 20 && W == 4) id = fused ? S20F : S20;
        else if (W == 4) id = fused ? SF_4 : S_4;
        else id = fused ? SF_2 : S_2;
        if (!h->dPSensXr) return id;
        // ndp_sens_params_enable (launch_rti has refused the unfused run-time horizon: S_4, S_2)
        switch (id) {
        case S20F_PROD: return P20F_PROD;
        case S20_PROD: return P20_PROD;
        case S20_CONS: return P20_CONS;
        case S20F: return P20F;
        case S20: return P20;
        case SF_4: return PF_4;
        default: return PF_2;
        }
    }
    if (phase == 2) return N == 20 ? K20_CONS : K40_CONS;
    if (phase == 1) {
        if (N != 20) return K40_PROD;
        if (tick) return fused ? K20F_PROD_TICK : K20_PROD_TICK;
        return fused ? K20F_PROD : K20_PROD;
    }
    if (ref && W == 4) {
        if (tick) return fused ? K20F_TICK : K20_TICK;
        return fused ? K20F : prefetched ? K20_LATE : K20;
    }
    if (ref && W == 2) return fused ? K20F_W2 : K20_W2;     // (NDP_DEV_WAVES = 2: the same program, two instances per workgroup)
    if (N == 40 && h->cfg.n_rti == 2 && W == 2 && !fused) return K40;   // BASELINE config 5's shape, compile-time as well
    if (fused) return (RtiId)(K3F_4 + wi);
    return (RtiId)((slots_for(N) <= 3 ? K3_4 : K5_4) + wi);
}

// One launch of a control-step kernel.  start / stop (either may be null): the timing pair or the step's completion event, carried
// by the dispatch packet itself (hipExtLaunchKernel).  The caller checks hipGetLastError.
static void launch_kern(const ndp_handle *h, RtiId id, hipStream_t s, KernArgs &ka, SensArgs &sa, hipEvent_t start = nullptr,
                        hipEvent_t stop = nullptr)
{
    const RtiKern &k = k_rti[id];
    h->rti_launched.fetch_or(1ull << id, std::memory_order_relaxed);
    const dim3 grid((h->cfg.batch + k.waves - 1) / k.waves), block(64 * k.waves);
    const size_t shm = (size_t)h->lds_per_wave * sizeof(double) * k.waves;
    PSensArgs pa{h->dPSensXr, h->dPSensUr, h->dPSensF};
    void *args[] = {&ka, &sa, &pa};     // (rti_kernel takes the first only, rti_sens_kernel the first two)
    if (start || stop) (void)hipExtLaunchKernel(k.fn, grid, block, args, shm, s, start, stop, 0);
    else (void)hipLaunchKernel(k.fn, grid, block, args, shm, s);
}

static int launch_rti(ndp_handle *h, const double *d_x0, const double *d_xr, const double *d_ur, const float *d_f,
                      double *d_u0, double *d_dbg, hipStream_t s, const Neigh *nb = nullptr, const StepOut *so = nullptr,
                      bool prefetched = false)
{
    int *d_status = so && so->status ? so->status : h->dStatus, *d_iters = so && so->iters ? so->iters : h->dIters;
    h->lastStatus = d_status; h->lastIters = d_iters;
    BatchPtrs bp{h->dKC, h->dTables, d_x0, d_xr, d_ur, d_f, h->dX, h->dU, d_u0, d_status, d_iters,
                 so ? so->Xm : nullptr, so ? so->Um : nullptr, d_dbg, h->dStamps,
                 so && so->xr_pitch ? so->xr_pitch : (size_t)(h->cfg.N + 1) * NX, so && so->ur_pitch ? so->ur_pitch : (size_t)h->cfg.N * NU, (size_t)NX,
                 so ? so->cmd : nullptr, so ? so->kthr : nullptr, so ? so->thrust_keep : nullptr, h->cfg.mass, so && so->f_f64 ? 1 : 0,
                 h->dAct};
    const bool fused = nb && nb->other;
    MlpArgs ma{fused ? h->dFrag : nullptr, fused ? nb->other : nullptr, fused ? nb->ego_xy : nullptr, h->dForce,
               h->cfg.r_horiz * h->cfg.r_horiz, fused ? nb->stride : NX, fused ? nb->index : nullptr, fused ? peer_mapped(nb->other) : 0,
               fused && nb->pitch ? nb->pitch : (size_t)(h->cfg.N + 1) * (fused ? nb->stride : NX), fused && nb->ego_pitch ? nb->ego_pitch : (size_t)2};
    QueueArgs qa{h->dQctr, h->dQids, reinterpret_cast<unsigned long long *>(h->dQctr + 16)};
    LateArgs la{prefetched ? h->dProto : nullptr, {h->dForceAB[0], h->dForceAB[1]}, h->prefetch_timeout_us,
                h->pf_groups_rti, h->pf_ntiles};
    KernArgs ka{h->P, bp, h->cfg.batch, h->lds_per_wave, ma, qa, la, so && so->tick ? *so->tick : TickArgs{}};
    SensArgs sa{h->dSensU0, h->sens_level >= 2 ? h->dSensU : nullptr, h->sens_level >= 2 ? h->dSensX : nullptr, h->sens_level};
    const bool tick1 = so && so->tick;   // (tick_enqueue hands a TickArgs over only for the shapes the TICK kernels exist for)
    const int pr = h->cfg.qp_precision;
    const bool q = h->use_queue && !d_dbg && !prefetched;      // (the late-force step is in place: its launch is the lean instantiation)
    // Tracked steps carry their completion event on a dispatch packet (hipExtLaunchKernel), which a stream capture cannot hold:
    // refuse instead of launching something the graph would silently drop the event of.
    h->last_step_tracked = false;
    if (h->track_steps) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        if (cs != hipStreamCaptureStatusNone) {
            h->err = "tracked control steps (ndp_track_steps) cannot be launched on a stream that is being captured: switch tracking off "
                     "and order the exchange through the stream (ndp_xchg_begin's after_stream)";
            return -15;
        }
    }
    int rc = begin_timing(h, s, 0, true);
    if (rc) return rc;
    // timed launch of a single-kernel step: the pair rides on the dispatch packet (otherwise recorded around the launches)
    const bool ext_timing = h->timing_open && !q && !pr && !(so && so->done) && !h->track_steps;
    if (h->timing_open && !ext_timing) NDP_HIP(h, hipEventRecord(h->events.back().a, s));
    if (pr && fused) { h->err = "qp_precision != 0 supports f / no disturbance only (run ndp_downwash first)"; return -12; }
    // tracked steps: the LAST launch of the step carries the completion event (in-place kernel, or the work list's reset launch; the
    // precision studies, not on the exchange's fast path, record it behind their launch)
    hipEvent_t stop = nullptr;
    if (so && so->done) stop = so->done;
    else if (h->track_steps) { stop = h->stepDone[++h->step_seq & 3]; h->last_step_tracked = true; }
    if (h->sens_level > 0 && (prefetched || tick1)) { h->err = "launch_rti: the late-force and tick forms have no sensitivity kernel"; return -2; }
    launch_kern(h, rti_pick(h, fused, tick1, prefetched, q ? 1 : 0), s, ka, sa, ext_timing ? h->events.back().a : nullptr,
                ext_timing ? h->events.back().b : q || pr ? nullptr : stop);
    if (ext_timing) h->timing_open = false;     // (end_timing has nothing left to record)
    NDP_HIP(h, hipGetLastError());
    if (q) {
        // work list: producer (every instance: one solve with the kept set's pins, done or defer), consumer (the deferred ones, from
        // scratch: active-set iterations, then the interior-point loop if need be; several RTI iterations: the automatic rule per
        // iteration), a one-wave launch that empties the list for the next step.  The consumer reads the fused producer's
        // force from dForce.
        KernArgs kc = ka;
        kc.bp.f = fused ? h->dForce : d_f;
        kc.ma.frag = nullptr; kc.ma.other = nullptr;
        // (active-set iterations off: a listed instance needs the interior-point loop, the consumer goes straight to it; on: the
        // producer lists every instance whose first solve -- with the kept set's pins -- did not settle, the consumer iterates on the set)
        if (h->cfg.n_rti == 1 && h->cfg.as_iter_max <= 0) kc.P.qp_mode = QP_IPM_ALWAYS;
        launch_kern(h, rti_pick(h, fused, tick1, prefetched, 2), s, kc, sa);
        NDP_HIP(h, hipGetLastError());
        if (stop) hipExtLaunchKernelGGL(queue_reset_kernel, dim3(1), dim3(64), 0, s, nullptr, stop, 0, h->dQctr, qa.ipm_total);
        else hipLaunchKernelGGL(queue_reset_kernel, dim3(1), dim3(64), 0, s, h->dQctr, qa.ipm_total);
        NDP_HIP(h, hipGetLastError());
    } else if (pr && stop) NDP_HIP(h, hipEventRecord(stop, s));
    const int rce = end_timing(h, s);
    queue_policy(h, s);
    return rce;
}

// downwash inside the RTI launch when one 32-row tile covers the horizon; otherwise mlp_kernel first
static bool can_fuse(const ndp_handle *h)
{
    return h->cfg.qp_precision == 0 && h->cfg.N + 1 <= 32 && slots_for(h->cfg.N) <= 3 &&
           (size_t)h->lds_per_wave * sizeof(double) * h->waves >= FR_TOTAL * sizeof(float);
}

// one control step on device pointers: [mlp_kernel ->] rti_kernel (no locking, no sync)
static int enqueue_step(ndp_handle *h, const double *d_x0, const double *d_xr, const double *d_ur, const float *d_f,
                        const Neigh &nb, double *d_u0, double *d_dbg, hipStream_t s, const StepOut *so = nullptr)
{
    // The unfused step at a run-time horizon has no parameter-sensitivity kernel (rti_psens_kernel): that instantiation of the shared body
    // sits at the register limit and would carry a scratch-memory frame.  The fused step (any N <= 27) and the N = 20 kernels serve them.
    if (h->dPSensXr && !(nb.other && can_fuse(h)) && !(h->cfg.N == 20 && h->waves == 4)) {
        h->err = "ndp_step: parameter sensitivities at N != 20 (or 2 instances per workgroup) need the fused step (neighbour windows "
                 "given): the unfused kernel of a run-time horizon has none";
        return -2;
    }
    if ((d_f || nb.other) && !h->cfg.use_fd) { h->err = "ndp_step: a disturbance force needs use_fd = 1 (NDP model)"; return -8; }
    if (nb.other) {
        if (d_f) { h->err = "ndp_step: pass either f or other, not both"; return -7; }
        if (nb.stride != 10 && nb.stride != 6) { h->err = "ndp_step: other_stride must be 10 or 6"; return -13; }
        if (!h->have_mlp) { h->err = "downwash requested but ndp_set_mlp_weights was never called"; return -6; }
        if (can_fuse(h)) return launch_rti(h, d_x0, d_xr, d_ur, nullptr, d_u0, d_dbg, s, &nb, so);
        int rc = launch_mlp(h, nb, d_xr, h->dForce, s, so ? so->xr_pitch : 0);
        if (rc) return rc;
        d_f = h->dForce;
    }
    return launch_rti(h, d_x0, d_xr, d_ur, d_f, d_u0, d_dbg, s, nullptr, so);
}

int ndp_reset_device(ndp_handle *h, const void *d_xr, const void *d_ur, void *stream)
{
    Entry g(h, d_xr && d_ur, stream);
    if (g.rc) return g.rc;
    NDP_HIP(h, hipMemcpyAsync(h->dX, d_xr, nxs(h) * 8, hipMemcpyDefault, g.s));
    NDP_HIP(h, hipMemcpyAsync(h->dU, d_ur, nus(h) * 8, hipMemcpyDefault, g.s));
    NDP_HIP(h, hipMemsetAsync(h->dAct, 0, act_bytes(h), g.s));      // a new iterate: the QPs start from an empty active set
    return g.noted(0);
}

int ndp_reset(ndp_handle *h, const double *xr, const double *ur)
{
    Entry g(h, xr && ur);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(h->dX, xr, nxs(h) * 8, hipMemcpyDefault, h->stream));
    NDP_HIP(h, hipMemcpyAsync(h->dU, ur, nus(h) * 8, hipMemcpyDefault, h->stream));
    NDP_HIP(h, hipMemsetAsync(h->dAct, 0, act_bytes(h), h->stream));
    return g.synced(0);
}

int ndp_step_device_ex(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                       const void *d_other, int other_stride, const void *d_other_index, const void *d_ego_xy,
                       void *d_u0, void *stream)
{
    Entry g(h, d_x0 && d_xr && d_ur && d_u0, stream);
    if (g.rc) return g.rc;
    Neigh nb;
    nb.other = (const double *)d_other; nb.stride = other_stride; nb.index = (const int *)d_other_index; nb.ego_xy = (const double *)d_ego_xy;
    return g.noted(enqueue_step(h, (const double *)d_x0, (const double *)d_xr, (const double *)d_ur, (const float *)d_f, nb,
                                (double *)d_u0, nullptr, g.s));
}

int ndp_step_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                    const void *d_other, const void *d_ego_xy, void *d_u0, void *stream)
{
    return ndp_step_device_ex(h, d_x0, d_xr, d_ur, d_f, d_other, NX, nullptr, d_ego_xy, d_u0, stream);
}

// ---- downwash one tick ahead (second stream) + the control step that consumes it
static int ensure_prefetch(ndp_handle *h)
{
    if (h->aux) return 0;
    if (!h->cfg.use_fd) { h->err = "downwash prefetch needs use_fd = 1 (NDP model)"; return -8; }
    if (h->use_queue && !h->queue_auto) { h->err = "downwash prefetch is not combined with the interior-point work list (set cfg.work_queue = 2)"; return -16; }
    if (h->cfg.qp_precision) { h->err = "downwash prefetch serves the fp64 product path only"; return -12; }
    if (h->cfg.N + 1 > 32) { h->err = "downwash prefetch needs N + 1 <= 32 (an instance's rows in at most two 32-row tiles)"; return -12; }
    if (!h->have_mlp) { h->err = "downwash requested but ndp_set_mlp_weights was never called"; return -6; }
    // (h->aux, created last, marks completion; members a failed earlier call did allocate are reused, not allocated again)
    for (int i = 0; i < 2; ++i) {
        if (!h->dForceAB[i]) NDP_HIP(h, hipMalloc((void **)&h->dForceAB[i], nfs(h) * 4));
        NDP_HIP(h, hipMemset(h->dForceAB[i], 0, nfs(h) * 4));
    }
    h->pf_ntiles = (unsigned)((h->cfg.batch * (h->cfg.N + 1) + 31) / 32);
    const size_t proto_words = (size_t)PF_EPOCH + 2 * (size_t)h->pf_ntiles;
    if (!h->dProto) NDP_HIP(h, hipMalloc((void **)&h->dProto, proto_words * 8));
    NDP_HIP(h, hipMemset(h->dProto, 0, proto_words * 8));
    {
        const unsigned grid_rti = (unsigned)((h->cfg.batch + h->waves - 1) / h->waves);
        h->pf_groups_rti = grid_rti < PF_GROUPS ? grid_rti : PF_GROUPS;
    }
    // its own hardware queue: the downwash launch has to RUN beside the control step (a stream that shares the caller's hardware
    // queue would execute behind it).  Streams of another priority level get queues of their own.
    int lo = 0, hi = 0;
    NDP_HIP(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
    if (!h->evFork) NDP_HIP(h, hipEventCreateWithFlags(&h->evFork, hipEventDisableTiming));
    if (!h->evJoin) NDP_HIP(h, hipEventCreateWithFlags(&h->evJoin, hipEventDisableTiming));
    NDP_HIP(h, hipStreamCreateWithPriority(&h->aux, hipStreamNonBlocking, hi));
    return 0;
}

int ndp_downwash_prefetch_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index,
                                 const void *d_ego_ref, const void *d_ego_xy, void *after_stream, void *on_stream)
{
    Entry g(h, d_other && d_ego_ref);
    if (g.rc) return g.rc;
    int rc = ensure_prefetch(h);
    if (rc) return rc;
    if (other_stride != 10 && other_stride != 6) { h->err = "ndp_downwash_prefetch_device: other_stride must be 10 or 6"; return -13; }
    hipStream_t a = on_stream ? (hipStream_t)on_stream : h->aux;
    if (after_stream) {      // the windows are produced on that stream (and, inside a capture, this is what brings the second stream in)
        NDP_HIP(h, hipEventRecord(h->evFork, (hipStream_t)after_stream));
        NDP_HIP(h, hipStreamWaitEvent(a, h->evFork, 0));
    }
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * np1;
    const int ntiles = (rows + 31) / 32;
    hipLaunchKernelGGL(prefetch_gate_kernel, dim3(1), dim3(64), 0, a, h->dProto, h->prefetch_timeout_us, h->pf_groups_rti);
    hipLaunchKernelGGL(mlp_stream_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, a, (const float *)h->dFrag, (const double *)d_other,
                       (const double *)d_ego_ref, (const double *)d_ego_xy, h->dForceAB[0], h->dForceAB[1], rows, np1,
                       h->cfg.r_horiz * h->cfg.r_horiz, other_stride, (const int *)d_other_index, h->dProto, peer_mapped(d_other));
    hipLaunchKernelGGL(prefetch_done_kernel, dim3(1), dim3(64), 0, a, h->dProto);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_prefetch_join(ndp_handle *h, void *stream)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->aux) return 0;
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    NDP_HIP(h, hipEventRecord(h->evJoin, h->aux));
    NDP_HIP(h, hipStreamWaitEvent(stream ? (hipStream_t)stream : h->stream, h->evJoin, 0));
    return 0;
}

int ndp_step_device_prefetched(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, void *d_u0, void *stream)
{
    Entry g(h, d_x0 && d_xr && d_ur && d_u0, stream, "ndp_step_device_prefetched");
    if (g.rc) return g.rc;
    int rc = ensure_prefetch(h);
    if (rc) return rc;
    return g.noted(launch_rti(h, (const double *)d_x0, (const double *)d_xr, (const double *)d_ur, nullptr, (double *)d_u0, nullptr, g.s,
                              nullptr, nullptr, true));
}

int ndp_prefetch_stats(ndp_handle *h, unsigned long long *out4 /* [5] */)
{
    if (!h || !out4) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    out4[0] = out4[1] = out4[2] = out4[3] = out4[4] = 0;
    if (!h->aux) return 0;
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = wait_all(h);
    if (rc) return rc;
    NDP_HIP(h, hipStreamSynchronize(h->aux));
    std::vector<unsigned long long> w(PF_EPOCH);
    NDP_HIP(h, hipMemcpy(w.data(), h->dProto, (size_t)PF_EPOCH * 8, hipMemcpyDeviceToHost));
    out4[0] = w[PF_CUR_M]; out4[1] = w[PF_RTI_C2] / h->pf_groups_rti;
    out4[2] = (unsigned)(w[PF_MISSED] & 0xffffffffu); out4[3] = (unsigned)(w[PF_GATE_TIMEOUT] & 0xffffffffu);
    out4[4] = (unsigned)(w[PF_SLOW] & 0xffffffffu);
    return 0;
}

void *ndp_device_force_slot(ndp_handle *h, int slot) { return h && (slot == 0 || slot == 1) ? h->dForceAB[slot] : nullptr; }

// ---- host-array step: ndp_step_begin (pack -> H2D -> kernel -> D2H, nothing waits) + ndp_step_end (wait, hand the results over)
static int ensure_slots(ndp_handle *h)
{
    if (h->slots_ready) return 0;
    for (int i = 0; i < 2; ++i) {
        ndp_handle::HostSlot &sl = h->slot[i];
        // (only what is missing: a call that failed part-way left the members it did allocate, and they are reused -- ndp_destroy frees them)
        if (!sl.hIn) NDP_HIP(h, hipHostMalloc((void **)&sl.hIn, h->in_bytes, hipHostMallocDefault));
        if (!sl.hOut) {
            NDP_HIP(h, hipHostMalloc((void **)&sl.hOut, h->out_all, hipHostMallocDefault));
            memset(sl.hOut, 0, h->out_bytes);
        }
        if (!sl.evOut) NDP_HIP(h, hipEventCreateWithFlags(&sl.evOut, hipEventDisableTiming));
    }
    // pack threads: NDP_PACK_THREADS, else half the cores this process may really use, at most 8; the caller packs too, so small blocks
    // need none.  (Rounds 3-5 counted the machine's hardware threads: in a container whose CPU quota is a fraction of the machine that
    // put seven spinning threads on two or three cores' worth of time -- the same ndp_step_begin / _end leg measured 4.5 M solves/s on one
    // box and 11.5 M on another.)
    int nt = 0;
    h->host_cores = usable_cores();
    if (const char *e = getenv("NDP_PACK_THREADS")) nt = atoi(e);
    else if (h->in_bytes > 2 * PACK_CHUNK) nt = (h->host_cores / 2 > 8 ? 8 : h->host_cores / 2) - 1;
    h->pack_threads = nt > 0 ? (nt > 64 ? 64 : nt) : 0;
    h->pool.reset(new (std::nothrow) PackPool(h->pack_threads));
    if (!h->pool) { h->err = "ensure_slots: out of memory"; return -4; }
    h->slots_ready = true;
    return 0;
}

static int step_begin_locked(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                             const double *other, const double *ego_xy, bool want_iter, double *dump, bool f_f64 = false)
{
    const size_t B = h->cfg.batch;
    hipStream_t s = h->stream;
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = ensure_slots(h);
    if (rc) return rc;
    if (h->slots_busy == 2) { h->err = "ndp_step_begin: two steps are already in flight (call ndp_step_end first)"; return -14; }
    if (h->ev_pending && (rc = wait_all(h))) return rc;       // work a caller left on its own stream comes first
    ndp_handle::HostSlot &sl = h->slot[h->slot_head];
    // the slot's previous use is over: its results were handed out by ndp_step_end (busy is false), so the kernel that read
    // its input mirror and wrote its output mirror has completed and both are free to overwrite
    // the block of THIS step: the arrays that were given, one behind the other (256-byte aligned), so that one transfer moves
    // exactly what the kernel reads; neighbour windows as their 6 position / velocity columns
    struct Seg { size_t off; const void *src; size_t len; size_t rows, row_len, src_stride; };
    Seg segs[6];
    int ns = 0;
    size_t o = 0;
    auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    auto add = [&](const void *src, size_t len, size_t rows = 0, size_t row_len = 0, size_t src_stride = 0) {
        segs[ns] = {o, src, len, rows, row_len, src_stride};
        o += up256(len);
        return segs[ns++].off;
    };
    const size_t rows_o = B * (size_t)(h->cfg.N + 1);
    const size_t o_x0 = add(x0, B * NX * 8), o_xr = add(xr, nxs(h) * 8), o_ur = add(ur, nus(h) * 8);
    const size_t o_f = f ? add(f, nfs(h) * (f_f64 ? 8 : 4)) : 0;
    const size_t o_other = other ? add(other, rows_o * 6 * 8, rows_o, 6 * 8, NX * 8) : 0;
    const size_t o_ego = ego_xy ? add(ego_xy, B * 2 * 8) : 0;
    const size_t used = o;          // <= in_bytes (the mirror holds every array at full width)
    std::vector<PackJob> jobs;
    for (int i = 0; i < ns; ++i) {
        if (segs[i].rows) {
            const size_t rows_per = PACK_CHUNK / segs[i].src_stride;
            for (size_t r = 0; r < segs[i].rows; r += rows_per) {
                const size_t n = segs[i].rows - r < rows_per ? segs[i].rows - r : rows_per;
                jobs.push_back({sl.hIn + segs[i].off + r * segs[i].row_len, (const unsigned char *)segs[i].src + r * segs[i].src_stride,
                                segs[i].row_len, n, segs[i].src_stride});
            }
            continue;
        }
        for (size_t c = 0; c < segs[i].len; c += PACK_CHUNK) {
            const size_t n = segs[i].len - c < PACK_CHUNK ? segs[i].len - c : PACK_CHUNK;
            jobs.push_back({sl.hIn + segs[i].off + c, (const unsigned char *)segs[i].src + c, n});
        }
    }
    const int nj = (int)jobs.size();
    PackPool &pool = *h->pool;
    const auto tp0 = std::chrono::steady_clock::now();
    pool.post(jobs.data(), nj);      // from here to pool.finish() nothing returns early: the workers read `jobs`
    for (int i = 0; i < nj; ++i) pool.wait_job(i);
    pool.finish();
    const auto tp1 = std::chrono::steady_clock::now();
    // Zero-copy: the kernel reads the input mirror itself over PCIe and writes u0 | status | iterations (| the new iterate, when
    // asked for) into the output mirror itself: page-locked host memory, device-accessible, no DMA operation.  (One transfer of
    // the block per step into an HBM copy on a stream of its own, beside the previous tick's kernel, was built and measured in
    // four sessions: 85-103 us per step at batch 1024 against 90-96 this way, 290-343 against 315-342 at 4096 -- between 8 %
    // better and 10 % worse, one tick at a time always 5 % worse.  PCIe moves ~40-48 GB/s here whoever issues the reads.  Not kept.)
    const unsigned char *ib = sl.hIn;
    (void)used;
    Neigh nb;
    nb.other = other ? (const double *)(ib + o_other) : nullptr;
    nb.stride = 6;
    nb.ego_xy = ego_xy ? (const double *)(ib + o_ego) : nullptr;
    StepOut so;
    so.status = (int *)(sl.hOut + h->off_st); so.iters = (int *)(sl.hOut + h->off_it);
    if (want_iter) { so.Xm = (double *)(sl.hOut + h->out_bytes); so.Um = so.Xm + nxs(h); }
    so.f_f64 = f_f64;
    // one packet less between the kernel's end and the host seeing it: the completion event rides on the step's last dispatch packet
    const bool ext_done = !dump && h->cfg.qp_precision == 0 && (!other || can_fuse(h)) && !getenv("NDP_HOST_EVENT_RECORD");
    if (ext_done) so.done = sl.evOut;
    rc = enqueue_step(h, (const double *)(ib + o_x0), (const double *)(ib + o_xr), (const double *)(ib + o_ur),
                      f ? (const float *)(ib + o_f) : nullptr, nb, (double *)(sl.hOut + h->off_u0), dump ? h->sdbg : nullptr, s, &so);
    if (rc) return rc;
    // (sl.evOut was marked by the step's own dispatch packet -- so.done -- unless the step ran the separate downwash launch path,
    // a debug dump or a precision study, where it is recorded behind the launches as usual)
    if (!ext_done) NDP_HIP(h, hipEventRecord(sl.evOut, s));
    sl.busy = true; sl.want_iter = want_iter; sl.dump = dump;
    h->host_us[0] = std::chrono::duration<double, std::micro>(tp1 - tp0).count();
    h->host_us[1] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tp1).count();
    h->slot_head ^= 1;
    ++h->slots_busy;
    return 0;
}

static int step_end_locked(ndp_handle *h, double *u0, double *X_out, double *U_out, int32_t *status_out, int32_t *iters_out)
{
    const size_t B = h->cfg.batch;
    if (h->slots_busy == 0) { h->err = "ndp_step_end: no step in flight (ndp_step_begin first)"; return -14; }
    if (h->tslot[h->slot_tail].busy) { h->err = "ndp_step_end: the oldest call in flight is a tick (ndp_tick_end it)"; return -14; }
    ndp_handle::HostSlot &sl = h->slot[h->slot_tail];
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    if ((X_out || U_out) && !sl.want_iter) { h->err = "ndp_step_end: the iterate was not requested at ndp_step_begin (flags bit 0)"; return -15; }
    // the step is a few tens of microseconds from done: poll the event before blocking on it (a blocking wait adds its wake-up)
    const auto tw0 = std::chrono::steady_clock::now();
    hipError_t e = hipErrorNotReady;
    for (int spin = 0; spin < 4000 && e == hipErrorNotReady; ++spin) e = hipEventQuery(sl.evOut);
    if (e == hipErrorNotReady) e = hipEventSynchronize(sl.evOut);
    if (e == hipSuccess && sl.dump)
        e = hipMemcpy(sl.dump, h->sdbg, (size_t)(lds_doubles(h->cfg.N) + DBG_EXTRA) * 8, hipMemcpyDeviceToHost);
    sl.busy = false;
    h->slot_tail ^= 1;
    --h->slots_busy;
    NDP_HIP(h, e);
    const auto tw1 = std::chrono::steady_clock::now();
    const unsigned char *ho = sl.hOut;
    if (u0) memcpy(u0, ho + h->off_u0, B * NU * 8);
    const int32_t *st = (const int32_t *)(ho + h->off_st);
    if (status_out) memcpy(status_out, st, B * 4);
    if (iters_out) copy_ipm_iters(iters_out, reinterpret_cast<const int32_t *>(ho + h->off_it), B);
    if (X_out) memcpy(X_out, ho + h->out_bytes, nxs(h) * 8);
    if (U_out) memcpy(U_out, ho + h->out_bytes + nxs(h) * 8, nus(h) * 8);
    int w = 0;
    for (size_t i = 0; i < B; ++i) w = st[i] > w ? st[i] : w;
    h->host_us[2] = std::chrono::duration<double, std::micro>(tw1 - tw0).count();
    h->host_us[3] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tw1).count();
    return w;
}

int ndp_debug_host_info(ndp_handle *h, int32_t *out3)
{
    if (!h || !out3) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    out3[0] = (int32_t)std::thread::hardware_concurrency();
    out3[1] = h->slots_ready ? h->host_cores : usable_cores();
    out3[2] = h->slots_ready ? h->pack_threads : -1;
    return 0;
}

int ndp_debug_rti_launched(ndp_handle *h, uint64_t *mask, int32_t *out3)
{
    if (!h) return -1;
    if (mask) *mask = h->rti_launched.exchange(0, std::memory_order_relaxed);
    if (out3) {
        out3[0] = RTI_KERNELS;
        out3[1] = h->waves;
        out3[2] = can_fuse(h) ? 1 : 0;
    }
    return 0;
}

int ndp_debug_host_timing(ndp_handle *h, double *out4)
{
    if (!h || !out4) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    for (int i = 0; i < 4; ++i) out4[i] = h->host_us[i];
    return 0;
}

int ndp_step_begin(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                   const double *other, const double *ego_xy, int flags)
{
    if (!h || !x0 || !xr || !ur) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    return step_begin_locked(h, x0, xr, ur, f, other, ego_xy, (flags & 1) != 0, nullptr);
}

int ndp_step_end(ndp_handle *h, double *u0, double *X_out, double *U_out, int32_t *status_out, int32_t *iters_out)
{
    if (!h || !u0) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    return step_end_locked(h, u0, X_out, U_out, status_out, iters_out);
}

// The synchronous form: begin + end under ONE lock (a concurrent caller cannot slip a step in between).
static int step_host(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                     const double *other, const double *ego_xy, double *u0, double *X_out, double *U_out,
                     int32_t *status_out, int32_t *iters_out, double *dump, bool f_f64 = false)
{
    if (!h || !x0 || !xr || !ur || !u0) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->slots_busy) { h->err = "ndp_step: steps begun with ndp_step_begin are still in flight (ndp_step_end them first)"; return -14; }
    int rc = step_begin_locked(h, x0, xr, ur, f, other, ego_xy, X_out || U_out, dump, f_f64);
    if (rc) return rc;
    return step_end_locked(h, u0, X_out, U_out, status_out, iters_out);
}

int ndp_step(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
             const double *other, const double *ego_xy, double *u0)
{
    return step_host(h, x0, xr, ur, f, other, ego_xy, u0, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int ndp_step_ex(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                const double *other, const double *ego_xy, double *u0, double *X_out, double *U_out,
                int32_t *status_out, int32_t *iters_out)
{
    return step_host(h, x0, xr, ur, f, other, ego_xy, u0, X_out, U_out, status_out, iters_out, nullptr);
}

int ndp_step_ex_f64(ndp_handle *h, const double *x0, const double *xr, const double *ur, const double *f, double *u0,
                    double *X_out, double *U_out, int32_t *status_out, int32_t *iters_out)
{
    return step_host(h, x0, xr, ur, reinterpret_cast<const float *>(f), nullptr, nullptr, u0, X_out, U_out, status_out, iters_out, nullptr, f != nullptr);
}

int ndp_step_debug(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                   const double *other, const double *ego_xy, double *u0, double *lds_dump)
{
    if (h && h->cfg.batch != 1) { h->err = "ndp_step_debug: batch must be 1"; return -9; }
    return step_host(h, x0, xr, ur, f, other, ego_xy, u0, nullptr, nullptr, nullptr, nullptr, lds_dump);
}

int ndp_downwash_device(ndp_handle *h, const void *d_other, const void *d_ego_ref, const void *d_ego_xy,
                        void *d_f_out, void *stream)
{
    Entry g(h, d_other && d_ego_ref && d_f_out, stream);
    if (g.rc) return g.rc;
    Neigh nb;
    nb.other = (const double *)d_other; nb.ego_xy = (const double *)d_ego_xy;
    return g.noted(launch_mlp(h, nb, (const double *)d_ego_ref, (float *)d_f_out, g.s));
}


// measurement hook: the LDS-free downwash kernel (see mlp_stream_kernel) on a caller's stream
int ndp_debug_downwash_stream_device(ndp_handle *h, const void *d_other, const void *d_ego_ref, const void *d_ego_xy,
                                     void *d_f_out, void *stream)
{
    Entry g(h, d_other && d_ego_ref && d_f_out, stream);
    if (g.rc) return g.rc;
    if (!h->have_mlp) { h->err = "downwash requested but ndp_set_mlp_weights was never called"; return -6; }
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * np1;
    const int ntiles = (rows + 31) / 32;
    hipLaunchKernelGGL(mlp_stream_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, g.s, (const float *)h->dFrag, (const double *)d_other,
                       (const double *)d_ego_ref, (const double *)d_ego_xy, (float *)d_f_out, (float *)d_f_out, rows, np1,
                       h->cfg.r_horiz * h->cfg.r_horiz, NX, (const int *)nullptr, (unsigned long long *)nullptr, peer_mapped(d_other));
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

int ndp_downwash(ndp_handle *h, const double *other, const double *ego_ref, const double *ego_xy, float *f_out)
{
    Entry g(h, other && ego_ref && f_out);
    if (g.rc) return g.rc;
    hipStream_t s = h->stream;
    NDP_HIP(h, hipMemcpyAsync(h->sother, other, nxs(h) * 8, hipMemcpyHostToDevice, s));
    NDP_HIP(h, hipMemcpyAsync(h->sxr, ego_ref, nxs(h) * 8, hipMemcpyHostToDevice, s));
    if (ego_xy) NDP_HIP(h, hipMemcpyAsync(h->sego, ego_xy, (size_t)h->cfg.batch * 2 * 8, hipMemcpyHostToDevice, s));
    Neigh nb;
    nb.other = h->sother; nb.ego_xy = ego_xy ? h->sego : nullptr;
    int rc = launch_mlp(h, nb, h->sxr, h->dForce, s);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(f_out, h->dForce, nfs(h) * 4, hipMemcpyDeviceToHost, s));
    return g.synced(0);
}

int ndp_get_iterate(ndp_handle *h, double *X, double *U)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if (X) NDP_HIP(h, hipMemcpy(X, h->dX, nxs(h) * 8, hipMemcpyDefault));
    if (U) NDP_HIP(h, hipMemcpy(U, h->dU, nus(h) * 8, hipMemcpyDefault));
    return 0;
}

int ndp_set_iterate(ndp_handle *h, const double *X, const double *U)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if (X) NDP_HIP(h, hipMemcpy(h->dX, X, nxs(h) * 8, hipMemcpyDefault));
    if (U) NDP_HIP(h, hipMemcpy(h->dU, U, nus(h) * 8, hipMemcpyDefault));
    NDP_HIP(h, hipMemset(h->dAct, 0, act_bytes(h)));
    return 0;
}

int ndp_get_active_set(ndp_handle *h, int32_t *sweeps, int8_t *act)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    const size_t B = (size_t)h->cfg.batch;
    if (sweeps) {
        NDP_HIP(h, hipMemcpy(sweeps, h->lastIters, B * 4, hipMemcpyDefault));
        for (size_t i = 0; i < B; ++i) sweeps[i] = (int32_t)((uint32_t)sweeps[i] >> ITERS_SWEEP_SHIFT);
    }
    if (act) NDP_HIP(h, hipMemcpy(act, h->dAct, act_bytes(h), hipMemcpyDefault));
    return 0;
}

int ndp_set_active_set(ndp_handle *h, const int8_t *act)
{
    Entry g(h, act);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    const size_t n = act_bytes(h);
    for (size_t i = 0; i < n; ++i)
        if (act[i] < -1 || act[i] > 1) { h->err = "ndp_set_active_set: entries are -1, 0 or +1"; return -1; }
    NDP_HIP(h, hipMemcpy(h->dAct, act, n, hipMemcpyDefault));
    return 0;
}

int ndp_get_status(ndp_handle *h, int32_t *status, int32_t *ipm_iters)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if (status) NDP_HIP(h, hipMemcpy(status, h->lastStatus, (size_t)h->cfg.batch * 4, hipMemcpyDefault));
    if (ipm_iters) {
        NDP_HIP(h, hipMemcpy(ipm_iters, h->lastIters, (size_t)h->cfg.batch * 4, hipMemcpyDefault));
        copy_ipm_iters(ipm_iters, ipm_iters, (size_t)h->cfg.batch);
    }
    return 0;
}

// ---- f3: hover-throttle estimator + actuator command (reference constants: params/estimator_params.py:13-18)
static ThrCfg thr_cfg(const ndp_handle *h)
{
    const double ts = 0.02, tau = 0.05;
    ThrCfg c;
    c.a1 = (2.0 * tau - ts) / (2.0 * tau + ts);
    c.a2 = 2.0 / (2.0 * tau + ts);
    c.hm = 1.0 / h->cfg.mass;
    c.g = h->cfg.gravity;
    c.R = 1.225; c.Q0 = 0.1; c.Q1 = 0.1;
    c.mass = h->cfg.mass;
    return c;
}

int ndp_throttle_reset(ndp_handle *h)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    hipLaunchKernelGGL(throttle_reset_kernel, dim3((h->cfg.batch + 255) / 256), dim3(256), 0, h->stream, h->dThr, 50.0, h->cfg.batch);
    NDP_HIP(h, hipGetLastError());
    return g.synced(0);
}

// The host-pointer forms below hold the handle's lock from the first staging copy to the read-back: they share the
// staging area sThr (and sx0 / sxr / sur / su0 of the step), which a concurrent call must not overwrite in between.
static int launch_throttle(ndp_handle *h, const double *d_vz, const double *d_throttle, double *d_k, hipStream_t s)
{
    hipLaunchKernelGGL(throttle_kernel, dim3((h->cfg.batch + 255) / 256), dim3(256), 0, s, thr_cfg(h), h->dThr, d_vz, d_throttle, d_k, h->cfg.batch);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_throttle_update_device(ndp_handle *h, const void *d_vz, const void *d_throttle, void *d_k, void *stream)
{
    Entry g(h, d_vz && d_throttle && d_k, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_throttle(h, (const double *)d_vz, (const double *)d_throttle, (double *)d_k, g.s));
}

int ndp_throttle_update(ndp_handle *h, const double *vz, const double *throttle, double *k)
{
    Entry g(h, vz && throttle && k);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch;
    NDP_HIP(h, hipMemcpyAsync(h->sThr, vz, B * 8, hipMemcpyHostToDevice, h->stream));
    NDP_HIP(h, hipMemcpyAsync(h->sThr + B, throttle, B * 8, hipMemcpyHostToDevice, h->stream));
    int rc = launch_throttle(h, h->sThr, h->sThr + B, h->sThr + 2 * B, h->stream);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(k, h->sThr + 2 * B, B * 8, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

static int launch_actuator(ndp_handle *h, const double *d_u0, const double *d_k, double *d_cmd, hipStream_t s)
{
    hipLaunchKernelGGL(actuator_kernel, dim3((h->cfg.batch + 255) / 256), dim3(256), 0, s, d_u0, d_k, d_cmd, h->cfg.mass, h->cfg.batch);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_actuator_cmd_device(ndp_handle *h, const void *d_u0, const void *d_k, void *d_cmd, void *stream)
{
    Entry g(h, d_u0 && d_k && d_cmd, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_actuator(h, (const double *)d_u0, (const double *)d_k, (double *)d_cmd, g.s));
}

int ndp_actuator_cmd(ndp_handle *h, const double *u0, const double *k, double *cmd)
{
    Entry g(h, u0 && k && cmd);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch;
    NDP_HIP(h, hipMemcpyAsync(h->sThr + 2 * B, k, B * 8, hipMemcpyHostToDevice, h->stream));
    NDP_HIP(h, hipMemcpyAsync(h->sThr + 3 * B, u0, B * 32, hipMemcpyHostToDevice, h->stream));
    int rc = launch_actuator(h, h->sThr + 3 * B, h->sThr + 2 * B, h->sThr + 7 * B, h->stream);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(cmd, h->sThr + 7 * B, B * 32, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

int ndp_throttle_get_state(ndp_handle *h, double *state)
{
    Entry g(h, state);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch;
    int rc = wait_all(h);
    if (rc) return rc;
    std::vector<double> soa(B * 8);
    NDP_HIP(h, hipMemcpy(soa.data(), h->dThr, B * 64, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < B; ++v)
        for (int i = 0; i < 8; ++i) state[v * 8 + i] = soa[(size_t)i * B + v];
    return 0;
}

// ---- f2: follower reference relay
int ndp_relay_reset(ndp_handle *h)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    NDP_HIP(h, hipMemsetAsync(h->dRelay, 0, (size_t)h->cfg.batch * 32, h->stream));
    return g.synced(0);
}

int ndp_relay_formation(ndp_handle *h, const double *form, double *offset_out)
{
    Entry g(h, form);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch;
    NDP_HIP(h, hipMemcpyAsync(h->sThr, form, B * 24, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(relay_formation_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, 0.8, h->dRelay, (const double *)h->sThr, (int)B);
    NDP_HIP(h, hipGetLastError());
    std::vector<double> st(offset_out ? B * 4 : 0);
    if (offset_out) NDP_HIP(h, hipMemcpyAsync(st.data(), h->dRelay, B * 32, hipMemcpyDeviceToHost, h->stream));
    int rc = g.synced(0);
    if (rc) return rc;
    for (size_t v = 0; offset_out && v < B; ++v)
        for (int a = 0; a < 3; ++a) offset_out[v * 3 + a] = st[v * 4 + a];
    return 0;
}

static int launch_relay_reference(ndp_handle *h, const double *d_xr_lead, double *d_xr_out, hipStream_t s)
{
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * np1;
    const size_t pieces = (size_t)rows * 5, per_block = 256 * RELAY_UNROLL;
    hipLaunchKernelGGL(relay_reference_kernel, dim3((unsigned)((pieces + per_block - 1) / per_block)), dim3(256), 0, s, (const double *)h->dRelay, d_xr_lead, d_xr_out, rows, np1);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_relay_reference_device(ndp_handle *h, const void *d_xr_lead, void *d_xr_out, void *stream)
{
    Entry g(h, d_xr_lead && d_xr_out, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_relay_reference(h, (const double *)d_xr_lead, (double *)d_xr_out, g.s));
}

int ndp_relay_reference(ndp_handle *h, const double *xr_lead, double *xr_out)
{
    Entry g(h, xr_lead && xr_out);
    if (g.rc) return g.rc;
    NDP_HIP(h, hipMemcpyAsync(h->sother, xr_lead, nxs(h) * 8, hipMemcpyHostToDevice, h->stream));
    int rc = launch_relay_reference(h, h->sother, h->sxr, h->stream);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(xr_out, h->sxr, nxs(h) * 8, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

// ---- f1: reference window generation
int ndp_ref_set_trajectory(ndp_handle *h, int n_seg, const double *coeff_x, const double *coeff_y, const double *coeff_z,
                           const double *coeff_yaw, const double *time_cum, const double *time_seg, const double *final_pt)
{
    Entry g(h, n_seg >= 1 && coeff_x && coeff_y && coeff_z && coeff_yaw && time_cum && time_seg && final_pt);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch, S = (size_t)n_seg;
    std::vector<double> host(traj_view(nullptr, B, S).doubles);     // (the hints start at 0)
    const TrajView v = traj_view(host.data(), B, S);
    for (size_t b = 0; b < B; ++b)
        for (size_t s = 0; s < S; ++s) {
            double *d = v.coeff + (b * S + s) * 28;          // interleave the four message arrays per segment
            for (int i = 0; i < 8; ++i) {
                d[i] = coeff_x[(b * S + s) * 8 + i];
                d[8 + i] = coeff_y[(b * S + s) * 8 + i];
                d[16 + i] = coeff_z[(b * S + s) * 8 + i];
            }
            for (int i = 0; i < 4; ++i) d[24 + i] = coeff_yaw[(b * S + s) * 4 + i];
        }
    memcpy(v.tcum, time_cum, B * (S + 1) * 8);
    memcpy(v.tseg, time_seg, B * S * 8);
    memcpy(v.fpt, final_pt, B * 3 * 8);
    for (double *c : v.segc) memset(c, 0xFF, B * SEGC_PER * 8);
    int rc = wait_all(h);
    if (rc) return rc;
    if (h->dTraj) { (void)hipFree(h->dTraj); h->dTraj = nullptr; }
    NDP_HIP(h, hipMalloc((void **)&h->dTraj, v.doubles * 8));
    NDP_HIP(h, hipMemcpy(h->dTraj, host.data(), v.doubles * 8, hipMemcpyHostToDevice));
    h->segc_par = 0;
    h->traj_seg = n_seg;
    return 0;
}

static RefCfg ref_cfg(const ndp_handle *h, double toff)
{
    return RefCfg{h->cfg.batch, h->cfg.N, h->traj_seg, h->cfg.dt, h->cfg.mass, h->cfg.gravity, toff};
}

// enqueue helper (no locking): windows at node-0 times d_t[b] (or 0 when null) + toff
static int launch_ref_window(ndp_handle *h, const double *d_t, double toff, double *d_xr, double *d_ur, hipStream_t s)
{
    if (!h->dTraj) { h->err = "ndp_ref_window: ndp_ref_set_trajectory was never called"; return -11; }
    const TrajView tv = traj_view(h);
    const int rows = h->cfg.batch * (h->cfg.N + 1);
    hipLaunchKernelGGL(ref_window_kernel, dim3((rows + REF_ROWS - 1) / REF_ROWS), dim3(REF_ROWS), 0, s, ref_cfg(h, toff), tv.coeff, tv.tcum, tv.tseg,
                       tv.fpt, d_t, d_xr, d_ur);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_ref_window_device(ndp_handle *h, const void *d_t, void *d_xr, void *d_ur, void *stream)
{
    Entry g(h, d_t && d_xr && d_ur, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_ref_window(h, (const double *)d_t, 0.0, (double *)d_xr, (double *)d_ur, g.s));
}

int ndp_ref_window(ndp_handle *h, const double *t, double *xr, double *ur)
{
    Entry g(h, t && xr && ur);
    if (g.rc) return g.rc;
    NDP_HIP(h, hipMemcpyAsync(h->sThr, t, (size_t)h->cfg.batch * 8, hipMemcpyHostToDevice, h->stream));
    int rc = launch_ref_window(h, h->sThr, 0.0, h->sxr, h->sur, h->stream);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(xr, h->sxr, nxs(h) * 8, hipMemcpyDeviceToHost, h->stream));
    NDP_HIP(h, hipMemcpyAsync(ur, h->sur, nus(h) * 8, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

// ---- f1, the reference's sliding list (ref_list_* kernels; layout: RingGeom)
static int list_ring(const ndp_handle *h) { return ring_geom(h).ring(); }

static int list_alloc(ndp_handle *h)
{
    if (h->dRingX) return 0;
    const RingGeom rg = ring_geom(h);
    NDP_HIP(h, hipMalloc((void **)&h->dRingX, (size_t)h->cfg.batch * (rg.px() + rg.pu()) * 8));
    h->dRingU = h->dRingX + (size_t)h->cfg.batch * rg.px();
    return 0;
}

// points at (d_t ? d_t[b] : 0) + toff + i * ts_nmpc, i = 0 .. npts-1, become list entries j0 + i (dup0: point 0 also entry j0 - 1)
static int launch_list_fill(ndp_handle *h, const double *d_t, double toff, int npts, unsigned long long j0, int dup0, hipStream_t s)
{
    if (!h->dTraj) { h->err = "ndp_ref_list: ndp_ref_set_trajectory was never called"; return -11; }
    const TrajView tv = traj_view(h);
    const int n = h->cfg.batch * npts;
    const int bs = npts == 1 ? 64 : 256;        // one point per vehicle (the per-tick advance): small blocks spread over the CUs
    hipLaunchKernelGGL(ref_list_fill_kernel, dim3((n + bs - 1) / bs), dim3(bs), 0, s, ref_cfg(h, toff), tv.coeff, tv.tcum, tv.tseg, tv.fpt, d_t,
                       h->cfg.ts_nmpc, npts, j0, ring_geom(h), dup0, h->dRingX, h->dRingU);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_ref_list_reset(ndp_handle *h)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = list_alloc(h);
    if (rc) return rc;
    if ((rc = wait_all(h))) return rc;
    h->list_n = 0;
    // entries 1 .. ring-1 = the points at i * ts_nmpc, i = 0 .. ring-2; the first one duplicated as entry 0 (:62-76)
    return g.synced(launch_list_fill(h, nullptr, 0.0, list_ring(h) - 1, 1, 1, h->stream));
}

int ndp_ref_list_fix_pt(ndp_handle *h, const double *x_odom, int quirk_b1)
{
    Entry g(h, x_odom);
    if (g.rc) return g.rc;
    int rc = list_alloc(h);
    if (rc) return rc;
    if ((rc = wait_all(h))) return rc;
    h->list_n = 0;
    NDP_HIP(h, hipMemcpyAsync(h->sThr, x_odom, (size_t)h->cfg.batch * 80, hipMemcpyHostToDevice, h->stream));
    const RingGeom rg = ring_geom(h);
    const size_t n = (size_t)h->cfg.batch * rg.step * 2 * rg.np1;
    hipLaunchKernelGGL(ref_list_fix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const double *)h->sThr,
                       quirk_b1 ? h->cfg.mass * h->cfg.gravity : h->cfg.gravity, h->cfg.batch, rg, h->dRingX, h->dRingU);
    NDP_HIP(h, hipGetLastError());
    return g.synced(0);
}

// pop the oldest entry, append the point at trajectory time t + T_horizon (get_nmpc_pts, :79-93)
static int list_advance(ndp_handle *h, const double *d_t, hipStream_t s)
{
    if (!h->dRingX) { h->err = "ndp_ref_list_advance: no list (ndp_ref_list_reset / ndp_ref_list_fix_pt first)"; return -11; }
    const int rc = launch_list_fill(h, d_t, h->cfg.N * h->cfg.dt, 1, h->list_n + (unsigned long long)list_ring(h), 0, s);
    if (rc) return rc;                                             // nothing was launched (e.g. no trajectory): the list stays as it is
    ++h->list_n;
    return 0;
}

int ndp_ref_list_advance_device(ndp_handle *h, const void *d_t, void *stream)
{
    Entry g(h, d_t, stream);
    if (g.rc) return g.rc;
    return g.noted(list_advance(h, (const double *)d_t, g.s));
}

static int launch_list_window(ndp_handle *h, double *d_xr, double *d_ur, hipStream_t s)
{
    if (!h->dRingX) { h->err = "ndp_ref_list_window: no list (ndp_ref_list_reset / ndp_ref_list_fix_pt first)"; return -11; }
    const size_t n = (size_t)h->cfg.batch * (5 * (h->cfg.N + 1) + 2 * h->cfg.N), per_block = 256 * WIN_UNROLL;
    hipLaunchKernelGGL(ref_list_window_kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), 0, s, (const double *)h->dRingX,
                       (const double *)h->dRingU, ring_geom(h), h->list_n, h->cfg.batch, d_xr, d_ur);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_ref_list_window_device(ndp_handle *h, void *d_xr, void *d_ur, void *stream)
{
    Entry g(h, d_xr && d_ur, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_list_window(h, (double *)d_xr, (double *)d_ur, g.s));
}

// t == NULL: only read the current window (get_nmpc_ref_from_long_list); else advance first (get_nmpc_pts)
int ndp_ref_list_window(ndp_handle *h, const double *t, double *xr, double *ur)
{
    Entry g(h, xr && ur);
    if (g.rc) return g.rc;
    int rc = 0;
    if (t) {
        NDP_HIP(h, hipMemcpyAsync(h->sThr, t, (size_t)h->cfg.batch * 8, hipMemcpyHostToDevice, h->stream));
        if ((rc = list_advance(h, h->sThr, h->stream))) return rc;
    }
    if ((rc = launch_list_window(h, h->sxr, h->sur, h->stream))) return rc;
    NDP_HIP(h, hipMemcpyAsync(xr, h->sxr, nxs(h) * 8, hipMemcpyDeviceToHost, h->stream));
    NDP_HIP(h, hipMemcpyAsync(ur, h->sur, nus(h) * 8, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

// ---- the node's control tick, end to end on the device (nmpc_node.py:211-231; kernels: rti_kernel<..., TICK>, or tick_pre_kernel + rti_kernel)
int ensure_tick(ndp_handle *h)
{
    if (h->dTickThrust) return 0;
    NDP_HIP(h, hipMalloc((void **)&h->dTickThrust, (size_t)h->cfg.batch * 8));
    NDP_HIP(h, hipMemsetAsync(h->dTickThrust, 0, (size_t)h->cfg.batch * 8, h->stream));     // AttitudeTarget(): thrust 0 (nmpc_node.py:104)
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    return 0;
}

int ndp_tick_config(ndp_handle *h, const int32_t *other_index, int gate_on_odometry)
{
    Entry g(h, true, nullptr, "ndp_tick_config");
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if ((rc = ensure_tick(h))) return rc;
    const size_t B = h->cfg.batch;
    bool any = false;
    if (other_index)
        for (size_t i = 0; i < B; ++i) {
            if (other_index[i] >= (int32_t)B) { h->err = "ndp_tick_config: other_index names an instance outside the handle"; return -2; }
            any = any || other_index[i] >= 0;
        }
    if (any && !h->cfg.use_fd) { h->err = "ndp_tick_config: neighbours (downwash) need use_fd = 1 (NDP model)"; return -8; }
    if (any && !h->have_mlp) { h->err = "ndp_tick_config: neighbours given but ndp_set_mlp_weights was never called"; return -6; }
    if (any) {
        if (!h->dTickIndex) NDP_HIP(h, hipMalloc((void **)&h->dTickIndex, B * 4));
        NDP_HIP(h, hipMemcpy(h->dTickIndex, other_index, B * 4, hipMemcpyHostToDevice));
    } else if (h->dTickIndex) {
        (void)hipFree(h->dTickIndex);
        h->dTickIndex = nullptr;
    }
    h->tick_gate = gate_on_odometry != 0;
    h->tick_remote = nullptr;
    return 0;
}

// The control tick with neighbours on OTHER ranks (nmpc_node.py:116-133,229-230 -> ndp_nmpc_leader_node.py:40,60-76: every vehicle
// publishes its window every tick, the leader consumes its neighbour's): the neighbour rows come from the caller's exchange buffer, and
// a tick is three enqueues with the exchange between the first two and the last:
//   ndp_tick_advance_device    list advance (+ estimator): this rank's window of the tick is complete, node N included
//   ndp_tick_window_pv_device  that window's position / velocity columns [B][N+1][6] -> the exchange's send buffer   ... exchange ...
//   ndp_tick_step_device       the control step (gate + network + RTI + actuator command), neighbour rows from the gathered windows
// Same arithmetic as the one-launch tick with the neighbour in the same handle (bit-equal: tests/test_tick.py).
int ndp_tick_config_remote(ndp_handle *h, const void *d_windows, int stride, int64_t rows, const int32_t *other_index, int gate_on_odometry)
{
    Entry g(h, d_windows && other_index, nullptr, "ndp_tick_config_remote");
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if ((rc = ensure_tick(h))) return rc;
    if (stride != 6 && stride != NX) { h->err = "ndp_tick_config_remote: stride must be 6 (position / velocity columns) or 10"; return -13; }
    if (!h->cfg.use_fd) { h->err = "ndp_tick_config_remote: neighbours (downwash) need use_fd = 1 (NDP model)"; return -8; }
    if (!h->have_mlp) { h->err = "ndp_tick_config_remote: ndp_set_mlp_weights was never called"; return -6; }
    if (!can_fuse(h)) { h->err = "ndp_tick_config_remote: serves the shapes whose downwash is fused into the control step (N + 1 <= 32, fp64)"; return -12; }
    const size_t B = h->cfg.batch;
    for (size_t i = 0; i < B; ++i)
        if ((int64_t)other_index[i] >= rows) { h->err = "ndp_tick_config_remote: other_index names a row outside the window buffer"; return -2; }
    if (!h->dTickIndex) NDP_HIP(h, hipMalloc((void **)&h->dTickIndex, B * 4));
    NDP_HIP(h, hipMemcpy(h->dTickIndex, other_index, B * 4, hipMemcpyHostToDevice));
    h->tick_gate = gate_on_odometry != 0;
    h->tick_remote = (const double *)d_windows;
    h->tick_remote_stride = stride;
    return 0;
}

// nmpc_ctl.reset(*ref_pub.get_nmpc_ref_from_long_list()) (nmpc_node.py:92,151-152): the iterate := the list's current window
int ndp_tick_reset(ndp_handle *h)
{
    Entry g(h, true, nullptr, "ndp_tick_reset");
    if (g.rc) return g.rc;
    if (h->slots_busy) { h->err = "ndp_tick_reset: ticks are still in flight (ndp_tick_end them first)"; return -14; }
    int rc = wait_all(h);
    if (rc) return rc;
    if ((rc = launch_list_window(h, h->dX, h->dU, h->stream))) return rc;
    NDP_HIP(h, hipMemsetAsync(h->dAct, 0, act_bytes(h), h->stream));      // reset(): the QPs start from an empty active set
    return g.synced(0);
}

// tick_pre_kernel's arguments.  adv: the list is advanced, its new entry the point at t[b] (device-accessible), or t_all for every vehicle
// when t is null, + T_horizon.  est: the estimator runs on vz[B] (null: column 5 of x_odom[B][10]) and throttle[B] (null: the thrust
// this handle commanded last tick).  pv: the advanced window's position / velocity columns also go there (ndp_xchg_tick_begin).
}  // extern "C"      (tick_pre: C++ linkage, it returns a TickPre)
TickPre tick_pre(const ndp_handle *h, bool adv, const double *t, double t_all, bool est, const double *x_odom, const double *vz,
                 const double *throttle, double *pv)
{
    TickPre a{};
    a.cf = ref_cfg(h, h->cfg.N * h->cfg.dt);
    if (adv) {
        const TrajView tv = traj_view(h);
        a.coeff = tv.coeff; a.tcum = tv.tcum; a.tseg = tv.tseg; a.fpt = tv.fpt; a.seg_hint = tv.hint;
    }
    a.t = t; a.t_all = t_all; a.advance = adv ? 1 : 0;
    a.rg = ring_geom(h);
    a.j_new = h->list_n + (unsigned long long)a.rg.ring();
    a.rx = h->dRingX; a.ru = h->dRingU;
    a.thr = thr_cfg(h); a.st = h->dThr;
    a.vz = vz ? vz : x_odom + 5; a.vz_pitch = vz ? 1 : NX;
    a.throttle = throttle ? throttle : h->dTickThrust;
    a.est = est ? 1 : 0;
    if (pv) { a.pv = pv; a.pv_slot = a.rg.slot(h->list_n + 1); }
    return a;
}
extern "C" {

// tick_pre_kernel, one thread per vehicle
void launch_tick_pre(const TickPre &a, hipStream_t s)
{
    hipLaunchKernelGGL(tick_pre_kernel, dim3((a.cf.B + 63) / 64), dim3(64), 0, s, a);
}

// the same work inside the one-launch tick (TickArgs), which reads the trajectory's segment cache the last such tick wrote
static TickArgs tick_args(const ndp_handle *h, const TickPre &a)
{
    TickArgs ta{};
    if (a.advance) {
        const TrajView tv = traj_view(h);
        ta.coeff = a.coeff; ta.tcum = a.tcum; ta.tseg = a.tseg; ta.fpt = a.fpt; ta.n_seg = a.cf.n_seg;
        ta.segc = tv.segc[h->segc_par]; ta.segc_wr = tv.segc[h->segc_par ^ 1];
    }
    ta.t = a.t; ta.t_all = a.t_all; ta.advance = a.advance;
    ta.toff = a.cf.toff; ta.mass = a.cf.mass; ta.g = a.cf.g;
    ta.j_new = a.j_new; ta.new_slot = a.rg.slot(a.j_new);
    ta.rg = a.rg; ta.rx = a.rx; ta.ru = a.ru;
    ta.thr = a.thr; ta.st = a.st;
    ta.vz = a.vz; ta.vz_pitch = a.vz_pitch; ta.throttle = a.throttle;
    ta.est = a.est;
    return ta;
}

// One tick's launches on `s`.  Every pointer is device-accessible (HBM or page-locked host memory): x_odom[B][10]; t[B] or null (the
// list is not advanced: hover at a fixed point, or a vehicle between two trajectories); vz[B] or null (column 5 of x_odom);
// throttle[B] or null (the thrust this handle commanded last tick); cmd[B][4]; u0_copy[B][4] or null.
// adv: the list is advanced; its times are t[B] (device-accessible), or t_all for every vehicle when t is null.
static int tick_enqueue(ndp_handle *h, hipStream_t s, const double *x_odom, bool adv, const double *t, double t_all, const double *vz,
                        const double *throttle, int flags, double *cmd, double *u0_copy, StepOut so)
{
    int rc = ensure_tick(h);
    if (rc) return rc;
    if (!h->dRingX) { h->err = "ndp_tick: no reference list (ndp_ref_list_fix_pt, or ndp_ref_set_trajectory + ndp_ref_list_reset, first)"; return -11; }
    if (adv && !h->dTraj) { h->err = "ndp_tick: a trajectory time was given but ndp_ref_set_trajectory was never called"; return -11; }
    if (h->tick_remote) { h->err = "ndp_tick: neighbours come from an exchange buffer (ndp_tick_config_remote): a tick is ndp_tick_advance_device, the exchange, ndp_tick_step_device"; return -17; }
    const int B = h->cfg.batch;
    const RingGeom rg = ring_geom(h);
    const bool est = (flags & TICK_ESTIMATE) != 0;
    // ONE launch per tick (rti_kernel<..., TICK>: list advance and estimator inside the control step's waves) for the reference
    // configuration's compile-time kernels; any other shape: tick_pre_kernel in front of the control step.  NDP_TICK_FORM=pre forces
    // the two-launch form (A/B measurements).
    static const bool force_pre = [] { const char *e = getenv("NDP_TICK_FORM"); return e && !strcmp(e, "pre"); }();
    // (a neighbour's window node N is made INSIDE the one-launch kernel's fused downwash: without the fused form -- can_fuse -- the
    // two-launch form serves)
    const bool one_launch = !force_pre && h->cfg.N == 20 && h->cfg.n_rti == 1 && h->waves == 4 && h->cfg.qp_precision == 0 &&
                            (!h->dTickIndex || can_fuse(h));
    // the list position and the cache's copies move on only when the tick's launches have been accepted (below)
    const unsigned long long n_after = h->list_n + (adv ? 1ull : 0ull);
    TickArgs ta;
    if (adv || est) {
        const TickPre a = tick_pre(h, adv, t, t_all, est, x_odom, vz, throttle);
        if (one_launch) {
            ta = tick_args(h, a);
            so.tick = &ta;
        } else {
            launch_tick_pre(a, s);
            NDP_HIP(h, hipGetLastError());
        }
    }
    const size_t slot = rg.slot(n_after);
    Neigh nb;
    if (h->dTickIndex) {
        nb.other = h->dRingX + slot * 10; nb.stride = NX; nb.index = h->dTickIndex; nb.pitch = rg.px();
        if (h->tick_gate) { nb.ego_xy = x_odom; nb.ego_pitch = NX; }
    }
    so.xr_pitch = rg.px(); so.ur_pitch = rg.pu();
    // nmpc_u_2_att_tgt is the control step's own last store (RtiIo::cmd): no third launch.  k_throttle = row 1 of the estimator's state
    // (k_throttle_init until the estimator has run)
    so.cmd = cmd; so.kthr = h->dThr + (size_t)B; so.thrust_keep = h->dTickThrust;
    rc = enqueue_step(h, x_odom, h->dRingX + slot * 10, h->dRingU + slot * 4, nullptr, nb, u0_copy ? u0_copy : h->su0, nullptr, s, &so);
    if (rc) return rc;               // (refused: the list stays where it was -- an entry the pre-launch may have written lies beyond every window)
    h->list_n = n_after;
    if (adv && so.tick) h->segc_par ^= 1;
    return 0;
}

int ndp_tick_advance_device(ndp_handle *h, const void *d_x_odom, const void *d_t, const void *d_vz, const void *d_throttle, int flags, void *stream)
{
    Entry g(h, d_x_odom, stream, "ndp_tick_advance_device");
    if (g.rc) return g.rc;
    int rc = ensure_tick(h);
    if (rc) return rc;
    if (!h->dRingX) { h->err = "ndp_tick_advance: no reference list (ndp_ref_list_fix_pt, or ndp_ref_set_trajectory + ndp_ref_list_reset, first)"; return -11; }
    const bool adv = d_t != nullptr, est = (flags & TICK_ESTIMATE) != 0, uni = adv && (flags & TICK_T_UNIFORM);
    if (adv && !h->dTraj) { h->err = "ndp_tick_advance: a trajectory time was given but ndp_ref_set_trajectory was never called"; return -11; }
    if (adv || est) {
        const TickPre a = tick_pre(h, adv, uni ? nullptr : (const double *)d_t, uni ? *(const double *)d_t : 0.0, est, (const double *)d_x_odom,
                                   (const double *)d_vz, (const double *)d_throttle);
        launch_tick_pre(a, g.s);
        NDP_HIP(h, hipGetLastError());
        if (adv) ++h->list_n;
    }
    return g.noted(0);
}

int ndp_tick_window_pv_device(ndp_handle *h, void *d_pv, void *stream)
{
    Entry g(h, d_pv, stream, "ndp_tick_window_pv_device");
    if (g.rc) return g.rc;
    if (!h->dRingX) { h->err = "ndp_tick_window_pv: no reference list"; return -11; }
    const RingGeom rg = ring_geom(h);
    launch_pack_pv_list(h->dRingX + rg.slot(h->list_n) * 10, rg.px(), h->cfg.N + 1, (double *)d_pv, h->cfg.batch, g.s);
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

// stage 3 on `s` (h->mu held): the control step of the window at list position `pos`, neighbour rows out of `windows`
int tick_step_enqueue(ndp_handle *h, hipStream_t s, const double *x_odom, double *cmd, double *u0, const double *windows, unsigned long long pos)
{
    if (!h->tick_remote) { h->err = "ndp_tick_step: ndp_tick_config_remote first (neighbours in the same handle: ndp_tick_device)"; return -17; }
    if (!h->dRingX) { h->err = "ndp_tick_step: no reference list"; return -11; }
    const RingGeom rg = ring_geom(h);
    const size_t slot = rg.slot(pos), B = h->cfg.batch;
    Neigh nb;
    nb.other = windows; nb.stride = h->tick_remote_stride; nb.index = h->dTickIndex;
    if (h->tick_gate) { nb.ego_xy = x_odom; nb.ego_pitch = NX; }
    StepOut so;
    so.xr_pitch = rg.px(); so.ur_pitch = rg.pu();
    so.cmd = cmd; so.kthr = h->dThr + B; so.thrust_keep = h->dTickThrust;
    return enqueue_step(h, x_odom, h->dRingX + slot * 10, h->dRingU + slot * 4, nullptr, nb, u0 ? u0 : h->su0, nullptr, s, &so);
}

int ndp_tick_step_device(ndp_handle *h, const void *d_x_odom, void *d_cmd, void *d_u0, void *stream)
{
    Entry g(h, d_x_odom && d_cmd, stream, "ndp_tick_step_device");
    if (g.rc) return g.rc;
    return g.noted(tick_step_enqueue(h, g.s, (const double *)d_x_odom, (double *)d_cmd, (double *)d_u0, h->tick_remote, h->list_n));
}

int ndp_tick_device(ndp_handle *h, const void *d_x_odom, const void *d_t, const void *d_vz, const void *d_throttle, int flags,
                    void *d_cmd, void *d_u0, void *stream)
{
    Entry g(h, d_x_odom && d_cmd, stream, "ndp_tick_device");
    if (g.rc) return g.rc;
    const bool uni = d_t && (flags & TICK_T_UNIFORM);       // (then d_t is HOST memory: one double, read here)
    return g.noted(tick_enqueue(h, g.s, (const double *)d_x_odom, d_t != nullptr, uni ? nullptr : (const double *)d_t, uni ? *(const double *)d_t : 0.0,
                                (const double *)d_vz, (const double *)d_throttle, flags, (double *)d_cmd, (double *)d_u0, StepOut()));
}

// host arrays: the inputs of a tick are packed into a slot's page-locked input mirror -- x_odom | t | vz | throttle, 80 + 24 bytes per
// vehicle at most -- which the tick's kernels read over PCIe themselves; cmd | status | iterations (| u0) are written into the
// slot's page-locked output mirror by the kernels (the same two slots, the same zero-copy scheme as ndp_step_begin / _end)
static int tick_begin_locked(ndp_handle *h, const double *x_odom, const double *t, const double *vz, const double *throttle, int flags)
{
    const size_t B = h->cfg.batch;
    int rc = ensure_slots(h);
    if (rc) return rc;
    if (h->slots_busy == 2) { h->err = "ndp_tick_begin: two ticks are already in flight (call ndp_tick_end first)"; return -14; }
    if (h->ev_pending && (rc = wait_all(h))) return rc;
    ndp_handle::HostSlot &sl = h->slot[h->slot_head];
    const auto tp0 = std::chrono::steady_clock::now();
    unsigned char *ib = sl.hIn;
    const size_t o_t = up256(B * NX * 8), o_vz = o_t + up256(B * 8), o_th = o_vz + up256(B * 8);    // (<= in_bytes: the mirror holds a whole step's inputs)
    memcpy(ib, x_odom, B * NX * 8);
    const bool uni = t && (flags & TICK_T_UNIFORM);         // one time for every vehicle: it travels in the kernel arguments
    if (t && !uni) memcpy(ib + o_t, t, B * 8);
    if (vz) memcpy(ib + o_vz, vz, B * 8);
    if (throttle) memcpy(ib + o_th, throttle, B * 8);
    const auto tp1 = std::chrono::steady_clock::now();
    StepOut so;
    so.status = (int *)(sl.hOut + h->off_st); so.iters = (int *)(sl.hOut + h->off_it);
    so.done = sl.evOut;
    const bool want_u0 = (flags & TICK_WANT_U0) != 0;
    rc = tick_enqueue(h, h->stream, (const double *)ib, t != nullptr, t && !uni ? (const double *)(ib + o_t) : nullptr, uni ? t[0] : 0.0,
                      vz ? (const double *)(ib + o_vz) : nullptr,
                      throttle ? (const double *)(ib + o_th) : nullptr, flags, (double *)(sl.hOut + h->off_u0),
                      want_u0 ? (double *)(sl.hOut + h->out_bytes) : nullptr, so);
    if (rc) return rc;
    sl.busy = true; sl.want_iter = false; sl.dump = nullptr;
    h->tslot[h->slot_head].busy = true; h->tslot[h->slot_head].want_u0 = want_u0;
    h->host_us[0] = std::chrono::duration<double, std::micro>(tp1 - tp0).count();
    h->host_us[1] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tp1).count();
    h->slot_head ^= 1;
    ++h->slots_busy;
    return 0;
}

static int tick_end_locked(ndp_handle *h, double *cmd, double *u0, int32_t *status_out, int32_t *iters_out)
{
    const size_t B = h->cfg.batch;
    if (h->slots_busy == 0 || !h->tslot[h->slot_tail].busy) { h->err = "ndp_tick_end: no tick in flight (ndp_tick_begin first)"; return -14; }
    ndp_handle::HostSlot &sl = h->slot[h->slot_tail];
    if (u0 && !h->tslot[h->slot_tail].want_u0) { h->err = "ndp_tick_end: u0 was not requested at ndp_tick_begin (flags bit 1)"; return -15; }
    const auto tw0 = std::chrono::steady_clock::now();
    hipError_t e = hipErrorNotReady;
    for (int spin = 0; spin < 4000 && e == hipErrorNotReady; ++spin) e = hipEventQuery(sl.evOut);
    if (e == hipErrorNotReady) e = hipEventSynchronize(sl.evOut);
    sl.busy = false;
    h->tslot[h->slot_tail].busy = false;
    h->slot_tail ^= 1;
    --h->slots_busy;
    NDP_HIP(h, e);
    const auto tw1 = std::chrono::steady_clock::now();
    const unsigned char *ho = sl.hOut;
    memcpy(cmd, ho + h->off_u0, B * NU * 8);
    if (u0) memcpy(u0, ho + h->out_bytes, B * NU * 8);
    const int32_t *st = (const int32_t *)(ho + h->off_st);
    if (status_out) memcpy(status_out, st, B * 4);
    if (iters_out) copy_ipm_iters(iters_out, reinterpret_cast<const int32_t *>(ho + h->off_it), B);
    int w = 0;
    for (size_t i = 0; i < B; ++i) w = st[i] > w ? st[i] : w;
    h->host_us[2] = std::chrono::duration<double, std::micro>(tw1 - tw0).count();
    h->host_us[3] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tw1).count();
    return w;
}

int ndp_tick_begin(ndp_handle *h, const double *x_odom, const double *t, const double *vz, const double *throttle, int flags)
{
    Entry g(h, x_odom, nullptr, "ndp_tick_begin");
    return g.rc ? g.rc : tick_begin_locked(h, x_odom, t, vz, throttle, flags);
}

int ndp_tick_end(ndp_handle *h, double *cmd, double *u0, int32_t *status_out, int32_t *ipm_iters_out)
{
    Entry g(h, cmd, nullptr, "ndp_tick_end");
    return g.rc ? g.rc : tick_end_locked(h, cmd, u0, status_out, ipm_iters_out);
}

int ndp_tick(ndp_handle *h, const double *x_odom, const double *t, const double *vz, const double *throttle, int flags,
             double *cmd, double *u0, int32_t *status_out, int32_t *ipm_iters_out)
{
    Entry g(h, x_odom && cmd, nullptr, "ndp_tick");      // (begin and end under the one lock)
    if (g.rc) return g.rc;
    if (h->slots_busy) { h->err = "ndp_tick: steps / ticks begun earlier are still in flight (end them first)"; return -14; }
    int rc = tick_begin_locked(h, x_odom, t, vz, throttle, flags | (u0 ? TICK_WANT_U0 : 0));
    if (rc) return rc;
    return tick_end_locked(h, cmd, u0, status_out, ipm_iters_out);
}

// ---- f4: plant step
static int launch_plant(ndp_handle *h, double *d_x, const double *d_u, const double *d_f, double dt, int substeps, hipStream_t s)
{
    hipLaunchKernelGGL(plant_kernel, dim3((h->cfg.batch + 255) / 256), dim3(256), 0, s, d_x, d_u, d_f, dt / substeps, substeps,
                       1.0 / h->cfg.mass, h->cfg.gravity, h->cfg.batch);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_plant_step_device(ndp_handle *h, void *d_x, const void *d_u, const void *d_f, double dt, int substeps, void *stream)
{
    Entry g(h, d_x && d_u && substeps >= 1, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_plant(h, (double *)d_x, (const double *)d_u, (const double *)d_f, dt, substeps, g.s));
}

int ndp_plant_step(ndp_handle *h, double *x, const double *u, const double *f, double dt, int substeps)
{
    Entry g(h, x && u && substeps >= 1);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch;
    NDP_HIP(h, hipMemcpyAsync(h->sx0, x, B * 80, hipMemcpyHostToDevice, h->stream));
    NDP_HIP(h, hipMemcpyAsync(h->su0, u, B * 32, hipMemcpyHostToDevice, h->stream));
    if (f) NDP_HIP(h, hipMemcpyAsync(h->sThr, f, B * 24, hipMemcpyHostToDevice, h->stream));
    int rc = launch_plant(h, h->sx0, h->su0, f ? h->sThr : nullptr, dt, substeps, h->stream);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(x, h->sx0, B * 80, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

// ---- f4: closed-loop rollout, everything enqueued back to back on one stream, nothing returns to the host in between
int ndp_rollout_device(ndp_handle *h, int ticks, double t0, double dt_tick, int substeps, void *d_x, void *d_log, void *stream)
{
    Entry g(h, ticks >= 1 && substeps >= 1 && d_x, stream, "ndp_rollout_device");
    if (g.rc) return g.rc;
    hipStream_t s = g.s;
    if (h->cfg.use_fd) { h->err = "ndp_rollout_device: the rollout drives the NMPC model (use_fd = 0)"; return -8; }
    const size_t B = h->cfg.batch;
    double *x = (double *)d_x, *log = (double *)d_log;
    int rc = launch_ref_window(h, nullptr, t0, h->sxr, h->sur, s);     // reset(xr, ur) at the first tick's reference
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(h->dX, h->sxr, nxs(h) * 8, hipMemcpyDefault, s));
    NDP_HIP(h, hipMemcpyAsync(h->dU, h->sur, nus(h) * 8, hipMemcpyDefault, s));
    for (int k = 0; k < ticks; ++k) {
        if (k > 0 && (rc = launch_ref_window(h, nullptr, t0 + k * dt_tick, h->sxr, h->sur, s))) return rc;
        if ((rc = launch_rti(h, x, h->sxr, h->sur, nullptr, h->su0, nullptr, s))) return rc;
        if ((rc = launch_plant(h, x, h->su0, nullptr, dt_tick, substeps, s))) return rc;
        if (log) NDP_HIP(h, hipMemcpyAsync(log + (size_t)k * B * NX, x, B * NX * 8, hipMemcpyDeviceToDevice, s));
    }
    return g.noted(0);
}

// test/profiling hook: every instance writes its phase stamps (shader clock) to [B][NDP_NSTAMP] doubles
int ndp_debug_stamps(ndp_handle *h, int enable, double *out)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    NDP_HIP(h, hipDeviceSynchronize());
    const size_t bytes = (size_t)h->cfg.batch * NDP_NSTAMP * 8;
    if (out && h->dStamps) NDP_HIP(h, hipMemcpy(out, h->dStamps, bytes, hipMemcpyDeviceToHost));
    if (enable && !h->dStamps) {
        NDP_HIP(h, hipMalloc((void **)&h->dStamps, bytes));
        NDP_HIP(h, hipMemset(h->dStamps, 0, bytes));
    } else if (!enable && h->dStamps) {
        (void)hipFree(h->dStamps);
        h->dStamps = nullptr;
    }
    return 0;
}

void *ndp_device_iterate_x(ndp_handle *h) { return h ? h->dX : nullptr; }
void *ndp_device_iterate_u(ndp_handle *h) { return h ? h->dU : nullptr; }
void *ndp_device_force(ndp_handle *h) { return h ? h->dForce : nullptr; }
int ndp_work_queue_enabled(ndp_handle *h) { return h ? (int)h->use_queue : -1; }

// ---- the sensitivity buffers: created on enabling, NaN until a step has written them
static int nan_buffer(ndp_handle *h, double *&p, size_t n)
{
    if (p) return 0;
    NDP_HIP(h, hipMalloc((void **)&p, n * 8));
    NDP_HIP(h, hipMemsetAsync(p, 0xff, n * 8, h->stream));
    return 0;
}
static void drop_buffer(double *&p) { if (p) (void)hipFree(p); p = nullptr; }
static int copy_out(ndp_handle *h, double *dst, const double *src, size_t n)
{
    if (dst) NDP_HIP(h, hipMemcpy(dst, src, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

// ---- initial-state sensitivities (rti_sens_kernel, RtiWave::sens_out)
int ndp_sens_enable(ndp_handle *h, int level)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (level < 0 || level > 2) { h->err = "ndp_sens_enable: level must be 0 (off), 1 (du0/dx0) or 2 (also dU/dx0 and dX/dx0)"; return -2; }
    if (level > 0) {
        if (slots_for(h->cfg.N) > 3) { h->err = "ndp_sens_enable: sensitivities are served for N <= 27 only (the five-slot kernels of N >= 28 have none)"; return -2; }
        if (h->cfg.qp_precision != 0) { h->err = "ndp_sens_enable: sensitivities need qp_precision 0 (the fp64 product path)"; return -2; }
        if (h->cfg.n_rti != 1) { h->err = "ndp_sens_enable: sensitivities need n_rti = 1 (the derivative of the step's one QP)"; return -2; }
        if (h->waves != 4 && h->waves != 2) { h->err = "ndp_sens_enable: the sensitivity kernels run 2 or 4 instances per workgroup"; return -2; }
    }
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = wait_all(h);                 // (steps in flight may still write the buffers)
    if (rc) return rc;
    const size_t B = h->cfg.batch, N = h->cfg.N;
    const size_t n0 = B * (size_t)sens_u0_pitch(), nu = B * (size_t)sens_u_pitch((int)N), nx = B * (size_t)sens_x_pitch((int)N);
    if (level < 2) { drop_buffer(h->dSensU); drop_buffer(h->dSensX); }
    if (level == 0) { for (double **p : {&h->dSensU0, &h->dPSensXr, &h->dPSensUr, &h->dPSensF}) drop_buffer(*p); h->sens_level = 0; return 0; }
    if ((rc = nan_buffer(h, h->dSensU0, n0))) return rc;
    if (level == 2 && ((rc = nan_buffer(h, h->dSensU, nu)) || (rc = nan_buffer(h, h->dSensX, nx)))) return rc;
    const int lds_bytes = (int)((size_t)h->lds_per_wave * sizeof(double) * h->waves);
    for (const RtiKern &k : k_rti)
        if (k.sens) NDP_HIP(h, hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    h->sens_level = level;
    return 0;
}

int ndp_sens_level(ndp_handle *h) { return h ? h->sens_level : -1; }

int ndp_get_sens(ndp_handle *h, double *du0_dx0, double *dU_dx0, double *dX_dx0)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->sens_level < 1) { h->err = "ndp_get_sens: sensitivities are not enabled (ndp_sens_enable)"; return -2; }
    if ((dU_dx0 || dX_dx0) && h->sens_level < 2) { h->err = "ndp_get_sens: dU/dx0 and dX/dx0 need sensitivity level 2"; return -2; }
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = wait_all(h);
    if (rc) return rc;
    const size_t B = h->cfg.batch;
    if ((rc = copy_out(h, du0_dx0, h->dSensU0, B * sens_u0_pitch()))) return rc;
    if ((rc = copy_out(h, dU_dx0, h->dSensU, B * sens_u_pitch(h->cfg.N)))) return rc;
    return copy_out(h, dX_dx0, h->dSensX, B * sens_x_pitch(h->cfg.N));
}

void *ndp_device_sens_u0(ndp_handle *h) { return h ? h->dSensU0 : nullptr; }
void *ndp_device_sens_u(ndp_handle *h) { return h ? h->dSensU : nullptr; }
void *ndp_device_sens_x(ndp_handle *h) { return h ? h->dSensX : nullptr; }

// ---- parameter sensitivities (rti_psens_kernel, RtiWave::psens_out)
int ndp_sens_params_enable(ndp_handle *h, int on)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (on && h->sens_level < 1) {
        h->err = "ndp_sens_params_enable: parameter sensitivities need initial-state sensitivities on (ndp_sens_enable(h, 1 or 2) first)";
        return -2;
    }
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = wait_all(h);                 // (steps in flight may still write the buffers)
    if (rc) return rc;
    if (!on) {
        for (double **p : {&h->dPSensXr, &h->dPSensUr, &h->dPSensF}) drop_buffer(*p);
        return 0;
    }
    const size_t B = h->cfg.batch;
    const int N = h->cfg.N;
    if ((rc = nan_buffer(h, h->dPSensXr, B * (size_t)psens_xr_pitch(N))) || (rc = nan_buffer(h, h->dPSensUr, B * (size_t)psens_ur_pitch(N))) ||
        (rc = nan_buffer(h, h->dPSensF, B * (size_t)psens_f_pitch(N))))
        return rc;
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    return 0;
}

int ndp_sens_params_enabled(ndp_handle *h) { return h ? (int)(h->dPSensXr != nullptr) : -1; }

int ndp_get_sens_params(ndp_handle *h, double *du0_dxr, double *du0_dur, double *du0_df)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->dPSensXr) { h->err = "ndp_get_sens_params: parameter sensitivities are not enabled (ndp_sens_params_enable)"; return -2; }
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = wait_all(h);
    if (rc) return rc;
    const size_t B = h->cfg.batch;
    const int N = h->cfg.N;
    if ((rc = copy_out(h, du0_dxr, h->dPSensXr, B * psens_xr_pitch(N)))) return rc;
    if ((rc = copy_out(h, du0_dur, h->dPSensUr, B * psens_ur_pitch(N)))) return rc;
    return copy_out(h, du0_df, h->dPSensF, B * psens_f_pitch(N));
}

void *ndp_device_sens_xr(ndp_handle *h) { return h ? h->dPSensXr : nullptr; }
void *ndp_device_sens_ur(ndp_handle *h) { return h ? h->dPSensUr : nullptr; }
void *ndp_device_sens_f(ndp_handle *h) { return h ? h->dPSensF : nullptr; }

// ---- adjoint of the control step (rti_vjp_kernel, RtiWave::vjp_out)
void *ndp_device_active_set(ndp_handle *h) { return h ? h->dAct : nullptr; }

// What the derivative kernels that recompute a recorded step share (rti_vjp_kernel, rti_wvjp_kernel, rti_jvp_kernel).  Their entries take
// the step's inputs and the tape it started from, never written (the recompute advances a copy: two calls on one tape give the same result),
// and optionally return the recomputed u0 and status for the caller to check against the recorded ones.
struct Tape {
    const void *x0, *xr, *ur, *f, *X_lin, *U_lin, *act_lin;
    void *u0_check, *status_check;
};

// The refusals all of those entries make, in their order: the configuration's and the required pointers', then `own` -- the entry's
// refusals of its own arguments, or null -- then the force's.  Empty: none.  noun: what the entry's texts call the derivative.
static std::string recompute_refusal(const ndp_cfg &c, const char *noun, const Tape &t, const char *own)
{
    const std::string the = std::string("the ") + noun;
    if (c.n_rti != 1) return the + " needs n_rti = 1 (the derivative of the step's one QP)";
    if (c.qp_precision != 0) return the + " needs qp_precision 0 (the fp64 product path)";
    if (slots_for(c.N) > 3) return the + " is served for N <= 27 only (the five-slot kernels of N >= 28 have none)";
    if (!t.x0 || !t.xr || !t.ur || !t.X_lin || !t.U_lin) return "x0, xr, ur and the tape's iterate (X_lin, U_lin) are required";
    if (own) return own;
    if (t.f && !c.use_fd) return "a disturbance force needs use_fd = 1 (NDP model)";
    return "";
}

// The launch: the handle's workspace (first call), the tape copied into it on the entry's stream, the step's kernel arguments on that
// copy, then the kernel for the horizon (fn20: the compile-time N = 20, else fn0) with a1, a2 behind them (a2: null if it takes two).
static int recompute_launch(ndp_handle *h, Entry &g, const Tape &t, const void *fn20, const void *fn0, void *a1, void *a2)
{
    const ndp_cfg &c = h->cfg;
    const size_t B = c.batch;
    hipStream_t s = g.s;
    if (!h->dVjp) {
        NDP_HIP(h, hipMalloc((void **)&h->dVjp, (nxs(h) + nus(h) + B * NU) * 8));
        NDP_HIP(h, hipMalloc((void **)&h->dVjpSt, B * 2 * 4));
        NDP_HIP(h, hipMalloc((void **)&h->dVjpAct, act_bytes(h)));
    }
    double *X = h->dVjp, *U = X + nxs(h), *u0 = U + nus(h);
    int *st = h->dVjpSt, *it = st + B;
    NDP_HIP(h, hipMemcpyAsync(X, t.X_lin, nxs(h) * 8, hipMemcpyDeviceToDevice, s));
    NDP_HIP(h, hipMemcpyAsync(U, t.U_lin, nus(h) * 8, hipMemcpyDeviceToDevice, s));
    if (t.act_lin) NDP_HIP(h, hipMemcpyAsync(h->dVjpAct, t.act_lin, act_bytes(h), hipMemcpyDeviceToDevice, s));
    else NDP_HIP(h, hipMemsetAsync(h->dVjpAct, 0, act_bytes(h), s));
    BatchPtrs bp{h->dKC, h->dTables, (const double *)t.x0, (const double *)t.xr, (const double *)t.ur, (const float *)t.f, X, U,
                 t.u0_check ? (double *)t.u0_check : u0, t.status_check ? (int *)t.status_check : st, it, nullptr, nullptr, nullptr, nullptr,
                 (size_t)(c.N + 1) * NX, (size_t)c.N * NU, (size_t)NX, nullptr, nullptr, nullptr, c.mass, 0, h->dVjpAct};
    KernArgs ka{h->P, bp, (int)B, h->lds_per_wave, MlpArgs{}, QueueArgs{}, LateArgs{}, TickArgs{}};
    const int W = h->waves;
    const void *fn = c.N == 20 ? fn20 : fn0;
    void *args[] = {&ka, a1, a2};
    NDP_HIP(h, hipLaunchKernel(fn, dim3((unsigned)((B + W - 1) / W)), dim3(64 * W), args, (size_t)h->lds_per_wave * sizeof(double) * W, s));
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

// model: the entry is ndp_step_vjp_model_device (rti_wvjp_kernel; d_gmodel required), else ndp_step_vjp_device (rti_vjp_kernel)
static int step_vjp(ndp_handle *h, const Tape &t, const void *d_gu0, const void *d_gX, const void *d_gU,
                    void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *stream, bool model, void *d_gmodel)
{
    Entry g(h, true, stream);
    if (g.rc) return g.rc;
    std::string why = recompute_refusal(h->cfg, "adjoint", t, !d_gu0 && !d_gX && !d_gU ? "no upstream gradient (gu0, gX and gU all NULL)" : nullptr);
    if (why.empty() && model && !d_gmodel) why = "gmodel is required (without it: ndp_step_vjp_device)";
    if (!why.empty()) { h->err = std::string(model ? "ndp_step_vjp_model_device: " : "ndp_step_vjp_device: ") + why; return -2; }
    VjpArgs va{(const double *)d_gu0, (const double *)d_gX, (const double *)d_gU, (double *)d_gx0, (double *)d_gxr, (double *)d_gur,
               (double *)d_gf};
    double *gm = (double *)d_gmodel;
    if (model) return recompute_launch(h, g, t, (const void *)rti_wvjp_kernel<20>, (const void *)rti_wvjp_kernel<0>, &va, &gm);
    return recompute_launch(h, g, t, (const void *)rti_vjp_kernel<20>, (const void *)rti_vjp_kernel<0>, &va, nullptr);
}

int ndp_step_vjp_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                        const void *d_X_lin, const void *d_U_lin, const void *d_act_lin,
                        const void *d_gu0, const void *d_gX, const void *d_gU,
                        void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_u0_check, void *d_status_check, void *stream)
{
    return step_vjp(h, Tape{d_x0, d_xr, d_ur, d_f, d_X_lin, d_U_lin, d_act_lin, d_u0_check, d_status_check}, d_gu0, d_gX, d_gU, d_gx0, d_gxr,
                    d_gur, d_gf, stream, false, nullptr);
}

int ndp_step_vjp_model_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                              const void *d_X_lin, const void *d_U_lin, const void *d_act_lin,
                              const void *d_gu0, const void *d_gX, const void *d_gU,
                              void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_gmodel, void *d_u0_check, void *d_status_check,
                              void *stream)
{
    return step_vjp(h, Tape{d_x0, d_xr, d_ur, d_f, d_X_lin, d_U_lin, d_act_lin, d_u0_check, d_status_check}, d_gu0, d_gX, d_gU, d_gx0, d_gxr,
                    d_gur, d_gf, stream, true, d_gmodel);
}

// ---- forward mode of the control step (rti_jvp_kernel, RtiWave::jvp_out): the adjoint's recompute, workspace and tape rules
int ndp_step_jvp_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                        const void *d_X_lin, const void *d_U_lin, const void *d_act_lin, int n_tan,
                        const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf,
                        void *d_du0, void *d_dX, void *d_dU, void *d_u0_check, void *d_status_check, void *stream)
{
    Entry g(h, true, stream);
    if (g.rc) return g.rc;
    const Tape t{d_x0, d_xr, d_ur, d_f, d_X_lin, d_U_lin, d_act_lin, d_u0_check, d_status_check};
    const char *own = nullptr;
    if (n_tan < 1 || n_tan > NDP_JVP_MAX_TANGENTS) own = "n_tan must be 1..8 (directions per call)";
    else if (!d_tx0 && !d_txr && !d_tur && !d_tf) own = "no tangent (tx0, txr, tur and tf all NULL)";
    else if (!d_du0 && !d_dX && !d_dU) own = "no output asked for (du0, dX and dU all NULL)";
    std::string why = recompute_refusal(h->cfg, "derivative", t, own);
    if (why.empty() && d_tf && !h->cfg.use_fd) why = "a force tangent needs use_fd = 1 (NDP model)";
    if (!why.empty()) { h->err = "ndp_step_jvp_device: " + why; return -2; }
    JvpArgs ja{(const double *)d_tx0, (const double *)d_txr, (const double *)d_tur, (const double *)d_tf, (double *)d_du0, (double *)d_dX,
               (double *)d_dU, n_tan};
    return recompute_launch(h, g, t, (const void *)rti_jvp_kernel<20>, (const void *)rti_jvp_kernel<0>, &ja, nullptr);
}

// ---- the model of a live handle: cost weights and mass
int ndp_set_model(ndp_handle *h, const double *Qd, const double *Rd, double mass)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    ndp_cfg c = h->cfg;
    const char *why = nullptr;
    if (Qd)
        for (int i = 0; i < 10; ++i) {
            if (!std::isfinite(Qd[i]) || Qd[i] < 0.0) why = "ndp_set_model: every Qd must be finite and >= 0";
            c.Qd[i] = Qd[i];
        }
    if (Rd)
        for (int i = 0; i < 4; ++i) {
            if (!std::isfinite(Rd[i]) || !(Rd[i] > 0.0)) why = "ndp_set_model: every Rd must be finite and > 0";
            c.Rd[i] = Rd[i];
        }
    if (std::isinf(mass)) why = "ndp_set_model: the mass must be finite (<= 0 or NaN: keep)";
    else if (mass > 0.0) c.mass = mass;
    if (!why && !as_gamma_holds(c, c.Rd))
        why = "ndp_set_model: as_gamma must be at least 1e8 * max(dt * Rd) when as_iter_max > 0 (ndp_create's rule: a weaker pin does not hold "
              "its input on the bound)";
    if (why) { h->err = why; return -2; }
    NDP_HIP(h, hipSetDevice(c.device));
    int rc = wait_all(h);                  // launches in flight read dKC; the copy below must not overtake them
    if (rc) return rc;
    // cfg, P (kernel arguments: the attitude weights, 1 / mass) and the constants table (KC_QD, KC_RD in LDS) change together; every
    // other reader of the mass (plant, actuator command, thrust estimator, reference flatness, BatchPtrs) takes it from cfg per call
    const RtiParams P = to_params(c);
    double kc[KC_HOST];
    fill_kc(P, kc);
    NDP_HIP(h, hipMemcpy(h->dKC, kc, sizeof(kc), hipMemcpyHostToDevice));
    h->cfg = c;
    h->P = P;
    return 0;
}
int ndp_refine_active(ndp_handle *h) { return h ? (int)(h->cfg.ipm_refine > 0 && slots_for(h->cfg.N) <= 3 && h->cfg.qp_precision == 0) : -1; }

int ndp_synchronize(ndp_handle *h)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    return wait_all(h);
}

int ndp_timing_enable(ndp_handle *h, int on)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    for (auto &e : h->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    h->events.clear();
    h->timing = on > 0 ? on : 0;
    h->launch_no[0] = h->launch_no[1] = 0;
    return 0;
}

int ndp_timing_read(ndp_handle *h, const char *name, double *total_ms, int64_t *launches)
{
    if (!h || !name) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    const int kind = (name[0] == 'm') ? 1 : 0;
    double tot = 0.0;
    int64_t n = 0;
    for (auto &e : h->events) {
        if (e.kind != kind) continue;
        NDP_HIP(h, hipEventSynchronize(e.b));
        float ms = 0.0f;
        NDP_HIP(h, hipEventElapsedTime(&ms, e.a, e.b));
        tot += ms;
        ++n;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = n;
    return n ? 0 : -10;
}

}  // extern "C"
