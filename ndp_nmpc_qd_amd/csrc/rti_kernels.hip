// rti_kernels.hip -- the control-step kernels and the one table the host reaches them through.
//   rti_kernel  : one wavefront per OCP instance runs the whole SQP-RTI step (rti_wave.hpp) out of its
//                 LDS slice; 4 waves (= 4 instances) per 256-thread workgroup, one per SIMD of a CU.
//                 FUSED: the downwash MLP tile (mlp_tile.hpp) runs in front of linearise inside the same launch.
//                 QMODE 1 / 2: producer / consumer of the work list (instances whose QP needs the interior point).
//                 TICK: a whole control tick of ndp_tick in the one launch (tick_wave.hpp).
//   rti_sens_kernel / rti_psens_kernel : the step with its initial-state / parameter sensitivities
//   rti_vjp_kernel / rti_wvjp_kernel / rti_jvp_kernel / rti_mjvp_kernel : the step recomputed from a tape, then its adjoint / forward-mode
//                 derivative (w, m: with the cost weights and the mass)
// This unit is by far the longest compile of the library, and host code elsewhere does not name a kernel of it: a table row (RtiId,
// rti_table.hpp) goes through launch_kern, a derivative kernel through recompute_kernel, so an edit of the host's units leaves it alone.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "wave_gfx950.hpp"   // defines the device qualifiers, must precede rti_wave.hpp
#include "cfg_params.hpp"
#include "cond_qp.hpp"
#include "host.hpp"
#include "mlp_common.hpp"
#include "mlp_tile.hpp"
#include "ref_point.hpp"
#include "tick_wave.hpp"

namespace ndp {

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

// Forward mode with directions of the cost weights and the mass beside the data's (ndp_step_jvp_model_device, RtiWave::jvp_out<true>):
// tmodel [B][T][16] = q' [10] | r' [4] | m' | (15: not read by the step), instance-major like the other tangents.  Kernels of their own,
// so that rti_jvp_kernel stays the code it was.
template <int NC>
__global__ __launch_bounds__(256) void rti_mjvp_kernel(KernArgs ka, JvpArgs ja, const double *tmodel)
{
    NDP_RECOMPUTE_PROLOGUE
    const size_t i = (size_t)inst * (size_t)ja.T, nx = (size_t)(N + 1) * NX, nu = (size_t)N * NU, nf = (size_t)(N + 1) * 3;
    const JvpIo jo{ja.tx0 ? ja.tx0 + i * NX : nullptr, ja.txr ? ja.txr + i * nx : nullptr, ja.tur ? ja.tur + i * nu : nullptr,
                   ja.tf ? ja.tf + i * nf : nullptr, ja.du0 ? ja.du0 + i * NU : nullptr, ja.dX ? ja.dX + i * nx : nullptr,
                   ja.dU ? ja.dU + i * nu : nullptr, ja.T, tmodel + i * 16};
    typename Prog::InBuf inb;
    double x0v;
    Prog::issue_first(P, io, inb, x0v);
    Prog::template run<false, true, false, false, false, false, true, true>(P, io, lds, inb, x0v, nullptr, nullptr, nullptr, nullptr, &jo);
}

#undef NDP_RECOMPUTE_PROLOGUE

// ---- Kernels of other concerns that stay in this unit for their code's sake.  Each inlines a device function it shares with the control-step
// kernels (the wave backends' mfma / mfma_k, stage_fragments, seg_locate), and the compiler specialises such a function when one unit
// holds a single caller of it: apart from the control-step kernels these, and the one-launch ticks apart from tick_pre_kernel, come out
// as different code.  Their launchers are at the end of the file; everything else of their concerns is in ndp_hip.hip / downwash.hip /
// tick.hip.
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

// the two-launch tick's first launch (tick.hip: which tick takes it), one thread per vehicle
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

}  // namespace ndp

using namespace ndp;

// RTI_K(...): the rti_kernel instantiation to reference.  The kernel-development builds (never the shipped library) collapse the
// instantiations so that an experiment compiles in 20 s instead of 3 min:
//   -DNDP_DEV_HEADLINE_ONLY  every instantiation but the reference configuration's two onto rti_kernel<3, 4, false, 20>; such a library
//                            serves N = 20, n_rti = 1 only
//   -DNDP_DEV_COND_ONLY      compile / register studies of the condensed study kernels: onto rti_kernel<5, 1, false, 0, 5 or 6>
//   -DNDP_DEV_N40_ONLY       register studies of config 5's shape (scripts/dev_regs.sh): onto rti_kernel<5, 2, false, 40, 0, 2, NDP_DEV_QMODE>
// RTI_SENS_K / RTI_PSENS_K(WAVES, FUSED, NC, QMODE): the rti_sens_kernel / rti_psens_kernel instantiation, collapsed likewise (onto one
// each but in the headline build).
#if defined(NDP_DEV_HEADLINE_ONLY) || defined(NDP_DEV_COND_ONLY) || defined(NDP_DEV_N40_ONLY)
#ifndef NDP_DEV_QMODE      // 1: study the work list's producer form (no interior-point code) in place of the in-place kernel
#define NDP_DEV_QMODE 0
#endif
template <int NSLOT, int WAVES, bool FUSED, int NC = 0, int PREC = 0, int NRC = (NC ? 1 : 0), int QMODE = 0, bool TICK = false>
struct RtiK {
#if defined(NDP_DEV_HEADLINE_ONLY)
    static constexpr auto fn = rti_kernel<3, (WAVES == 2 && NC == 20 ? 2 : 4), (FUSED && NC == 20 && QMODE == 0), 20, 0, 1, NDP_DEV_QMODE, (TICK && NC == 20 && QMODE == 0)>;
#elif defined(NDP_DEV_COND_ONLY)
    static constexpr auto fn = rti_kernel<5, 1, false, 0, (PREC == 6 ? 6 : 5)>;
#else
    static constexpr auto fn = rti_kernel<5, 2, false, 40, 0, 2, NDP_DEV_QMODE>;
#endif
};
#if defined(NDP_DEV_HEADLINE_ONLY)
#define NDP_DEV_SENS_ARGS 4, (FUSED && NC == 20 && QMODE == 0), 20, NDP_DEV_QMODE
#else
#define NDP_DEV_SENS_ARGS 4, false, 20, 0
#endif
template <int WAVES, bool FUSED, int NC, int QMODE>
struct RtiSensK { static constexpr auto fn = rti_sens_kernel<NDP_DEV_SENS_ARGS>; };
template <int WAVES, bool FUSED, int NC, int QMODE>
struct RtiPSensK { static constexpr auto fn = rti_psens_kernel<NDP_DEV_SENS_ARGS>; };
#define RTI_K(...) (RtiK<__VA_ARGS__>::fn)
#define RTI_SENS_K(...) (RtiSensK<__VA_ARGS__>::fn)
#define RTI_PSENS_K(...) (RtiPSensK<__VA_ARGS__>::fn)
#else
#define RTI_K(...) (rti_kernel<__VA_ARGS__>)
#define RTI_SENS_K(...) (rti_sens_kernel<__VA_ARGS__>)
#define RTI_PSENS_K(...) (rti_psens_kernel<__VA_ARGS__>)
#endif

// the shapes the work-queue form of rti_kernel is instantiated for (compile-time horizon and iteration count)
bool queue_shape(const ndp_handle *h)
{
    return h->cfg.qp_precision == 0 &&
           ((h->cfg.N == 20 && h->cfg.n_rti == 1 && h->waves == 4) || (h->cfg.N == 40 && h->cfg.n_rti == 2 && h->waves == 2));
}

// Every control-step kernel the library launches, one entry per instantiation (RTI_K / RTI_SENS_K: collapsed in the development
// builds).  rti_pick chooses the entry of a call; rti_set_lds gives every plain / sensitivity entry its dynamic LDS.
// (The order of the rows is the order the kernels lie in the code object.)
struct RtiKern {
    const void *fn;
    int waves;                 // instances per workgroup: the launch geometry
    bool sens;                 // rti_sens_kernel (KernArgs, SensArgs) or rti_psens_kernel (KernArgs, SensArgs, PSensArgs), else rti_kernel (KernArgs)
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

// One launch of a control-step kernel.  start / stop (either may be null): the timing pair or the step's completion event, carried
// by the dispatch packet itself (hipExtLaunchKernel).  The caller checks hipGetLastError.
void launch_kern(const ndp_handle *h, RtiId id, hipStream_t s, KernArgs &ka, SensArgs &sa, hipEvent_t start, hipEvent_t stop)
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

// The derivative kernels that recompute a recorded step (ndp_hip.hip: recompute_launch), by RecomputeId; n20: the compile-time N = 20.
// lds: the dynamic-LDS ceiling to set instead of the creating handle's own bytes.  The attribute belongs to the function, not to a handle: set
// to the most any handle asks for (ndp_create halves the waves until a workgroup fits 160 KiB), a handle of a short horizon created after one
// of a long horizon cannot lower it under the first one's launches of the shared <0> kernel.
// (The order of the rows is RecomputeId's.)
static const struct { const void *fn20, *fn0; int lds; const char *set; } k_recompute[] = {
    {(const void *)rti_wvjp_kernel<20>, (const void *)rti_wvjp_kernel<0>, 160 * 1024, "hipFuncSetAttribute(rti_wvjp_kernel)"},   // (ndp_step_vjp_model_device)
    {(const void *)rti_jvp_kernel<20>, (const void *)rti_jvp_kernel<0>, 0, "hipFuncSetAttribute(rti_jvp_kernel)"},                // (forward mode: ndp_step_jvp_device)
    {(const void *)rti_vjp_kernel<20>, (const void *)rti_vjp_kernel<0>, 0, "hipFuncSetAttribute(rti_vjp_kernel)"},                // (the adjoint: ndp_step_vjp_device)
    {(const void *)rti_mjvp_kernel<20>, (const void *)rti_mjvp_kernel<0>, 160 * 1024, "hipFuncSetAttribute(rti_mjvp_kernel)"},    // (ndp_step_jvp_model_device)
};
const void *recompute_kernel(RecomputeId id, bool n20) { return n20 ? k_recompute[id].fn20 : k_recompute[id].fn0; }

// allow the big dynamic-LDS launches: the table's plain rows and the recompute kernels (sens false: ndp_create) or its sensitivity rows
// (ndp_sens_enable).  *what: the call a failure came from, for the caller's error text.
hipError_t rti_set_lds(bool sens, int lds_bytes, const char **what)
{
    hipError_t e;
    *what = "hipFuncSetAttribute";
    for (const RtiKern &k : k_rti)
        if (k.sens == sens && (e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)) != hipSuccess) return e;
    if (sens) return hipSuccess;
    for (const auto &k : k_recompute) {
        *what = k.set;
        for (const void *fn : {k.fn20, k.fn0})
            if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds ? k.lds : lds_bytes)) != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- launchers of the kernels kept here (see above)
extern "C" {

int ndp_debug_mfma_probe(const double *a, const double *b, const double *c, double *d)
{
    DevBuf<double> da, db, dc, dd;
    if (da.alloc(64 * 8) != hipSuccess || db.alloc(64 * 8) != hipSuccess || dc.alloc(256 * 8) != hipSuccess || dd.alloc(832 * 8) != hipSuccess)
        return -1;
    (void)hipMemcpy(da, a, 64 * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, b, 64 * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dc, c, 256 * 8, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, 0, da, db, dc, dd);
    const hipError_t e = hipMemcpy(d, dd, 832 * 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : -2;
}

int ndp_debug_mfma_probe_f32(const float *a, const float *b, const float *c, float *d, int mode)
{
    DevBuf<float> da, db, dc, dd;
    if (da.alloc(256 * 4) != hipSuccess || db.alloc(256 * 4) != hipSuccess || dc.alloc(256 * 4) != hipSuccess || dd.alloc(320 * 4) != hipSuccess)
        return -1;
    (void)hipMemcpy(da, a, 256 * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, b, 256 * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(dc, c, 256 * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(mfma_probe32_kernel, dim3(1), dim3(64), 0, 0, da, db, dc, dd, mode);
    const hipError_t e = hipMemcpy(d, dd, 320 * 4, hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : -2;
}

// allow mlp_kernel's dynamic-LDS launch (ndp_create)
hipError_t mlp_prepare(void)
{
    return hipFuncSetAttribute((const void *)mlp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(FR_TOTAL * sizeof(float)));
}

int launch_mlp(ndp_handle *h, const Neigh &nb, const double *d_ego, float *d_f, hipStream_t s, size_t ego_pitch)
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

// tick_pre_kernel, one thread per vehicle
void launch_tick_pre(const TickPre &a, hipStream_t s)
{
    hipLaunchKernelGGL(tick_pre_kernel, dim3((a.cf.B + 63) / 64), dim3(64), 0, s, a);
}

}  // extern "C"
