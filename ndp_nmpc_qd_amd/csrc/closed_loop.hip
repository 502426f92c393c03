// closed_loop.hip -- the closed loop over GIVEN reference windows and forces (the "ext" form), recorded, and its two derivative modes, each as
// one call: ndp_closed_loop_device (control step -> plant tick -> the next tick's x0, `ticks` times, everything enqueued on one stream),
// ndp_closed_loop_vjp_device (the gradient of a loss on that flight in x_0, the windows, the forces and the controller's own numbers) and
// ndp_closed_loop_jvp_device (the tangents of that flight along directions of x_0, the windows and the forces).
// And the FORMATION's form of the first two, with the force on the plant made inside the loop from the vehicles' actual states:
// ndp_closed_loop_formation_config (the index and its reverse lists, built on the host), ndp_closed_loop_formation_device (the existing
// force launch in front of each step; no new kernel), ndp_closed_loop_formation_vjp_device and ndp_plant_force_scatter_device:
//   closed_loop_formation_rev_link_kernel  closed_loop_rev_link_kernel's lane body (closed_loop_rev_lane.inc, shared as text) with two
//                                hooks: gx_f -- the gather of tick k + 1's g_z over the vehicle's list and its own slots (cl_gather) --
//                                into lambda, and gF_k = gfps[k] + gfp_k out to the force's adjoint (plant_force_vjp_kernel, unchanged),
//                                which runs between the link and the step's adjoint; spare workgroups add tick k + 1's fp32 g_w into an
//                                fp64 accumulator, the tail launch rounds it once
//   closed_loop_scatter_kernel   cl_gather alone: g_z per slot onto the states, one lane per vehicle, no atomics
//
// The control step and its derivatives are the existing kernels, launched unchanged (enqueue_step; recompute_on_workspace with rti_vjp_kernel
// / rti_wvjp_kernel / rti_jvp_kernel).  What is new is everything BETWEEN two of them, one launch per tick and direction:
//   closed_loop_fwd_link_kernel  behind step k: the plant tick (plant_tick: ndp_plant_step_device's bits) from x_k and u0_k into xs[k], the
//                                status words into their log, and the engine's post-step iterate and kept set copied into tape slot k + 1
//                                (and X into Xs[k]) in 16-byte pieces
//   closed_loop_rev_link_kernel  in front of the adjoint of tick k: lambda = gxs_k + (gx_p + gx0) of tick k + 1, the plant tick's adjoint
//                                (the arithmetic of plant_rollout_vjp_kernel's tick body), gu0 = gus_k + gu_p for the step's adjoint,
//                                gfp[k], tick k + 1's model-gradient row folded into the total, and tape slot k copied into the adjoint's
//                                workspace; a tail launch behind tick 0 forms gx0 = gx_p + gx0 and the last fold.  Each launch also sees
//                                the status words tick k + 1's adjoint recomputed: where nonzero, gfp[k + 1] and the plant's mass share
//                                become NaN (ClRev::st_prev)
//   closed_loop_tan_link_kernel  behind the forward mode of step k: the plant tick's tangent (the arithmetic of plant_rollout_jvp_kernel's
//                                tick body) at (x_k, u0_k, fp_k) along (dxs[k-1], dus[k], tfp[k]) into dxs[k], one lane per (vehicle,
//                                direction), and tape slot k + 1 copied into the forward mode's workspace; a head launch copies slot 0.
//                                The launch sees tick k's recomputed status words: where nonzero, or where the incoming tangent is NaN
//                                (an earlier tick failed), dxs[k] and dus[k] become NaN (a pinned row of the step's du0 would stay 0)
// One lane per vehicle in 64-lane workgroups for the plant (plant_deriv.hip's shape: a long serial fp64 chain per lane, spread over many
// CUs); the copies run on further workgroups of the same launch, grid-stride.  No LDS, no atomics, no scratch.
// Host side: ClView (tick k's slices, its tape slot, a link's two copies), cl_check (the refusals of all three calls, around plant_deriv.hip's
// plant_seq_check), cl_deriv_begin (what the derivative calls share before they enqueue); one body per direction for the ext form and the
// formation's (cl_forward, cl_reverse: a ClFormation or null), the forward mode's launch loop in its entry; each reads top to bottom.
#include <hip/hip_runtime.h>

#include "../../include/ndp_nmpc.h"
#include "host.hpp"
#include "plant_dyn.hpp"
#include "plant_adj.hpp"
#include "plant_tan.hpp"
#include "mlp_common.hpp"

namespace ndp {

enum { CL_LANES = 64, CL_MAX_COPY_BLOCKS = 2048 };

struct ClCopy {                // one contiguous run, moved in 16-byte pieces (both ends 16-byte aligned), its tail byte by byte; dst null: none
    const unsigned char *src;
    unsigned char *dst;
    size_t bytes;
};

struct ClPlant {               // the plant's shape and the model's two numbers (plant_deriv.hip: PlantSeq)
    int B, sub, plant_blocks;  // plant_blocks: the launch's first workgroups, one lane per vehicle; the rest copy
    double h, inv_mass, g;
};

struct ClFwd {
    ClPlant p;
    const double *xin, *u, *fp;     // x_k [B][10], u0_k [B][4], fp_k [B][3] or null
    double *xout;                   // xs[k]
    const int *st_src;              // the step's status words ...
    int *st_dst;                    // ... into d_status[k], or null
    ClCopy cp[3];                   // iterate -> tape slot, kept set -> tape slot, X -> Xs[k]
};

struct ClRev {
    ClPlant p;                      // plant_blocks workgroups, one lane per vehicle, in the tail launch too
    int tail;                       // 1: the launch behind tick 0 (no plant: gx0 and the last fold)
    const double *xin, *u, *fp;     // x_k, u0_k, fp_k (null: none)
    const double *gxs, *gus;        // the upstreams of x_{k+1} and u0_k, or null
    const double *c_p, *c_s;        // what tick k + 1 handed back: its plant's gx_p and its step's gx0 (null at the last tick)
    double *gxp, *gu0;              // out: gx_p, and gu0 = gus_k + gu_p for the step's adjoint
    double *gfp;                    // out: gfp[k], or null
    double *gm_tot;                 // [B][16] the model gradient's total, or null
    const double *gm_row;           // [B][16] tick k + 1's row (the step's rti_wvjp_kernel), null at the last tick
    double *gx0;                    // tail: d_gx0, or null
    const int *st_prev;             // tick k + 1's recomputed status words (its adjoint has run), null at the last tick: where nonzero,
    double *gfp_prev;               // gfp[k + 1] (or null) and the plant's mass share become NaN -- the plant's adjoint alone would not
                                    // make them so at the vehicle's LAST failed tick (the force's gradient does not read the state)
    ClCopy cp[2];                   // tape slot k -> the adjoint's workspace: iterate, kept set
};

// The formation's reverse lists (ndp_closed_loop_formation_config): vehicle v is heard through the edges edge[offset[v] .. offset[v+1]),
// e = w K + j with index[w][j] == v, ascending; empty (o < 0 or o >= B) and self (o == w) slots are in no list
struct ClGather {
    const int *index, *offset, *edge;   // [B][K], [B+1], [offset[B]]
    const double *gz;                   // [B][K][6] the force adjoint's gradient per slot, or null: nothing to gather
    int B, K;
};

struct ClForm {                     // the formation: what the force's adjoint hands over, and what it is handed
    ClGather g;                     // tick k + 1's g_z (the force adjoint has run)
    const double *gfps;             // [B][3] the upstream of fps[k], or null
    double *gF;                     // out [B][3]: gfps[k] + gfp_k, the upstream of tick k's force adjoint
    const double *x;                // x_k [B][10], and the gate as the force took it: a vehicle that hears a non-finite state through an
    int gate;                       // open slot gets gF = NaN (ClForm::force)
    double r2;
    __device__ __forceinline__ void incoming(int v, double *lam) const;
    __device__ __forceinline__ void force(int v, double g0, double g1, double g2) const;
};

struct ClAcc {                      // the weight gradient over the ticks, last tick first: acc = gw (first) or acc + gw, in fp64
    const float *gw;                // [NDP_MLP_NPARAM] tick k + 1's, or null: none
    double *acc;
    float *out;                     // the tail: the sum rounded once, or null
    int first;
};

struct ClRevF {
    ClRev r;
    ClForm f;
    ClAcc acc;
};

struct ClScatter {
    ClGather g;
    double *gx;                     // out [B][10]
};

struct ClTan {
    ClPlant p;                      // plant_blocks workgroups, one lane per (vehicle, direction): lane i = v T + t (B: the vehicles)
    int T;
    const double *xin, *u, *fp;     // x_k [B][10], u0_k [B][4], fp_k [B][3] or null
    const double *tx, *tfp;         // the tangent of x_k [B][T][10] (d_tx0, then dxs[k-1]; null: 0) and of fp_k [B][T][3] (null: 0)
    const double *tm;               // the model direction [B][T][16] or null: column 15, the plant's mass, moves the force as -(m' / m) fp_k
    double *du;                     // dus[k] [B][T][4]: the step's du0 as rti_jvp_kernel left it, read; NaN written where the tick failed
    double *dx;                     // out: dxs[k] [B][T][10]
    const int *st;                  // tick k's recomputed status words (its forward mode has run)
    ClCopy cp[2];                   // tape slot k + 1 -> the forward mode's workspace: iterate, kept set
};

__device__ __forceinline__ void cl_copy(const ClCopy &c, size_t i0, size_t stride)
{
    if (!c.dst) return;
    const size_t pieces = c.bytes >> 4, tail = c.bytes & 15;
    const uint4 *s = reinterpret_cast<const uint4 *>(c.src);
    uint4 *d = reinterpret_cast<uint4 *>(c.dst);
    for (size_t i = i0; i < pieces; i += stride) d[i] = s[i];
    if (i0 < tail) c.dst[(pieces << 4) + i0] = c.src[(pieces << 4) + i0];
}

__global__ __launch_bounds__(CL_LANES) void closed_loop_fwd_link_kernel(ClFwd a)
{
    if ((int)blockIdx.x >= a.p.plant_blocks) {
        const size_t i0 = (size_t)((int)blockIdx.x - a.p.plant_blocks) * CL_LANES + threadIdx.x;
        const size_t stride = (size_t)((int)gridDim.x - a.p.plant_blocks) * CL_LANES;
#pragma unroll
        for (int j = 0; j < 3; ++j) cl_copy(a.cp[j], i0, stride);
        return;
    }
    const int v = (int)(blockIdx.x * CL_LANES + threadIdx.x);
    if (v >= a.p.B) return;
    double xv[10], uv[4];
    plant_ld_row<5>(a.xin + (size_t)v * 10, xv);
    plant_ld_row<2>(a.u + (size_t)v * 4, uv);
    plant_tick(xv, uv, a.fp, (size_t)v * 3, a.p.h, a.p.sub, a.p.inv_mass, a.p.g);
    plant_st_row<5>(a.xout + (size_t)v * 10, xv);
    if (a.st_dst) a.st_dst[v] = a.st_src[v];
}

// The additions, in this order (include/ndp_nmpc.h states it): lambda = gxs_k + (gx_p + gx0), both of tick k + 1; gu0 = gus_k + gu_p;
// the model gradient last tick first: total = row_{K-1}, then + row_{K-2}, ... (columns 0..14), column 15 = p_{K-1} + p_{K-2} + ... with
// p_k = -(1/m) <gfp_k, fp_k>; d_gx0 = gx_p + gx0 of tick 0.  A null upstream adds nothing (the other operand as it is).
__global__ __launch_bounds__(CL_LANES) void closed_loop_rev_link_kernel(ClRev a)
{
    if ((int)blockIdx.x >= a.p.plant_blocks) {
        const size_t i0 = (size_t)((int)blockIdx.x - a.p.plant_blocks) * CL_LANES + threadIdx.x;
        const size_t stride = (size_t)((int)gridDim.x - a.p.plant_blocks) * CL_LANES;
#pragma unroll
        for (int j = 0; j < 2; ++j) cl_copy(a.cp[j], i0, stride);
        return;
    }
    const int v = (int)(blockIdx.x * CL_LANES + threadIdx.x);
    if (v >= a.p.B) return;
#define CL_REV_INCOMING(v, lam)
#define CL_REV_FORCE(v, g0, g1, g2)
#include "closed_loop_rev_lane.inc"
#undef CL_REV_INCOMING
#undef CL_REV_FORCE
}

// gx_f of vehicle v, the first six columns: (the sum over v's list, in list order, of gz[e]) - (the sum in slot order of v's own slots
// that are neither empty nor self).  Each sum starts from its first term as it is (an empty one is +0), then one subtraction.  A gather:
// every lane reads, none writes another's row.  False: v hears nobody and nobody hears v (out is +0).
__device__ __forceinline__ bool cl_gather(const ClGather &c, int v, double *out)
{
    double in[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, own[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool any_in = false, any_own = false;
    const int e1 = c.offset[v + 1];
    for (int q = c.offset[v]; q < e1; ++q) {
        const double *g = c.gz + (size_t)c.edge[q] * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) in[i] = any_in ? in[i] + g[i] : g[i];
        any_in = true;
    }
    for (int j = 0; j < c.K; ++j) {
        const int o = c.index[(size_t)v * c.K + j];
        if (o < 0 || o >= c.B || o == v) continue;
        const double *g = c.gz + ((size_t)v * c.K + j) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) own[i] = any_own ? own[i] + g[i] : g[i];
        any_own = true;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = in[i] - own[i];
    return any_in || any_own;
}

// lambda's share through the neighbours: (gx_p + gx0) + gx_f.  A vehicle outside every list and with no slot of its own adds nothing
// (its lambda is the "ext" form's, bit for bit)
__device__ __forceinline__ void ClForm::incoming(int v, double *lam) const
{
    if (!g.gz) return;
    double gxf[6];
    if (!cl_gather(g, v, gxf)) return;
#pragma unroll
    for (int i = 0; i < 6; ++i) lam[i] = lam[i] + gxf[i];
}

__device__ __forceinline__ void ClForm::force(int v, double g0, double g1, double g2) const
{
    if (gfps) { g0 = gfps[(size_t)v * 3] + g0; g1 = gfps[(size_t)v * 3 + 1] + g1; g2 = gfps[(size_t)v * 3 + 2] + g2; }
    // A vehicle that hears a non-finite relative state through an open slot flew under a meaningless force (the network's ReLU swallows
    // a NaN, so fps[k] may well be finite): its gF is NaN -- the force's adjoint then leaves the vehicle out of g_w and gives NaN in the
    // g_z of its open slots, as for any non-finite upstream
    const double *xe = x + (size_t)v * 10;
    bool lost = false;
    for (int j = 0; j < g.K; ++j) {
        const int o = g.index[(size_t)v * g.K + j];
        if (o < 0 || o >= g.B || o == v) continue;
        const double *xo = x + (size_t)o * 10;
        if (gate && !gate_open(xo, xe, r2)) continue;
#pragma unroll
        for (int i = 0; i < 6; ++i) lost = lost || !__builtin_isfinite(xo[i] - xe[i]);
    }
    if (lost) g0 = g1 = g2 = __builtin_nan("");
    gF[(size_t)v * 3] = g0; gF[(size_t)v * 3 + 1] = g1; gF[(size_t)v * 3 + 2] = g2;
}

__device__ __forceinline__ void cl_accumulate(const ClAcc &c, size_t i0, size_t stride)
{
    if (!c.gw) return;
    for (size_t i = i0; i < (size_t)NDP_MLP_NPARAM; i += stride) {
        const double t = c.first ? (double)c.gw[i] : c.acc[i] + (double)c.gw[i];
        if (c.out) c.out[i] = (float)t;
        else c.acc[i] = t;
    }
}

// closed_loop_rev_link_kernel with the vehicles coupled through the plant force: the same lane body (closed_loop_rev_lane.inc), ClForm's
// two hooks in it; the spare
// workgroups also add tick k + 1's weight gradient into the fp64 accumulator (the tail: and round it)
__global__ __launch_bounds__(CL_LANES) void closed_loop_formation_rev_link_kernel(ClRevF A)
{
    if ((int)blockIdx.x >= A.r.p.plant_blocks) {
        const size_t i0 = (size_t)((int)blockIdx.x - A.r.p.plant_blocks) * CL_LANES + threadIdx.x;
        const size_t stride = (size_t)((int)gridDim.x - A.r.p.plant_blocks) * CL_LANES;
#pragma unroll
        for (int j = 0; j < 2; ++j) cl_copy(A.r.cp[j], i0, stride);
        cl_accumulate(A.acc, i0, stride);
        return;
    }
    const int v = (int)(blockIdx.x * CL_LANES + threadIdx.x);
    if (v >= A.r.p.B) return;
    const ClRev &a = A.r;
#define CL_REV_INCOMING(v, lam) A.f.incoming(v, lam);
#define CL_REV_FORCE(v, g0, g1, g2) A.f.force(v, g0, g1, g2);
#include "closed_loop_rev_lane.inc"
#undef CL_REV_INCOMING
#undef CL_REV_FORCE
}

// ndp_plant_force_scatter_device: g_z per slot onto the states, as a gather
__global__ __launch_bounds__(CL_LANES) void closed_loop_scatter_kernel(ClScatter a)
{
    const int v = (int)(blockIdx.x * CL_LANES + threadIdx.x);
    if (v >= a.g.B) return;
    double o[10];
    cl_gather(a.g, v, o);
    o[6] = o[7] = o[8] = o[9] = 0.0;
    plant_st_row<5>(a.gx + (size_t)v * 10, o);
}

// The plant tick's tangent, plant_rollout_jvp_kernel's tick body: a lane carries the vehicle's primal (recomputed from x_k) and ONE tangent,
// so its arithmetic does not know T.  failed: the tick's status word is nonzero, or the incoming tangent holds a NaN (an earlier tick of
// this vehicle failed) -- then the lane's rows of dxs[k] and dus[k] are NaN, whatever the step's forward mode left in a pinned row.
__global__ __launch_bounds__(CL_LANES) void closed_loop_tan_link_kernel(ClTan a)
{
    if ((int)blockIdx.x >= a.p.plant_blocks) {
        const size_t i0 = (size_t)((int)blockIdx.x - a.p.plant_blocks) * CL_LANES + threadIdx.x;
        const size_t stride = (size_t)((int)gridDim.x - a.p.plant_blocks) * CL_LANES;
#pragma unroll
        for (int j = 0; j < 2; ++j) cl_copy(a.cp[j], i0, stride);
        return;
    }
    const size_t lanes = (size_t)a.p.B * a.T, i = (size_t)blockIdx.x * CL_LANES + threadIdx.x;
    if (i >= lanes) return;
    const size_t v = i / (size_t)a.T;
    double xv[10], y[10], dx[10], uv[4], du[4], acc[3], dacc[3] = {0.0, 0.0, 0.0};
    plant_ld_row<5>(a.xin + v * 10, xv);
    plant_ld_row<2>(a.u + v * 4, uv);
    plant_ld_row<2>(a.du + i * 4, du);
#pragma unroll
    for (int j = 0; j < 10; ++j) dx[j] = 0.0;
    if (a.tx) plant_ld_row<5>(a.tx + i * 10, dx);
    bool failed = a.st[v] != 0;
#pragma unroll
    for (int j = 0; j < 10; ++j) failed = failed || dx[j] != dx[j];
    if (a.tfp) { dacc[0] = a.tfp[i * 3] * a.p.inv_mass; dacc[1] = a.tfp[i * 3 + 1] * a.p.inv_mass; dacc[2] = a.tfp[i * 3 + 2] * a.p.inv_mass; }
    if (a.tm && a.fp) {            // the plant sees the mass only as fp / m (plant_acc): along tfp - (m' / m) fp_k
        const double c = a.tm[i * 16 + 15] * a.p.inv_mass;
#pragma unroll
        for (int j = 0; j < 3; ++j) dacc[j] = ((a.tfp ? a.tfp[i * 3 + j] : 0.0) - c * a.fp[v * 3 + j]) * a.p.inv_mass;
    }
    plant_acc(a.fp, v * 3, a.p.inv_mass, a.p.g, acc);
#pragma unroll
    for (int j = 0; j < 10; ++j) y[j] = xv[j];
    for (int s = 0; s < a.p.sub; ++s) {
        plant_rk4_jvp(y, uv, acc, a.p.h, dx, du, dacc);
        plant_rk4(y, uv, acc, a.p.h);
    }
    plant_tick(xv, uv, a.fp, v * 3, a.p.h, a.p.sub, a.p.inv_mass, a.p.g);      // (y renormalised is xv: the same operations)
    const double n = sqrt(y[6] * y[6] + y[7] * y[7] + y[8] * y[8] + y[9] * y[9]);
    const double d = xv[6] * dx[6] + xv[7] * dx[7] + xv[8] * dx[8] + xv[9] * dx[9];
#pragma unroll
    for (int j = 6; j < 10; ++j) dx[j] = (dx[j] - xv[j] * d) / n;
    if (failed) {
        const double nan = __builtin_nan("");
#pragma unroll
        for (int j = 0; j < 10; ++j) dx[j] = nan;
#pragma unroll
        for (int j = 0; j < 4; ++j) du[j] = nan;
        plant_st_row<2>(a.du + i * 4, du);
    }
    plant_st_row<5>(a.dx + i * 10, dx);
}

}  // namespace ndp

using namespace ndp;

// ---- the tape: per tick one slot = X_lin [B][N+1][10] fp64 | U_lin [B][N][4] fp64 | act_lin [B][4N] int8, padded to 256 bytes
static size_t cl_iterate_bytes(const ndp_handle *h) { return (nxs(h) + nus(h)) * 8; }
static size_t cl_slot_bytes(const ndp_handle *h) { return up256(cl_iterate_bytes(h) + act_bytes(h)); }

static ClPlant cl_plant(const ndp_handle *h, double dt, int substeps, bool plant)
{
    const int B = h->cfg.batch;
    const PlantNum n = plant_num(h, dt, substeps);
    return ClPlant{B, substeps, plant ? (B + CL_LANES - 1) / CL_LANES : 0, n.h, n.inv_mass, n.g};
}

static unsigned cl_copy_blocks(size_t bytes)
{
    const size_t per_block = (size_t)CL_LANES * 4 * 16;       // four pieces per lane before the grid-stride loop comes round
    const size_t n = (bytes + per_block - 1) / per_block;
    return (unsigned)(n < 1 ? 1 : n > CL_MAX_COPY_BLOCKS ? CL_MAX_COPY_BLOCKS : n);
}

template <class T> static T *cl_at(T *p, int k, size_t n) { return p ? p + (size_t)k * n : nullptr; }      // tick k of n per tick; null stays null

// A call's view of the flight, built once (host only): tick k's slices of the arrays all three entries take, and a link's two tape copies
struct ClView {
    const ndp_handle *h;
    const double *x0, *xr, *ur;
    const float *f;
    const double *fp, *xs, *us;
    unsigned char *tape;                     // (written by the forward only, where null means unrecorded)
    size_t B, slot, itb, ab;                 // vehicles; the bytes of a tape slot, of its iterate, of its kept set
    const double *x(int k) const { return k ? xs + (size_t)(k - 1) * B * NX : x0; }      // x_k: the call's x0, then the log's rows
    const double *u0(int k) const { return cl_at(us, k, B * NU); }
    const double *xrk(int k) const { return cl_at(xr, k, nxs(h)); }
    const double *urk(int k) const { return cl_at(ur, k, nus(h)); }
    const float *fk(int k) const { return cl_at(f, k, nfs(h)); }
    const double *fpk(int k) const { return cl_at(fp, k, B * 3); }
    // tick k's step as the recompute takes it (its tape is the workspace's copy), its status words to st (null: the workspace's)
    Tape step(int k, int *st) const { return Tape{x(k), xrk(k), urk(k), fk(k), nullptr, nullptr, nullptr, nullptr, st}; }
    void record(int k, ClCopy *cp) const     // the engine's pair into tape slot k (dU lies right behind dX)
    {
        cp[0] = ClCopy{(const unsigned char *)h->dX, tape + (size_t)k * slot, itb};
        cp[1] = ClCopy{(const unsigned char *)h->dAct.get(), tape + (size_t)k * slot + itb, ab};
    }
    void replay(int k, ClCopy *cp) const     // tape slot k into the workspace the derivative kernels recompute on
    {
        cp[0] = ClCopy{tape + (size_t)k * slot, (unsigned char *)h->dVjp.get(), itb};
        cp[1] = ClCopy{tape + (size_t)k * slot + itb, (unsigned char *)h->dVjpAct.get(), ab};
    }
};
static ClView cl_view(const ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f, const void *d_fp,
                      const void *d_xs, const void *d_us, const void *d_tape)
{
    return ClView{h, (const double *)d_x0, (const double *)d_xr, (const double *)d_ur, (const float *)d_f, (const double *)d_fp, (const double *)d_xs,
                  (const double *)d_us, (unsigned char *)d_tape, (size_t)h->cfg.batch, cl_slot_bytes(h), cl_iterate_bytes(h), act_bytes(h)};
}

// the refusals the three calls share, nothing enqueued: -2 with the reason in ndp_last_error
static int cl_check(ndp_handle *h, const char *who, int ticks, int substeps, const void *d_f)
{
    if (h->sens_level) return sens_refuse(h, who);
    int rc = plant_seq_check(h, who, ticks, substeps);
    if (rc) return rc;
    if (d_f && !h->cfg.use_fd) { h->err = std::string(who) + ": a disturbance force (d_f) needs use_fd = 1 (NDP model)"; return -2; }
    return 0;
}

// the formation calls' own two, behind cl_check: -2 not configured, -6 no weights (as the force call)
static int cl_form_check(ndp_handle *h, const char *who)
{
    if (!h->dFormIndex) { h->err = std::string(who) + ": no formation configured (ndp_closed_loop_formation_config)"; return -2; }
    if (!h->have_mlp) { h->err = std::string(who) + ": ndp_set_mlp_weights was never called"; return -6; }
    return 0;
}

static ClGather cl_gather_of(const ndp_handle *h, const double *gz)
{
    const int B = h->cfg.batch, K = h->form_K;
    return ClGather{h->dFormIndex, h->dFormIndex + (size_t)B * K, h->dFormIndex + (size_t)B * K + B + 1, gz, B, K};
}

// What the derivative calls do behind their frame and before they enqueue: cl_check, the recompute's refusals (noun: what it calls the
// derivative) around the entry's own -- a missing tape in front of `own`, the entry's others -- and the recompute's workspace.
static int cl_deriv_begin(ndp_handle *h, const char *who, const char *noun, int ticks, int substeps, const ClView &v, const char *own,
                          bool formation = false)
{
    int rc = cl_check(h, who, ticks, substeps, v.f);
    if (rc) return rc;
    if (formation && (rc = cl_form_check(h, who))) return rc;
    if (!v.tape) own = formation ? "d_tape is required (the forward's, recorded by ndp_closed_loop_formation_device)"
                                 : "d_tape is required (the forward's, recorded by ndp_closed_loop_device)";
    const void *lin = v.tape ? (const void *)v.tape : (const void *)v.x0;       // (a missing tape is refused by `own`, not as a missing iterate)
    const std::string why = recompute_refusal(h->cfg, noun, Tape{v.x0, v.xr, v.ur, v.f, lin, lin, nullptr, nullptr, nullptr}, own);
    if (!why.empty()) { h->err = std::string(who) + ": " + why; return -2; }
    return recompute_workspace(h);
}

// What the formation's calls add to the "ext" form's (null: the ext form): the gate and scale of the force on the plant, which the
// forward makes from the states into v.fp (its log d_fps); the reverse call's upstream on that log and its weight gradient
struct ClFormation {
    int gate;
    double scale;
    const void *d_gfps;
    void *d_gw;
};

// The forward of both forms, behind the entry's frame: the refusals, then everything enqueued on g.s
static int cl_forward(ndp_handle *h, Entry &g, const char *who, int ticks, double dt, int substeps, const ClView &v, void *d_xs, void *d_us,
                      void *d_Xs, void *d_status, const ClFormation *form)
{
    int rc = cl_check(h, who, ticks, substeps, v.f);
    if (rc) return rc;
    if (form && (rc = cl_form_check(h, who))) return rc;
    hipStream_t s = g.s;
    const size_t B = v.B;
    const unsigned cb = cl_copy_blocks(v.itb + v.ab + (d_Xs ? nxs(h) * 8 : 0));
    if (v.tape) {                  // slot 0: what the first step starts from
        ClFwd a{};
        a.p = cl_plant(h, dt, substeps, false);
        v.record(0, a.cp);
        hipLaunchKernelGGL(closed_loop_fwd_link_kernel, dim3(cb), dim3(CL_LANES), 0, s, a);
        NDP_HIP(h, hipGetLastError());
    }
    for (int k = 0; k < ticks; ++k) {
        double *u0 = cl_at((double *)d_us, k, B * NU);
        // the formation: the force from the states of this tick, before any of them moves (ndp_rollout_formation_multi_device's rule)
        if (form && (rc = launch_plant_force(h, v.x(k), h->dFormIndex, h->form_K, form->gate, form->scale, const_cast<double *>(v.fpk(k)),
                                             nullptr, s))) return rc;
        if ((rc = enqueue_step(h, v.x(k), v.xrk(k), v.urk(k), v.fk(k), Neigh{}, u0, nullptr, s))) return rc;
        ClFwd a{};
        a.p = cl_plant(h, dt, substeps, true);
        a.xin = v.x(k); a.u = u0; a.fp = v.fpk(k);
        a.xout = cl_at((double *)d_xs, k, B * NX);
        a.st_src = h->lastStatus; a.st_dst = cl_at((int *)d_status, k, B);
        if (v.tape && k + 1 < ticks) v.record(k + 1, a.cp);
        if (d_Xs) a.cp[2] = ClCopy{(const unsigned char *)h->dX, (unsigned char *)d_Xs + (size_t)k * nxs(h) * 8, nxs(h) * 8};
        hipLaunchKernelGGL(closed_loop_fwd_link_kernel, dim3((unsigned)a.p.plant_blocks + cb), dim3(CL_LANES), 0, s, a);
        NDP_HIP(h, hipGetLastError());
    }
    return g.noted(0);
}

// The reverse sweep of both forms, behind the entry's frame.  own: the entry's refusal (no upstream, no output) or null.  The ext form
// launches closed_loop_rev_link_kernel on the ClRev alone; the formation wraps the same ClRev into a ClRevF and runs the force's adjoint
// between the link and the step's adjoint.  d_gfp: the ext form's output (null in the formation, where the force is no leaf).
static int cl_reverse(ndp_handle *h, Entry &g, const char *who, int ticks, double dt, int substeps, const ClView &v, const char *own,
                      const void *d_gxs, const void *d_gus, const void *d_gXs, void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_gfp,
                      void *d_gmodel, void *d_status_check, const ClFormation *form)
{
    int rc = cl_deriv_begin(h, who, "adjoint", ticks, substeps, v, own, form != nullptr);
    if (rc) return rc;
    hipStream_t s = g.s;
    const size_t B = v.B;
    NDP_HIP(h, h->dClWs.ensure(B * (NU + NX + NX + 16) * 8));
    double *ws_gu0 = h->dClWs, *ws_gxp = ws_gu0 + B * NU, *ws_gx0 = ws_gxp + B * NX, *ws_gm = ws_gx0 + B * NX;
    double *ws_gF = nullptr, *ws_gz = nullptr, *ws_acc = nullptr;
    float *ws_gw = nullptr;
    if (form) {
        const size_t np2 = ((size_t)NDP_MLP_NPARAM + 1) / 2;       // a tick's fp32 g_w, in doubles
        NDP_HIP(h, h->dFormWs.ensure((B * 3 + B * NDP_MAX_NEIGH * 6 + NDP_MLP_NPARAM + np2) * 8));
        ws_gF = h->dFormWs; ws_gz = ws_gF + B * 3; ws_acc = ws_gz + B * NDP_MAX_NEIGH * 6;
        if (form->d_gw) ws_gw = (float *)(ws_acc + NDP_MLP_NPARAM);
    }
    const bool model = d_gmodel != nullptr;
    const unsigned cb = cl_copy_blocks(v.itb + v.ab);
    // where tick k's adjoint leaves its recomputed status words: the caller's log, or the workspace's
    auto st_of = [&](int k) { return d_status_check ? (const int *)d_status_check + (size_t)k * B : (const int *)h->dVjpSt; };
    // one link launch: the plain kernel, or the formation's around the same ClRev (gz: the g_z it gathers, null: none)
    auto link = [&](const ClRev &r, unsigned blocks, const double *gz, const double *gfps, const double *x, const ClAcc &acc) {
        if (!form) {
            hipLaunchKernelGGL(closed_loop_rev_link_kernel, dim3(blocks), dim3(CL_LANES), 0, s, r);
            return;
        }
        ClRevF a{};
        a.r = r;
        a.f.g = cl_gather_of(h, gz);
        a.f.gfps = gfps; a.f.gF = ws_gF;
        a.f.x = x; a.f.gate = form->gate ? 1 : 0; a.f.r2 = h->cfg.r_horiz * h->cfg.r_horiz;
        a.acc = acc;
        hipLaunchKernelGGL(closed_loop_formation_rev_link_kernel, dim3(blocks), dim3(CL_LANES), 0, s, a);
    };
    for (int k = ticks - 1; k >= 0; --k) {
        const bool last = k == ticks - 1;
        ClRev a{};
        a.p = cl_plant(h, dt, substeps, true);
        a.xin = v.x(k); a.u = v.u0(k); a.fp = v.fpk(k);
        a.gxs = cl_at((const double *)d_gxs, k, B * NX);
        a.gus = cl_at((const double *)d_gus, k, B * NU);
        a.c_p = last ? nullptr : ws_gxp; a.c_s = last ? nullptr : ws_gx0;
        a.gxp = ws_gxp; a.gu0 = ws_gu0;
        a.gfp = cl_at((double *)d_gfp, k, B * 3);
        a.gm_tot = (double *)d_gmodel; a.gm_row = last ? nullptr : ws_gm;
        a.st_prev = last ? nullptr : st_of(k + 1); a.gfp_prev = last ? nullptr : cl_at((double *)d_gfp, k + 1, B * 3);
        v.replay(k, a.cp);
        link(a, (unsigned)a.p.plant_blocks + cb, last ? nullptr : ws_gz, form ? cl_at((const double *)form->d_gfps, k, B * 3) : nullptr, v.x(k),
             ClAcc{last ? nullptr : ws_gw, ws_acc, nullptr, k == ticks - 2});
        NDP_HIP(h, hipGetLastError());
        // the formation: the force's adjoint at x_k on gF_k -- g_z per slot for the next link's gather, this tick's fp32 g_w
        if (form && (rc = launch_plant_force_vjp(h, who, v.x(k), h->dFormIndex, h->form_K, form->gate, form->scale, ws_gF, ws_gz, ws_gw, s)))
            return rc;
        VjpArgs va{ws_gu0, cl_at((const double *)d_gXs, k, nxs(h)), nullptr, ws_gx0, cl_at((double *)d_gxr, k, nxs(h)),
                   cl_at((double *)d_gur, k, nus(h)), cl_at((double *)d_gf, k, nfs(h))};
        double *gm = ws_gm;
        const Tape t = v.step(k, cl_at((int *)d_status_check, k, B));
        if (model) rc = recompute_on_workspace(h, s, t, recompute_kernel(RC_WVJP, true), recompute_kernel(RC_WVJP, false), &va, &gm);
        else rc = recompute_on_workspace(h, s, t, recompute_kernel(RC_VJP, true), recompute_kernel(RC_VJP, false), &va, nullptr);
        if (rc) return rc;
    }
    // behind tick 0: d_gx0 = gx_p + gx0 (the formation: + gx_f), tick 0's row into the model gradient, a failed tick 0's gfp, d_gw rounded once
    if (d_gx0 || d_gfp || ws_gw || model) {
        ClRev a{};
        a.p = cl_plant(h, dt, substeps, true);
        a.tail = 1;
        a.c_p = ws_gxp; a.c_s = ws_gx0;
        a.gx0 = (double *)d_gx0;
        a.gm_tot = (double *)d_gmodel; a.gm_row = ws_gm;
        a.st_prev = st_of(0); a.gfp_prev = (double *)d_gfp;
        const unsigned ab = ws_gw ? cl_copy_blocks((size_t)NDP_MLP_NPARAM * 8) : 0u;
        link(a, (unsigned)a.p.plant_blocks + ab, ws_gz, nullptr, nullptr, ClAcc{ws_gw, ws_acc, form ? (float *)form->d_gw : nullptr, ticks == 1});
        NDP_HIP(h, hipGetLastError());
    }
    return g.noted(0);
}

extern "C" {

int ndp_closed_loop_tape_bytes(ndp_handle *h, int ticks, size_t *bytes)
{
    if (!h || !bytes) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (ticks < 1) { h->err = "ndp_closed_loop_tape_bytes: ticks must be >= 1, got " + std::to_string(ticks); return -2; }
    *bytes = (size_t)ticks * cl_slot_bytes(h);
    return 0;
}

int ndp_closed_loop_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_xr, const void *d_ur,
                           const void *d_f, const void *d_fp, void *d_xs, void *d_us, void *d_Xs, void *d_status, void *d_tape, void *stream)
{
    Entry g(h, d_x0 && d_xr && d_ur && d_xs && d_us, stream);
    if (g.rc) return g.rc;
    return cl_forward(h, g, "ndp_closed_loop_device", ticks, dt, substeps, cl_view(h, d_x0, d_xr, d_ur, d_f, d_fp, d_xs, d_us, d_tape), d_xs, d_us,
                      d_Xs, d_status, nullptr);
}

int ndp_closed_loop_vjp_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_xr, const void *d_ur,
                               const void *d_f, const void *d_fp, const void *d_xs, const void *d_us, const void *d_tape, const void *d_gxs,
                               const void *d_gus, const void *d_gXs, void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_gfp,
                               void *d_gmodel, void *d_status_check, void *stream)
{
    Entry g(h, d_x0 && d_xr && d_ur && d_xs && d_us, stream);
    if (g.rc) return g.rc;
    const char *own = nullptr;
    if (!d_gxs && !d_gus && !d_gXs) own = "no upstream gradient (d_gxs, d_gus and d_gXs all NULL)";
    else if (!d_gx0 && !d_gxr && !d_gur && !d_gf && !d_gfp && !d_gmodel) own = "no output asked for (d_gx0, d_gxr, d_gur, d_gf, d_gfp and d_gmodel all NULL)";
    return cl_reverse(h, g, "ndp_closed_loop_vjp_device", ticks, dt, substeps, cl_view(h, d_x0, d_xr, d_ur, d_f, d_fp, d_xs, d_us, d_tape), own,
                      d_gxs, d_gus, d_gXs, d_gx0, d_gxr, d_gur, d_gf, d_gfp, d_gmodel, d_status_check, nullptr);
}

}  // extern "C"

// model: the entry is ndp_closed_loop_jvp_model_device (rti_mjvp_kernel per tick along the constant d_tmodel [B][T][16], required; its
// column 15 in the link), else ndp_closed_loop_jvp_device (rti_jvp_kernel)
static int cl_tangent(ndp_handle *h, Entry &g, const char *name, int ticks, double dt, int substeps, const ClView &v, int n_tan,
                      const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf, const void *d_tfp, bool model,
                      const void *d_tmodel, void *d_dxs, void *d_dus, void *d_dXs, void *d_dUs, void *d_status_check)
{
    const char *own = nullptr;
    if (n_tan < 1 || n_tan > NDP_JVP_MAX_TANGENTS) own = "n_tan must be 1..8 (directions per call)";
    else if (model && !d_tmodel) own = "d_tmodel is required (without it: ndp_closed_loop_jvp_device)";
    else if (!model && !d_tx0 && !d_txr && !d_tur && !d_tf && !d_tfp) own = "no tangent given (d_tx0, d_txr, d_tur, d_tf and d_tfp all NULL)";
    else if (d_tf && !h->cfg.use_fd) own = "a force tangent (d_tf) needs use_fd = 1 (NDP model)";
    else if (!d_dxs || !d_dus) own = "d_dxs and d_dus are required (the tangents of the two logs)";
    int rc = cl_deriv_begin(h, name, "derivative", ticks, substeps, v, own);
    if (rc) return rc;
    const RecomputeId kid = model ? RC_MJVP : RC_JVP;
    const double *tm = (const double *)d_tmodel;
    hipStream_t s = g.s;
    const size_t B = v.B, T = (size_t)n_tan;
    const unsigned cb = cl_copy_blocks(v.itb + v.ab), pb = (unsigned)((B * T + CL_LANES - 1) / CL_LANES);
    {                              // the head: slot 0 into the workspace
        ClTan a{};
        a.p = cl_plant(h, dt, substeps, false);
        v.replay(0, a.cp);
        hipLaunchKernelGGL(closed_loop_tan_link_kernel, dim3(cb), dim3(CL_LANES), 0, s, a);
        NDP_HIP(h, hipGetLastError());
    }
    double *dxs = (double *)d_dxs, *dus = (double *)d_dus;
    for (int k = 0; k < ticks; ++k) {
        const double *tx = k ? dxs + (size_t)(k - 1) * B * T * NX : (const double *)d_tx0;
        double *du = dus + (size_t)k * B * T * NU;
        int *st = cl_at((int *)d_status_check, k, B);
        // (tick 0 with no direction of the step's -- only d_tfp given -- is launched like every other: it recomputes the tick's status word,
        // and jvp_out with all four NULL writes the zeros, or the NaNs of a failed vehicle, that this tick's link reads)
        JvpArgs ja{tx, cl_at((const double *)d_txr, k, T * nxs(h)), cl_at((const double *)d_tur, k, T * nus(h)),
                   cl_at((const double *)d_tf, k, T * nfs(h)), du, cl_at((double *)d_dXs, k, T * nxs(h)), cl_at((double *)d_dUs, k, T * nus(h)),
                   n_tan};
        if ((rc = recompute_on_workspace(h, s, v.step(k, st), recompute_kernel(kid, true), recompute_kernel(kid, false), &ja, model ? &tm : nullptr)))
            return rc;
        ClTan a{};
        a.p = cl_plant(h, dt, substeps, true);
        a.p.plant_blocks = (int)pb;
        a.T = n_tan;
        a.xin = v.x(k); a.u = v.u0(k); a.fp = v.fpk(k);
        a.tx = tx; a.tfp = cl_at((const double *)d_tfp, k, B * T * 3);
        a.tm = tm;
        a.du = du; a.dx = dxs + (size_t)k * B * T * NX;
        a.st = st ? st : h->dVjpSt;
        const bool more = k + 1 < ticks;
        if (more) v.replay(k + 1, a.cp);
        hipLaunchKernelGGL(closed_loop_tan_link_kernel, dim3(pb + (more ? cb : 0u)), dim3(CL_LANES), 0, s, a);
        NDP_HIP(h, hipGetLastError());
    }
    return g.noted(0);
}

extern "C" {

int ndp_closed_loop_jvp_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_xr, const void *d_ur,
                               const void *d_f, const void *d_fp, const void *d_xs, const void *d_us, const void *d_tape, int n_tan,
                               const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf, const void *d_tfp, void *d_dxs,
                               void *d_dus, void *d_dXs, void *d_dUs, void *d_status_check, void *stream)
{
    Entry g(h, d_x0 && d_xr && d_ur && d_xs && d_us, stream);
    if (g.rc) return g.rc;
    return cl_tangent(h, g, "ndp_closed_loop_jvp_device", ticks, dt, substeps, cl_view(h, d_x0, d_xr, d_ur, d_f, d_fp, d_xs, d_us, d_tape), n_tan,
                      d_tx0, d_txr, d_tur, d_tf, d_tfp, false, nullptr, d_dxs, d_dus, d_dXs, d_dUs, d_status_check);
}

int ndp_closed_loop_jvp_model_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_xr, const void *d_ur,
                                     const void *d_f, const void *d_fp, const void *d_xs, const void *d_us, const void *d_tape, int n_tan,
                                     const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf, const void *d_tfp,
                                     const void *d_tmodel, void *d_dxs, void *d_dus, void *d_dXs, void *d_dUs, void *d_status_check,
                                     void *stream)
{
    Entry g(h, d_x0 && d_xr && d_ur && d_xs && d_us, stream);
    if (g.rc) return g.rc;
    return cl_tangent(h, g, "ndp_closed_loop_jvp_model_device", ticks, dt, substeps, cl_view(h, d_x0, d_xr, d_ur, d_f, d_fp, d_xs, d_us, d_tape),
                      n_tan, d_tx0, d_txr, d_tur, d_tf, d_tfp, true, d_tmodel, d_dxs, d_dus, d_dXs, d_dUs, d_status_check);
}

// ---- the formation: the plant force made from the states inside the loop, and the reverse sweep across the vehicles
int ndp_closed_loop_formation_config(ndp_handle *h, const int32_t *other_index, int K)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if (!other_index) {
        h->dFormIndex.reset();
        h->form_K = h->form_edges = 0;
        return 0;
    }
    if ((rc = check_neigh(h, "ndp_closed_loop_formation_config", K))) return rc;
    const int B = h->cfg.batch;
    const size_t slots = (size_t)B * K;
    auto heard = [&](size_t e) { const int o = other_index[e]; return o >= 0 && o < B && o != (int)(e / K) ? o : -1; };
    // index | offset | edge in one host block: a counting pass, then the edges in ascending e (each list comes out ascending)
    std::vector<int32_t> blk(slots + B + 1, 0);
    int32_t *off = blk.data() + slots;
    for (size_t e = 0; e < slots; ++e) {
        blk[e] = other_index[e];
        if (heard(e) >= 0) ++off[heard(e) + 1];
    }
    for (int v = 0; v < B; ++v) off[v + 1] += off[v];
    const int edges = off[B];
    blk.resize(slots + B + 1 + (size_t)edges);
    off = blk.data() + slots;
    std::vector<int32_t> fill(off, off + B);
    for (size_t e = 0; e < slots; ++e)
        if (heard(e) >= 0) blk[slots + B + 1 + (size_t)fill[heard(e)]++] = (int32_t)e;
    h->dFormIndex.reset();
    h->form_K = h->form_edges = 0;
    DevBuf<int> d_blk;                                 // (local until the copy is in: nothing stays configured behind a failed one)
    NDP_HIP(h, d_blk.alloc(blk.size() * 4));
    NDP_HIP(h, hipMemcpy(d_blk, blk.data(), blk.size() * 4, hipMemcpyHostToDevice));
    h->dFormIndex = std::move(d_blk); h->form_K = K; h->form_edges = edges;
    return 0;
}

int ndp_plant_force_scatter_device(ndp_handle *h, const void *d_gz, void *d_gx, void *stream)
{
    Entry g(h, d_gz && d_gx, stream);
    if (g.rc) return g.rc;
    if (!h->dFormIndex) { h->err = "ndp_plant_force_scatter_device: no formation configured (ndp_closed_loop_formation_config)"; return -2; }
    ClScatter a{cl_gather_of(h, (const double *)d_gz), (double *)d_gx};
    hipLaunchKernelGGL(closed_loop_scatter_kernel, dim3((unsigned)((a.g.B + CL_LANES - 1) / CL_LANES)), dim3(CL_LANES), 0, g.s, a);
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

int ndp_closed_loop_formation_device(ndp_handle *h, int ticks, double dt, int substeps, int gate, double plant_scale, const void *d_x0,
                                     const void *d_xr, const void *d_ur, const void *d_f, void *d_xs, void *d_us, void *d_fps, void *d_Xs,
                                     void *d_status, void *d_tape, void *stream)
{
    Entry g(h, d_x0 && d_xr && d_ur && d_xs && d_us && d_fps, stream);
    if (g.rc) return g.rc;
    const ClFormation form{gate, plant_scale, nullptr, nullptr};
    return cl_forward(h, g, "ndp_closed_loop_formation_device", ticks, dt, substeps, cl_view(h, d_x0, d_xr, d_ur, d_f, d_fps, d_xs, d_us, d_tape),
                      d_xs, d_us, d_Xs, d_status, &form);
}

int ndp_closed_loop_formation_vjp_device(ndp_handle *h, int ticks, double dt, int substeps, int gate, double plant_scale, const void *d_x0,
                                         const void *d_xr, const void *d_ur, const void *d_f, const void *d_xs, const void *d_us,
                                         const void *d_fps, const void *d_tape, const void *d_gxs, const void *d_gus, const void *d_gXs,
                                         const void *d_gfps, void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_gw, void *d_gmodel,
                                         void *d_status_check, void *stream)
{
    Entry g(h, d_x0 && d_xr && d_ur && d_xs && d_us && d_fps, stream);
    if (g.rc) return g.rc;
    const char *own = nullptr;
    if (!d_gxs && !d_gus && !d_gXs && !d_gfps) own = "no upstream gradient (d_gxs, d_gus, d_gXs and d_gfps all NULL)";
    else if (!d_gx0 && !d_gxr && !d_gur && !d_gf && !d_gw && !d_gmodel) own = "no output asked for (d_gx0, d_gxr, d_gur, d_gf, d_gw and d_gmodel all NULL)";
    const ClFormation form{gate, plant_scale, d_gfps, d_gw};
    return cl_reverse(h, g, "ndp_closed_loop_formation_vjp_device", ticks, dt, substeps,
                      cl_view(h, d_x0, d_xr, d_ur, d_f, d_fps, d_xs, d_us, d_tape), own, d_gxs, d_gus, d_gXs, d_gx0, d_gxr, d_gur, d_gf, nullptr,
                      d_gmodel, d_status_check, &form);
}

}  // extern "C"
