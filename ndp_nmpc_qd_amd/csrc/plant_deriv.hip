// plant_deriv.hip -- the plant over a GIVEN input sequence, and its derivatives: ndp_plant_rollout_device (B vehicles over `ticks` ticks of
// inputs u and forces f in one launch, the state in registers from the first tick to the last), ndp_plant_rollout_vjp_device (reverse mode)
// and ndp_plant_rollout_jvp_device (forward mode).  One lane per vehicle (forward mode: per vehicle and direction), 64-lane workgroups:
// every lane runs one long serial fp64 chain, so what a small batch needs is to be spread over many CUs.  No LDS, no atomics, no
// workspace, no scratch.  plant_seq_check, the ticks / substeps refusals, is shared with closed_loop.hip (host.hpp).
//
// What is differentiated is the arithmetic of a tick as plant_tick (plant_dyn.hpp) performs it: acc = f / mass - g held over the tick, the
// RK4 substeps with u and acc held, then q / |q| applied ONCE to the un-normalised end state.  The primal values every kernel here writes
// or restarts from are plant_tick's, bit for bit; the stage states a derivative is taken AT (rk4_stages) are recomputed with plain
// expressions and may differ from them in the last place, which moves a derivative by rounding only.
#include <hip/hip_runtime.h>

#include "../../include/ndp_nmpc.h"
#include "host.hpp"
#include "plant_dyn.hpp"
#include "plant_adj.hpp"
#include "plant_tan.hpp"

namespace ndp {

enum { PLANT_LANES = 64 };

struct PlantSeq {              // what the three kernels share: the sequence's shape and the model's two numbers
    int ticks, sub, B;
    double h, inv_mass, g;     // h: the substep, dt / substeps as ndp_plant_step_device forms it
};

// ---- reverse mode: rk4_stages, plant_f_vjp and plant_rk4_vjp are plant_adj.hpp's (closed_loop.hip's reverse link inlines them too)

// ---- forward mode: plant_f_jvp and plant_rk4_jvp are plant_tan.hpp's (closed_loop.hip's tangent link inlines them too)

// ------------------------------------------------------------------------------------------ kernels
// The forward: row k of xs = plant_kernel applied k + 1 times, bit for bit (plant_tick).  x0 may be any tick's slot of xs: a lane reads
// its own row of x0 before it writes anything and writes its own rows only (so neither is __restrict__).
__global__ __launch_bounds__(PLANT_LANES) void plant_rollout_kernel(PlantSeq p, const double *x0, const double *__restrict__ u,
                                                                    const double *__restrict__ f, double *xs)
{
    const int v = (int)(blockIdx.x * PLANT_LANES + threadIdx.x);
    if (v >= p.B) return;
    double xv[10], uv[4];
    plant_ld_row<5>(x0 + (size_t)v * 10, xv);
    for (int k = 0; k < p.ticks; ++k) {
        const size_t row = (size_t)k * p.B + v;
        plant_ld_row<2>(u + row * 4, uv);
        plant_tick(xv, uv, f, row * 3, p.h, p.sub, p.inv_mass, p.g);
        plant_st_row<5>(xs + row * 10, xv);
    }
}

// Reverse mode, tick by tick from the last: tick k restarts from the log (xs[k-1], x0 at k = 0), so the chain is never re-integrated
// from its start.  Within a tick the un-normalised end state and the substeps' start states are recomputed from the tick's input state
// -- substep s by s plant_rk4 steps, O(sub^2) cheap steps per tick instead of `sub` stored states: everything stays in registers.
//   lam: dL / d(the state after tick k) = gxs[k] + what tick k + 1 handed back; through q / |q|: lam_y = (lam_q - q <q, lam_q>) / |y_q|.
// gu, gf, gx0: each null = not wanted (the arithmetic is the same either way: an output does not depend on which others are asked for).
__global__ __launch_bounds__(PLANT_LANES) void plant_rollout_vjp_kernel(PlantSeq p, const double *__restrict__ x0, const double *__restrict__ u,
                                                                        const double *__restrict__ f, const double *__restrict__ xs,
                                                                        const double *__restrict__ gxs, double *__restrict__ gx0,
                                                                        double *__restrict__ gu, double *__restrict__ gf)
{
    const int v = (int)(blockIdx.x * PLANT_LANES + threadIdx.x);
    if (v >= p.B) return;
    double lam[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) lam[i] = 0.0;
    for (int k = p.ticks - 1; k >= 0; --k) {
        const size_t row = (size_t)k * p.B + v;
        double xin[10], y[10], uv[4], acc[3], gk[10], guv[4] = {0.0, 0.0, 0.0, 0.0}, gacc[3] = {0.0, 0.0, 0.0};
        plant_ld_row<5>(k ? xs + (row - p.B) * 10 : x0 + (size_t)v * 10, xin);
        plant_ld_row<2>(u + row * 4, uv);
        plant_ld_row<5>(gxs + row * 10, gk);
        plant_acc(f, row * 3, p.inv_mass, p.g, acc);
#pragma unroll
        for (int i = 0; i < 10; ++i) { lam[i] += gk[i]; y[i] = xin[i]; }
        for (int s = 0; s < p.sub; ++s) plant_rk4(y, uv, acc, p.h);
        const double n = plant_renorm(y);                    // y[6..9]: the tick's output quaternion
        const double d = y[6] * lam[6] + y[7] * lam[7] + y[8] * lam[8] + y[9] * lam[9];
#pragma unroll
        for (int i = 6; i < 10; ++i) lam[i] = (lam[i] - y[i] * d) / n;
        for (int s = p.sub - 1; s >= 0; --s) {
#pragma unroll
            for (int i = 0; i < 10; ++i) y[i] = xin[i];
            for (int j = 0; j < s; ++j) plant_rk4(y, uv, acc, p.h);
            plant_rk4_vjp(y, uv, acc, p.h, lam, guv, gacc);
        }
        if (gu) plant_st_row<2>(gu + row * 4, guv);
        if (gf) { gf[row * 3] = gacc[0] * p.inv_mass; gf[row * 3 + 1] = gacc[1] * p.inv_mass; gf[row * 3 + 2] = gacc[2] * p.inv_mass; }
    }
    if (gx0) plant_st_row<5>(gx0 + (size_t)v * 10, lam);
}

// Forward mode, one lane per (vehicle, direction): lane i = v T + t carries the vehicle's primal (plant_tick: the forward's bits, what
// xs_check receives from the t = 0 lane) and ONE tangent, so T directions in a call are T one-direction calls bit for bit -- a lane's
// arithmetic does not know T.  tx0 [B][T][10], tu [ticks][B][T][4], tf [ticks][B][T][3] (each null = 0), dxs [ticks][B][T][10]: all
// rows of lane i at (k B T + i).
__global__ __launch_bounds__(PLANT_LANES) void plant_rollout_jvp_kernel(PlantSeq p, int T, const double *__restrict__ x0,
                                                                        const double *__restrict__ u, const double *__restrict__ f,
                                                                        const double *__restrict__ tx0, const double *__restrict__ tu,
                                                                        const double *__restrict__ tf, double *__restrict__ dxs,
                                                                        double *__restrict__ xs_check)
{
    const size_t lanes = (size_t)p.B * T, i = (size_t)blockIdx.x * PLANT_LANES + threadIdx.x;
    if (i >= lanes) return;
    const size_t v = i / (size_t)T;
    const bool first = i - v * T == 0;
    double xv[10], dx[10];
    plant_ld_row<5>(x0 + v * 10, xv);
#pragma unroll
    for (int j = 0; j < 10; ++j) dx[j] = 0.0;
    if (tx0) plant_ld_row<5>(tx0 + i * 10, dx);
    for (int k = 0; k < p.ticks; ++k) {
        const size_t row = (size_t)k * p.B + v, lrow = (size_t)k * lanes + i;
        double y[10], uv[4], acc[3], du[4] = {0.0, 0.0, 0.0, 0.0}, dacc[3] = {0.0, 0.0, 0.0};
        plant_ld_row<2>(u + row * 4, uv);
        if (tu) plant_ld_row<2>(tu + lrow * 4, du);
        if (tf) { dacc[0] = tf[lrow * 3] * p.inv_mass; dacc[1] = tf[lrow * 3 + 1] * p.inv_mass; dacc[2] = tf[lrow * 3 + 2] * p.inv_mass; }
        plant_acc(f, row * 3, p.inv_mass, p.g, acc);
#pragma unroll
        for (int j = 0; j < 10; ++j) y[j] = xv[j];
        for (int s = 0; s < p.sub; ++s) {
            plant_rk4_jvp(y, uv, acc, p.h, dx, du, dacc);
            plant_rk4(y, uv, acc, p.h);
        }
        plant_tick(xv, uv, f, row * 3, p.h, p.sub, p.inv_mass, p.g);      // (y renormalised is xv: the same operations)
        const double n = sqrt(y[6] * y[6] + y[7] * y[7] + y[8] * y[8] + y[9] * y[9]);
        const double d = xv[6] * dx[6] + xv[7] * dx[7] + xv[8] * dx[8] + xv[9] * dx[9];
#pragma unroll
        for (int j = 6; j < 10; ++j) dx[j] = (dx[j] - xv[j] * d) / n;
        plant_st_row<5>(dxs + lrow * 10, dx);
        if (xs_check && first) plant_st_row<5>(xs_check + row * 10, xv);
    }
}

}  // namespace ndp

using namespace ndp;

static PlantSeq plant_seq(const ndp_handle *h, int ticks, double dt, int substeps)
{
    const PlantNum n = plant_num(h, dt, substeps);
    return PlantSeq{ticks, substeps, h->cfg.batch, n.h, n.inv_mass, n.g};
}

extern "C" {

// the refusals the three calls here and closed_loop.hip's three share, nothing enqueued: -2 with the reason in ndp_last_error
int plant_seq_check(ndp_handle *h, const char *who, int ticks, int substeps)
{
    if (ticks < 1) { h->err = std::string(who) + ": ticks must be >= 1, got " + std::to_string(ticks); return -2; }
    if (substeps < 1 || substeps > NDP_PLANT_MAX_SUBSTEPS) {
        h->err = std::string(who) + ": substeps must be 1..16 (NDP_PLANT_MAX_SUBSTEPS), got " + std::to_string(substeps);
        return -2;
    }
    return 0;
}

int ndp_plant_rollout_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_u, const void *d_f,
                             void *d_xs, void *stream)
{
    Entry g(h, d_x0 && d_u && d_xs, stream);
    if (g.rc) return g.rc;
    int rc = plant_seq_check(h, "ndp_plant_rollout_device", ticks, substeps);
    if (rc) return rc;
    const PlantSeq p = plant_seq(h, ticks, dt, substeps);
    hipLaunchKernelGGL(plant_rollout_kernel, dim3((p.B + PLANT_LANES - 1) / PLANT_LANES), dim3(PLANT_LANES), 0, g.s, p, (const double *)d_x0,
                       (const double *)d_u, (const double *)d_f, (double *)d_xs);
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

int ndp_plant_rollout_vjp_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_u, const void *d_f,
                                 const void *d_xs, const void *d_gxs, void *d_gx0, void *d_gu, void *d_gf, void *stream)
{
    Entry g(h, d_x0 && d_u && d_xs && d_gxs, stream);
    if (g.rc) return g.rc;
    int rc = plant_seq_check(h, "ndp_plant_rollout_vjp_device", ticks, substeps);
    if (rc) return rc;
    if (!d_gx0 && !d_gu && !d_gf) { h->err = "ndp_plant_rollout_vjp_device: no output asked for (d_gx0, d_gu and d_gf all NULL)"; return -2; }
    const PlantSeq p = plant_seq(h, ticks, dt, substeps);
    hipLaunchKernelGGL(plant_rollout_vjp_kernel, dim3((p.B + PLANT_LANES - 1) / PLANT_LANES), dim3(PLANT_LANES), 0, g.s, p,
                       (const double *)d_x0, (const double *)d_u, (const double *)d_f, (const double *)d_xs, (const double *)d_gxs,
                       (double *)d_gx0, (double *)d_gu, (double *)d_gf);
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

int ndp_plant_rollout_jvp_device(ndp_handle *h, int ticks, double dt, int substeps, const void *d_x0, const void *d_u, const void *d_f,
                                 int n_tan, const void *d_tx0, const void *d_tu, const void *d_tf, void *d_dxs, void *d_xs_check,
                                 void *stream)
{
    Entry g(h, d_x0 && d_u, stream);
    if (g.rc) return g.rc;
    int rc = plant_seq_check(h, "ndp_plant_rollout_jvp_device", ticks, substeps);
    if (rc) return rc;
    const char *why = nullptr;
    if (n_tan < 1 || n_tan > NDP_JVP_MAX_TANGENTS) why = "ndp_plant_rollout_jvp_device: n_tan must be 1..8 (directions per call)";
    else if (!d_tx0 && !d_tu && !d_tf) why = "ndp_plant_rollout_jvp_device: no tangent given (d_tx0, d_tu and d_tf all NULL)";
    else if (!d_dxs) why = "ndp_plant_rollout_jvp_device: d_dxs is required (the tangent of the log)";
    if (why) { h->err = why; return -2; }
    const PlantSeq p = plant_seq(h, ticks, dt, substeps);
    const size_t lanes = (size_t)p.B * n_tan;
    hipLaunchKernelGGL(plant_rollout_jvp_kernel, dim3((unsigned)((lanes + PLANT_LANES - 1) / PLANT_LANES)), dim3(PLANT_LANES), 0, g.s, p, n_tan,
                       (const double *)d_x0, (const double *)d_u, (const double *)d_f, (const double *)d_tx0, (const double *)d_tu,
                       (const double *)d_tf, (double *)d_dxs, (double *)d_xs_check);
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

}  // extern "C"
