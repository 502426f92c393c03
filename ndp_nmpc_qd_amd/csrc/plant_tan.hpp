// plant_tan.hpp -- the forward mode of the plant's RK4 substep as device functions: what plant_rollout_jvp_kernel (plant_deriv.hip) and the
// closed loop's tangent link (closed_loop.hip) inline.  The stage states a tangent is taken AT are plant_adj.hpp's rk4_stages.
// Like plant_adj.hpp's these are plain expressions with contraction left to the compiler: inlined into another kernel they may round
// differently in the last place, which moves a derivative by rounding only (the primal values every kernel writes or restarts from are
// plant_tick's, bit for bit).
#pragma once
#include <hip/hip_runtime.h>

#include "plant_adj.hpp"

namespace ndp {

// dd = (d plant_f / dx) dx + (d plant_f / du) du + dacc
__device__ __forceinline__ void plant_f_jvp(const double *x, const double *u, const double *dx, const double *du, const double *dacc,
                                            double *dd)
{
    const double qw = x[6], qx = x[7], qy = x[8], qz = x[9], pw = dx[6], px = dx[7], py = dx[8], pz = dx[9];
    dd[0] = dx[3]; dd[1] = dx[4]; dd[2] = dx[5];
    dd[3] = 2.0 * ((px * qz + qx * pz + pw * qy + qw * py) * u[3] + (qx * qz + qw * qy) * du[3]) + dacc[0];
    dd[4] = 2.0 * ((py * qz + qy * pz - pw * qx - qw * px) * u[3] + (qy * qz - qw * qx) * du[3]) + dacc[1];
    dd[5] = -4.0 * (qx * px + qy * py) * u[3] + (1.0 - 2.0 * qx * qx - 2.0 * qy * qy) * du[3] + dacc[2];
    dd[6] = (-du[0] * qx - u[0] * px - du[1] * qy - u[1] * py - du[2] * qz - u[2] * pz) * 0.5;
    dd[7] = (du[0] * qw + u[0] * pw + du[2] * qy + u[2] * py - du[1] * qz - u[1] * pz) * 0.5;
    dd[8] = (du[1] * qw + u[1] * pw - du[2] * qx - u[2] * px + du[0] * qz + u[0] * pz) * 0.5;
    dd[9] = (du[2] * qw + u[2] * pw + du[1] * qx + u[1] * px - du[0] * qy - u[0] * py) * 0.5;
}

// the tangent of one RK4 substep that starts at x: dx becomes the end state's
__device__ __forceinline__ void plant_rk4_jvp(const double *x, const double *u, const double *acc, double h, double *dx, const double *du,
                                              const double *dacc)
{
    double X2[10], X3[10], X4[10], dk[10], dX[10], sum[10];
    rk4_stages(x, u, acc, h, X2, X3, X4);
    plant_f_jvp(x, u, dx, du, dacc, dk);
#pragma unroll
    for (int i = 0; i < 10; ++i) { sum[i] = dk[i]; dX[i] = dx[i] + 0.5 * h * dk[i]; }
    plant_f_jvp(X2, u, dX, du, dacc, dk);
#pragma unroll
    for (int i = 0; i < 10; ++i) { sum[i] += 2.0 * dk[i]; dX[i] = dx[i] + 0.5 * h * dk[i]; }
    plant_f_jvp(X3, u, dX, du, dacc, dk);
#pragma unroll
    for (int i = 0; i < 10; ++i) { sum[i] += 2.0 * dk[i]; dX[i] = dx[i] + h * dk[i]; }
    plant_f_jvp(X4, u, dX, du, dacc, dk);
#pragma unroll
    for (int i = 0; i < 10; ++i) dx[i] += h / 6.0 * (sum[i] + dk[i]);
}

}  // namespace ndp
