// plant_adj.hpp -- the reverse mode of the plant's RK4 substep as device functions: what plant_rollout_vjp_kernel (plant_deriv.hip) and the
// closed loop's reverse link (closed_loop.hip) inline; rk4_stages also serves plant_deriv.hip's forward mode.
// Unlike plant_dyn.hpp's tick these are plain expressions with contraction left to the compiler: inlined into another kernel they may round
// differently in the last place, which moves a derivative by rounding only (the primal values every kernel writes or restarts from are
// plant_tick's, bit for bit).
#pragma once
#include <hip/hip_runtime.h>

#include "plant_dyn.hpp"

namespace ndp {

// the stage states X2, X3, X4 of the RK4 substep that starts at x (X1 = x)
__device__ __forceinline__ void rk4_stages(const double *x, const double *u, const double *acc, double h, double *X2, double *X3, double *X4)
{
    double k[10];
    plant_f(x, u, acc, k);
#pragma unroll
    for (int i = 0; i < 10; ++i) X2[i] = x[i] + 0.5 * h * k[i];
    plant_f(X2, u, acc, k);
#pragma unroll
    for (int i = 0; i < 10; ++i) X3[i] = x[i] + 0.5 * h * k[i];
    plant_f(X3, u, acc, k);
#pragma unroll
    for (int i = 0; i < 10; ++i) X4[i] = x[i] + h * k[i];
}

// gx = (d plant_f / dx)' gd (written); gu += (d plant_f / du)' gd; gacc += (d plant_f / dacc)' gd
__device__ __forceinline__ void plant_f_vjp(const double *x, const double *u, const double *gd, double *gx, double *gu, double *gacc)
{
    const double qw = x[6], qx = x[7], qy = x[8], qz = x[9];
    const double t3 = 2.0 * u[3] * gd[3], t4 = 2.0 * u[3] * gd[4], t5 = 4.0 * u[3] * gd[5];
    gx[0] = 0.0; gx[1] = 0.0; gx[2] = 0.0;
    gx[3] = gd[0]; gx[4] = gd[1]; gx[5] = gd[2];
    gx[6] = t3 * qy - t4 * qx + 0.5 * (u[0] * gd[7] + u[1] * gd[8] + u[2] * gd[9]);
    gx[7] = t3 * qz - t4 * qw - t5 * qx + 0.5 * (-u[0] * gd[6] - u[2] * gd[8] + u[1] * gd[9]);
    gx[8] = t3 * qw + t4 * qz - t5 * qy + 0.5 * (-u[1] * gd[6] + u[2] * gd[7] - u[0] * gd[9]);
    gx[9] = t3 * qx + t4 * qy + 0.5 * (-u[2] * gd[6] - u[1] * gd[7] + u[0] * gd[8]);
    gu[0] += 0.5 * (-qx * gd[6] + qw * gd[7] + qz * gd[8] - qy * gd[9]);
    gu[1] += 0.5 * (-qy * gd[6] - qz * gd[7] + qw * gd[8] + qx * gd[9]);
    gu[2] += 0.5 * (-qz * gd[6] + qy * gd[7] - qx * gd[8] + qw * gd[9]);
    gu[3] += 2.0 * (qx * qz + qw * qy) * gd[3] + 2.0 * (qy * qz - qw * qx) * gd[4] + (1.0 - 2.0 * qx * qx - 2.0 * qy * qy) * gd[5];
    gacc[0] += gd[3]; gacc[1] += gd[4]; gacc[2] += gd[5];
}

// the adjoint of one RK4 substep that started at x: lam (of the substep's end state) becomes that of x; gu, gacc accumulate
__device__ __forceinline__ void plant_rk4_vjp(const double *x, const double *u, const double *acc, double h, double *lam, double *gu,
                                              double *gacc)
{
    double X2[10], X3[10], X4[10], gk[10], gX[10], out[10];
    rk4_stages(x, u, acc, h, X2, X3, X4);
#pragma unroll
    for (int i = 0; i < 10; ++i) gk[i] = h / 6.0 * lam[i];
    plant_f_vjp(X4, u, gk, gX, gu, gacc);
#pragma unroll
    for (int i = 0; i < 10; ++i) { out[i] = lam[i] + gX[i]; gk[i] = h / 3.0 * lam[i] + h * gX[i]; }
    plant_f_vjp(X3, u, gk, gX, gu, gacc);
#pragma unroll
    for (int i = 0; i < 10; ++i) { out[i] += gX[i]; gk[i] = h / 3.0 * lam[i] + 0.5 * h * gX[i]; }
    plant_f_vjp(X2, u, gk, gX, gu, gacc);
#pragma unroll
    for (int i = 0; i < 10; ++i) { out[i] += gX[i]; gk[i] = h / 6.0 * lam[i] + 0.5 * h * gX[i]; }
    plant_f_vjp(x, u, gk, gX, gu, gacc);
#pragma unroll
    for (int i = 0; i < 10; ++i) lam[i] = out[i] + gX[i];
}

}  // namespace ndp
