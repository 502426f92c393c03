// plant_dyn.hpp -- the rigid-body plant as device functions: what plant_kernel (rows.hip) and the kernels over an input sequence
// (plant_deriv.hip) inline.
// A tick's arithmetic -- force -> acceleration, the RK4 substeps with u and the force held, the quaternion renormalised once behind
// them -- is written out operation by operation (plant_tick and its parts: every product, sum and fused multiply-add is named, nothing is
// left to contract), so that it rounds the same way in every kernel it is inlined into, whatever surrounds it.  That is what makes a row of
// ndp_plant_rollout_device's log bit-equal to successive ndp_plant_step_device calls.  Written as the expressions of plant_f below with
// contraction left to the compiler, the same text came out rounded differently from one kernel to the next (which of a sum's two products
// is formed first and rounded, which is fused: it follows the order in which the surrounding code defines its values).  The operations
// are those the compiler chose for plant_kernel when that was the only user -- its results have not changed.
#pragma once
#include <hip/hip_runtime.h>

namespace ndp {

// the OCP's own dynamics (nmpc_body_rate_ctl.py:147-158 + f/mass) as plain expressions: for code that does not promise plant_kernel's
// bits (the stage states a derivative is taken at)
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

// ---- the tick, operation by operation
// the acceleration a tick holds: the vehicle's force row f[o .. o + 2] over the mass, minus gravity; f null (uniform): no force
__device__ __forceinline__ void plant_acc(const double *f, size_t o, double inv_mass, double g, double *acc)
{
#pragma clang fp contract(off)
    acc[0] = 0.0; acc[1] = 0.0; acc[2] = -g;
    if (f) { acc[0] = f[o] * inv_mass; acc[1] = f[o + 1] * inv_mass; acc[2] = __builtin_fma(inv_mass, f[o + 2], -g); }
}

// plant_f at the attitude q = (qw, qx, qy, qz): a[3] the acceleration (rows 3..5), r[4] TWICE the quaternion's rate (rows 6..9 before
// their factor 0.5)
__device__ __forceinline__ void plant_rates(const double *q, const double *u, const double *acc, double *a, double *r)
{
#pragma clang fp contract(off)
    const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    const double c0 = __builtin_fma(qw, qy, qx * qz), c1 = __builtin_fma(qy, qz, -(qw * qx));
    const double c2 = __builtin_fma(-qy, qy + qy, __builtin_fma(-qx, qx + qx, 1.0));
    a[0] = __builtin_fma(u[3], c0 + c0, acc[0]);
    a[1] = __builtin_fma(u[3], c1 + c1, acc[1]);
    a[2] = __builtin_fma(u[3], c2, acc[2]);
    r[0] = __builtin_fma(-u[2], qz, __builtin_fma(-u[0], qx, -(u[1] * qy)));
    r[1] = __builtin_fma(-u[1], qz, __builtin_fma(u[0], qw, u[2] * qy));
    r[2] = __builtin_fma(u[0], qz, __builtin_fma(u[1], qw, -(u[2] * qx)));
    r[3] = __builtin_fma(-u[0], qy, __builtin_fma(u[2], qw, u[1] * qx));
}

// one RK4 substep of length h, in place.  Stage i's slope: position rows v + c_i h a_(i-1) (never stored), velocity rows a_i, quaternion
// rows 0.5 r_i; the last stage's 0.5 is taken inside the weighted sum.
__device__ __forceinline__ void plant_rk4(double *xv, const double *uv, const double *acc, double h)
{
#pragma clang fp contract(off)
    const double hh = h * 0.5, h6 = h / 6.0;
    double a1[3], a2[3], a3[3], a4[3], r[4], k1[4], k2[4], k3[4], q[4];
    plant_rates(xv + 6, uv, acc, a1, r);
#pragma unroll
    for (int i = 0; i < 4; ++i) { k1[i] = r[i] * 0.5; q[i] = __builtin_fma(hh, k1[i], xv[6 + i]); }
    plant_rates(q, uv, acc, a2, r);
#pragma unroll
    for (int i = 0; i < 4; ++i) { k2[i] = r[i] * 0.5; q[i] = __builtin_fma(hh, k2[i], xv[6 + i]); }
    plant_rates(q, uv, acc, a3, r);
#pragma unroll
    for (int i = 0; i < 4; ++i) { k3[i] = r[i] * 0.5; q[i] = __builtin_fma(h, k3[i], xv[6 + i]); }
    plant_rates(q, uv, acc, a4, r);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double v = xv[3 + i];
        const double s12 = __builtin_fma(2.0, __builtin_fma(hh, a1[i], v), v);            // k1 + 2 k2
        const double s123 = __builtin_fma(2.0, __builtin_fma(hh, a2[i], v), s12);
        xv[i] = __builtin_fma(h6, __builtin_fma(h, a3[i], v) + s123, xv[i]);
        xv[3 + i] = __builtin_fma(h6, a4[i] + __builtin_fma(2.0, a3[i], __builtin_fma(2.0, a2[i], a1[i])), v);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        xv[6 + i] = __builtin_fma(h6, __builtin_fma(0.5, r[i], __builtin_fma(2.0, k3[i], __builtin_fma(2.0, k2[i], k1[i]))), xv[6 + i]);
}

// q / |q| on xv[6..9]; returns |q|
__device__ __forceinline__ double plant_renorm(double *xv)
{
#pragma clang fp contract(off)
    const double n = sqrt(__builtin_fma(xv[9], xv[9], __builtin_fma(xv[8], xv[8], __builtin_fma(xv[6], xv[6], xv[7] * xv[7]))));
#pragma unroll
    for (int i = 6; i < 10; ++i) xv[i] /= n;
    return n;
}

// One tick of the plant in place: xv[10] over `sub` substeps of length h with uv[4] and the force row f[o .. o + 2] (f null: none)
// held, then the quaternion renormalised once.
__device__ __forceinline__ void plant_tick(double *xv, const double *uv, const double *f, size_t o, double h, int sub, double inv_mass,
                                           double g)
{
    double acc[3];
    plant_acc(f, o, inv_mass, g, acc);
    for (int s = 0; s < sub; ++s) plant_rk4(xv, uv, acc, h);
    plant_renorm(xv);
}

// a vehicle's row of 2 N2 doubles in 16-byte pieces (rows of 10 and 4 doubles are 16-byte aligned)
template <int N2>
__device__ __forceinline__ void plant_ld_row(const double *p, double *r)
{
#pragma unroll
    for (int i = 0; i < N2; ++i) {
        const double2 t = reinterpret_cast<const double2 *>(p)[i];
        r[2 * i] = t.x; r[2 * i + 1] = t.y;
    }
}
template <int N2>
__device__ __forceinline__ void plant_st_row(double *p, const double *r)
{
#pragma unroll
    for (int i = 0; i < N2; ++i) reinterpret_cast<double2 *>(p)[i] = make_double2(r[2 * i], r[2 * i + 1]);
}

}  // namespace ndp
