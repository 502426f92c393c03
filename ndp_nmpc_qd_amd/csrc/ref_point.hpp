// ref_point.hpp -- device code of the rows that more than one unit's kernels inline (rows.hip: ref_window_kernel, ref_list_fill_kernel,
// throttle_kernel; tick.hip: tick_pre_kernel; rti_kernels.hip: the one-launch tick): the reference point in its three pieces with the
// f64 flatness helpers, the store of a point into the reference list, and one update of the hover-throttle estimator.
#pragma once
#include <hip/hip_runtime.h>

#include "kern_args.hpp"
#include "mlp_common.hpp"   // nc_mul / nc_add

namespace ndp {

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
// fdlibm kernel polynomials -- deterministic, shared by every kernel that makes a reference point.  sincos_n is not correctly rounded
// and not "under 1 ulp": its ABSOLUTE error stays under 2^-52 = 2.2e-16 (one rounding of the reduced argument + the kernels' ulp; held
// on the device for |x| <= 1e5 by the `yaw` family of tests/test_ref_point_gpu.py and on a port of this arithmetic for |x| <= 1e8 by
// tests/test_ref_point.py, largest seen 1.9e-16); in ulps of the result that is up to ~2 on random arguments and more beside a zero.
// The quadrant comes from (int)k: |x| must stay below 2^31 pi / 2 ~ 3.4e9.
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

// a point -> list entry j of vehicle b, both copies (the list's layout: RingGeom, rows.hip)
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

// Hover-throttle estimator (2-state Kalman filter on [f_collect, k_throttle] + Tustin differentiator): see rows.hip, f3.
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

}  // namespace ndp
