"""One reference point restated in mpmath at 50 digits: segment choice, polynomial values, flatness map, quaternion, x / u packing.

Written from the formulas the oracle cites (base_pt_publisher.py:93-133: hover at final_pt past the end, first time_cum entry
above t minus one, normalised segment time, derivative d carries d! / time_seg^d; pt_publisher.py:188-248: thrust direction,
heading, body axes, body rates from the jerk, quaternion_from_matrix of ROS geometry with its trace branch and three diagonal
branches; :115-146: x = [p, v, qw, qx, qy, qz], u = [wx, wy, wz, collective force / mass]).  Every input is a double and enters
exactly; nothing is rounded before the end.  Needs mpmath: the CPU tests and the fixture generator use it, the GPU tests read
the generator's output (tests/golden/ref_point_golden.npz) instead.
"""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50

MASS, GRAVITY = 1.4844, 9.81
TRACE = 3            # branch number of the trace branch; 0, 1, 2 = index of the largest diagonal entry of R


def _m(v):
    return mpf(float(v))


def segment(time_cum, t):
    """-1: hover at final_pt (t >= time_cum[-1]); else the first entry above t, minus one, 0 for t in front of time_cum[0]."""
    time_cum = [float(v) for v in time_cum]
    t = float(t)
    if t >= time_cum[-1]:
        return -1
    i = 0
    while i < len(time_cum) - 1 and not time_cum[i] > t:
        i += 1
    return max(i - 1, 0)


def _poly(c, s, d):
    """d-th derivative of sum_i c[i] s^i at s."""
    acc = mpf(0)
    for i in range(d, len(c)):
        f = mpf(1)
        for k in range(d):
            f *= (i - k)
        acc += f * c[i] * s ** (i - d)
    return acc


def traj_point_mp(coeff, time_cum, time_seg, final_pt, t):
    """coeff[n_seg, 28] of one vehicle (x8 y8 z8 yaw4 per segment) -> (pvaj[12], yaw, yaw rate, segment), mpf."""
    coeff = np.asarray(coeff, dtype=np.float64)
    seg = segment(time_cum, t)
    if seg < 0:
        return [_m(v) for v in final_pt] + [mpf(0)] * 9, mpf(0), mpf(0), seg
    ts = _m(time_seg[seg])
    s = (_m(t) - _m(time_cum[seg])) / ts
    rec = [_m(v) for v in coeff[seg]]
    pvaj = [_poly(rec[8 * a:8 * a + 8], s, d) / ts ** d for d in range(4) for a in range(3)]
    return pvaj, _poly(rec[24:28], s, 0), _poly(rec[24:28], s, 1) / ts, seg


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _unit(a):
    n = mp.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return [v / n for v in a], n


def quaternion_mp(R):
    """quaternion_from_matrix on the 3x3 rotation R (homogeneous entry 1): ([x, y, z, w], branch, margin)."""
    d = [R[0][0], R[1][1], R[2][2]]
    tt = d[0] + d[1] + d[2] + 1
    q = [None] * 4
    if tt > 1:
        branch, margin = TRACE, tt - 1
        q[3] = tt
        q[2] = R[1][0] - R[0][1]
        q[1] = R[0][2] - R[2][0]
        q[0] = R[2][1] - R[1][2]
    else:
        i = 1 if d[1] > d[0] else 0
        if d[2] > d[i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        srt = sorted(d)
        branch, margin = i, min(1 - tt, srt[2] - srt[1])
        tt = d[i] - (d[j] + d[k]) + 1
        q[i] = tt
        q[j] = R[i][j] + R[j][i]
        q[k] = R[k][i] + R[i][k]
        q[3] = R[k][j] - R[j][k]
    sc = mpf(1) / (2 * mp.sqrt(tt))
    return [v * sc for v in q], branch, margin


def flatness_mp(pvaj, yaw, yawd, mass=MASS, g=GRAVITY):
    """The flatness map on mpf values: dict with x[10], u[4], R (rows), rates, force, q_xyzw, branch, margin, nzx = |z_b x x_c|."""
    acc, jerk = pvaj[6:9], pvaj[9:12]
    zb, tn = _unit([acc[0], acc[1], acc[2] + _m(g)])
    xc = [mp.cos(yaw), mp.sin(yaw), mpf(0)]
    yb, nzx = _unit(_cross(zb, xc))
    xb = _cross(yb, zb)
    zj = zb[0] * jerk[0] + zb[1] * jerk[1] + zb[2] * jerk[2]
    ho = [(jerk[i] - zj * zb[i]) / tn for i in range(3)]            # mass / u1 = 1 / |t_des|
    wp = -(ho[0] * yb[0] + ho[1] * yb[1] + ho[2] * yb[2])
    wq = ho[0] * xb[0] + ho[1] * xb[1] + ho[2] * xb[2]
    wr = yawd * zb[2]
    R = [[xb[i], yb[i], zb[i]] for i in range(3)]
    q, branch, margin = quaternion_mp(R)
    return {"x": list(pvaj[0:6]) + [q[3], q[0], q[1], q[2]], "u": [wp, wq, wr, tn], "R": R, "rates": [wp, wq, wr],
            "force": tn * _m(mass), "q_xyzw": q, "branch": branch, "margin": margin, "nzx": nzx}


def _f(v):
    return np.array([float(e) for e in v])


def ref_point(coeff, time_cum, time_seg, final_pt, t, mass=MASS, g=GRAVITY):
    """One reference point of one vehicle at trajectory time t (a double): (x[10], u[4], segment, branch, margin), the values
    rounded to double once, at the end."""
    pvaj, yaw, yawd, seg = traj_point_mp(coeff, time_cum, time_seg, final_pt, t)
    f = flatness_mp(pvaj, yaw, yawd, mass, g)
    return _f(f["x"]), _f(f["u"]), seg, f["branch"], float(f["margin"])


def one_segment(p, v, a, j, yaw, yawd, T=2.0):
    """A prescribed point as a one-segment trajectory: c_k = value T^k / k!, so that the point sits at s = 0 (query time 0).
    Returns coeff[1, 28]; time_cum = [0, T], time_seg = [T]."""
    c = np.zeros((1, 28))
    for ax in range(3):
        c[0, 8 * ax + 0] = p[ax]
        c[0, 8 * ax + 1] = v[ax] * T
        c[0, 8 * ax + 2] = a[ax] * T ** 2 / 2.0
        c[0, 8 * ax + 3] = j[ax] * T ** 3 / 6.0
    c[0, 24], c[0, 25] = yaw, yawd * T
    return c
