"""Fixture of the reference-point tests (tests/test_ref_point.py, tests/test_ref_point_gpu.py): case families at the edges of the
device's reference point (csrc/ref_point.hpp), inputs and expected outputs.  The expected values are the 50-digit restatement's
(tests/ref_point_ref.py), rounded to double once; the oracle's own error against them, per family, sets the device's bar.

    python tests/golden/make_ref_point_golden.py            writes tests/golden/ref_point_golden.npz

Needs mpmath and the built oracle.  The coefficients are stored, not the waypoints: a linear solve is not bit-reproducible across
machines, the polynomial values of given coefficients are.

Point families (one-segment trajectories of length T, value number k of a point: c_k = value T^k / k!; with T = 2 and query time 0
the polynomial part is exact and the family tests the flatness map alone), arrays <family>_coeff[P,1,28] _tcum[P,2] _tseg[P,1]
_fpt[P,3] _t[P] -> _x[P,10] _u[P,4] _seg[P] _branch[P] _margin[P]:
  fixture    the 164 points of flat_golden.npz (what the reference's own flatness code was run on)
  attitude   thrust directions tilted up to 170 deg, |a + g e3| from 0.05 to 100 m/s^2, jerk up to 50 m/s^3, every yaw: at least 16
             points on each of the four quaternion branches
  yaw        k pi/2 + d, k = -8..8, d in {0, +-1e-15, +-1e-9, +-(pi/4 - 1e-9)} at level and at tilted thrust; random yaw within
             +-50, +-1e3, +-1e5 with yaw rates, level and tilted
  poly       septic and cubic coefficients, |c| <= 100, time_seg in {1/16, 1/4, 3.75, 48}, s in {0, 2^-30, 0.5, 1 - 2^-20, 1 - 2^-53}
The segments family, per n_seg in N_SEGS 8 segment-tagged vehicles (tests/ref_point_cases.py), arrays seg<n>_coeff[8,n,28] _tcum
_tseg _fpt:
  _t[8,Q]     every time_cum[i] with the double before and behind it, -0.01, 20 random times -> _x _u _seg _branch _margin
  _wt[W]      a node-0 time of vehicles 0..W-1 whose window crosses segments  -> _wx[W,N+1,10] _wu _wseg _wmargin at t + k dt
  _kt[8,T]    (n_seg in TICK_N_SEGS) the tick sequence's clocks, _ktt = t + T_horizon -> _kseg[8,T]; _kx[K,T,10] _ku _kmargin of
              vehicles 0..K-1
oracle_err_<family>: the oracle's error (max over components of |got - want| / max(1, |want|)) on the family's points.
"""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import ref_point_cases as RC  # noqa: E402
from tests import ref_point_ref as RP  # noqa: E402

G = RP.GRAVITY
N_WIN, DT_WIN = 20, 0.1                 # the window whose nodes 1..N are held (the engine's default horizon)
W_VEH, K_VEH = 2, 2                     # vehicles with stored window / tick values per n_seg
NZX_MIN = 1e-2                          # |z_b x x_c| below which the reference's own map is singular


def _points(pts, T=2.0):
    """[(p, v, a, j, yaw, yawd)] -> the arrays of a point family at query time 0"""
    P = len(pts)
    coeff = np.concatenate([RP.one_segment(*pt, T=T) for pt in pts], axis=0).reshape(P, 1, 28)
    return {"coeff": coeff, "tcum": np.tile([0.0, T], (P, 1)), "tseg": np.full((P, 1), T), "fpt": np.zeros((P, 3)), "t": np.zeros(P)}


def _fixture_family():
    flat = np.load(os.path.join(HERE, "flat_golden.npz"))
    return _points([(p[0:3], p[3:6], p[6:9], p[9:12], y[0], y[1]) for p, y in zip(flat["flat_pvaj"], flat["flat_yaw"])])


def _attitude_family():
    rng = np.random.Generator(np.random.PCG64(20251018))
    pts = []
    P = 144
    for i in range(P):
        tilt = np.deg2rad(rng.uniform(0.0, 90.0) if i % 3 == 0 else rng.uniform(90.0, 170.0))
        if i < 4:
            tilt = np.deg2rad(170.0)
        az = rng.uniform(0.0, 2 * np.pi)
        zb = np.array([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)])
        mag = (0.05, 100.0)[i % 2] if i < 8 else float(np.exp(rng.uniform(np.log(0.05), np.log(100.0))))
        a = mag * zb - np.array([0.0, 0.0, G])
        jd = rng.normal(size=3)
        j = jd / np.linalg.norm(jd) * (50.0 if i % 8 == 1 else rng.uniform(0.0, 50.0))
        pts.append((rng.uniform(-3, 3, 3), rng.uniform(-2, 2, 3), a, j, rng.uniform(-np.pi, np.pi), rng.uniform(-2.0, 2.0)))
    return _points(pts)


_TILTED = (np.array([3.0, -2.0, 1.0]), np.array([4.0, 1.0, -7.0]))      # a, j of the tilted thrust


def _yaw_family():
    rng = np.random.Generator(np.random.PCG64(20251019))
    pts = []
    z = np.zeros(3)
    for tilted in (False, True):
        a, j = _TILTED if tilted else (z, z)
        for k in range(-8, 9):
            for d in (0.0, 1e-15, -1e-15, 1e-9, -1e-9, np.pi / 4 - 1e-9, -(np.pi / 4 - 1e-9)):
                pts.append((z, z, a, j, k * (np.pi / 2) + d, 0.3))
        for lim in (50.0, 1e3, 1e5):
            for _ in range(24):
                pts.append((z, z, a, j, rng.uniform(-lim, lim), rng.uniform(-3.0, 3.0)))
    return _points(pts)


def _poly_family():
    rng = np.random.Generator(np.random.PCG64(20251020))
    coeff, tcum, tseg, tq = [], [], [], []
    for T in (1.0 / 16, 0.25, 3.75, 48.0):
        for s in (0.0, 2.0 ** -30, 0.5, 1.0 - 2.0 ** -20, np.nextafter(1.0, 0.0)):
            for cubic in (False, True):
                for draw in range(3):
                    c = rng.uniform(-100.0, 100.0, 28) * (1.0 if draw == 0 else 0.5 ** np.concatenate([np.arange(8)] * 3 + [np.arange(4)]))
                    if cubic:
                        c.reshape(-1)[[4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23]] = 0.0
                    t = s * T
                    assert t < T and (s == 0.0 or t > 0.0)
                    coeff.append(c); tcum.append([0.0, T]); tseg.append([T]); tq.append(t)
    P = len(tq)
    return {"coeff": np.array(coeff).reshape(P, 1, 28), "tcum": np.array(tcum), "tseg": np.array(tseg), "fpt": np.zeros((P, 3)),
            "t": np.array(tq)}


def _fused(t, k, dt):
    """t + k dt with the product not rounded (a fused multiply-add), correctly rounded"""
    return float(Fraction(t) + k * Fraction(dt))


def _window_time(rng, cum):
    """A node-0 time whose N_WIN + 1 node times are the same doubles with and without a fused multiply-add, cross a segment boundary
    where there is one, and stay 1e-9 s away from every time_cum entry at the nodes k > 0."""
    for _ in range(10000):
        t = float(rng.uniform(0.0, max(cum[-1] - 1.0, 0.5 * cum[-1])))
        tk = RC.node_times(t, N_WIN, DT_WIN)
        if any(_fused(t, k, DT_WIN) != tk[k] for k in range(N_WIN + 1)):
            continue
        if np.min(np.abs(tk[1:, None] - cum[None, :])) < 1e-9:
            continue
        if len(cum) > 2 and RC.segment_of(cum, tk[0]) == RC.segment_of(cum, tk[-1]):
            continue
        return t
    raise RuntimeError("no window time found")


def _segments_inputs():
    rng = np.random.Generator(np.random.PCG64(20251021))
    out = {}
    for n in RC.N_SEGS:
        coeff, cum, tseg, fpt = RC.tagged_trajectories(rng, RC.N_VEH, n)
        assert np.array_equal(cum * 64, np.rint(cum * 64)) and np.array_equal((cum - RC.T_HORIZON) + RC.T_HORIZON, cum)
        tq = []
        for v in range(RC.N_VEH):
            row = []
            for c in cum[v]:
                row += [np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)]
            row += [-0.01] + list(rng.uniform(0.0, cum[v, -1], 20))
            tq.append(row)
        out.update({f"seg{n}_coeff": coeff, f"seg{n}_tcum": cum, f"seg{n}_tseg": tseg, f"seg{n}_fpt": fpt, f"seg{n}_t": np.array(tq),
                    f"seg{n}_wt": np.array([_window_time(rng, cum[v]) for v in range(W_VEH)])})
        if n in RC.TICK_N_SEGS:
            kt = [RC.tick_times(cum[v], v) for v in range(RC.N_VEH)]
            out[f"seg{n}_kt"] = np.array([k[0] for k in kt])
            out[f"seg{n}_ktt"] = np.array([k[1] for k in kt])
    return out


def inputs():
    out = {}
    for name, fam in (("fixture", _fixture_family()), ("attitude", _attitude_family()), ("yaw", _yaw_family()), ("poly", _poly_family())):
        out.update({f"{name}_{k}": v for k, v in fam.items()})
    out.update(_segments_inputs())
    return out


def _mp_points(coeff, cum, tseg, fpt, times):
    """mp reference points of ONE vehicle at `times` (any shape) -> x, u, seg, branch, margin of that shape"""
    times = np.asarray(times, dtype=np.float64)
    x, u = np.zeros(times.shape + (10,)), np.zeros(times.shape + (4,))
    seg, br, mg = np.zeros(times.shape, dtype=np.int8), np.zeros(times.shape, dtype=np.int8), np.zeros(times.shape)
    for i in np.ndindex(times.shape):
        x[i], u[i], seg[i], br[i], mg[i] = RP.ref_point(coeff, cum, tseg, fpt, times[i])
    return x, u, seg, br, mg


def expected(g):
    """The expected outputs of every family, from the stored inputs alone."""
    out = {}
    for name in RC.POINT_FAMILIES:
        P = g[f"{name}_t"].shape[0]
        r = [_mp_points(g[f"{name}_coeff"][i], g[f"{name}_tcum"][i], g[f"{name}_tseg"][i], g[f"{name}_fpt"][i], g[f"{name}_t"][i]) for i in range(P)]
        for j, k in enumerate(("x", "u", "seg", "branch", "margin")):
            out[f"{name}_{k}"] = np.array([e[j] for e in r])
    for n in RC.N_SEGS:
        def veh(v, times):
            return _mp_points(g[f"seg{n}_coeff"][v], g[f"seg{n}_tcum"][v], g[f"seg{n}_tseg"][v], g[f"seg{n}_fpt"][v], times)
        r = [veh(v, g[f"seg{n}_t"][v]) for v in range(RC.N_VEH)]
        for j, k in enumerate(("x", "u", "seg", "branch", "margin")):
            out[f"seg{n}_{k}"] = np.array([e[j] for e in r])
        r = [veh(v, RC.node_times(float(t), N_WIN, DT_WIN)) for v, t in enumerate(g[f"seg{n}_wt"])]
        out[f"seg{n}_wx"], out[f"seg{n}_wu"] = np.array([e[0] for e in r]), np.array([e[1][:-1] for e in r])
        out[f"seg{n}_wseg"], out[f"seg{n}_wmargin"] = np.array([e[2] for e in r]), np.array([e[4] for e in r])
        if n in RC.TICK_N_SEGS:
            tt = g[f"seg{n}_ktt"]
            out[f"seg{n}_kseg"] = np.array([[RC.segment_of(g[f"seg{n}_tcum"][v], t) for t in tt[v]] for v in range(RC.N_VEH)], dtype=np.int8)
            r = [veh(v, tt[v]) for v in range(K_VEH)]
            assert all(np.array_equal(e[2], out[f"seg{n}_kseg"][v]) for v, e in enumerate(r))
            out[f"seg{n}_kx"], out[f"seg{n}_ku"], out[f"seg{n}_kmargin"] = (np.array([e[j] for e in r]) for j in (0, 1, 4))
    return out


def family_points(g, name):
    """Every stored point of a family as flat lists: (coeff, cum, tseg, fpt of its vehicle, time, x, u, seg, margin)"""
    pts = []
    if name in RC.POINT_FAMILIES:
        for i in range(g[f"{name}_t"].shape[0]):
            pts.append((g[f"{name}_coeff"][i], g[f"{name}_tcum"][i], g[f"{name}_tseg"][i], g[f"{name}_fpt"][i], float(g[f"{name}_t"][i]),
                        g[f"{name}_x"][i], g[f"{name}_u"][i], int(g[f"{name}_seg"][i]), float(g[f"{name}_margin"][i])))
        return pts
    for n in RC.N_SEGS:
        tr = [(g[f"seg{n}_coeff"][v], g[f"seg{n}_tcum"][v], g[f"seg{n}_tseg"][v], g[f"seg{n}_fpt"][v]) for v in range(RC.N_VEH)]
        for v in range(RC.N_VEH):
            for q, t in enumerate(g[f"seg{n}_t"][v]):
                pts.append(tr[v] + (float(t), g[f"seg{n}_x"][v, q], g[f"seg{n}_u"][v, q], int(g[f"seg{n}_seg"][v, q]), float(g[f"seg{n}_margin"][v, q])))
        for v, t0 in enumerate(g[f"seg{n}_wt"]):
            for k, t in enumerate(RC.node_times(float(t0), N_WIN, DT_WIN)[:-1]):      # (node N has no u row)
                pts.append(tr[v] + (float(t), g[f"seg{n}_wx"][v, k], g[f"seg{n}_wu"][v, k], int(g[f"seg{n}_wseg"][v, k]), float(g[f"seg{n}_wmargin"][v, k])))
        if n in RC.TICK_N_SEGS:
            for v in range(g[f"seg{n}_kx"].shape[0]):
                for i, t in enumerate(g[f"seg{n}_ktt"][v]):
                    pts.append(tr[v] + (float(t), g[f"seg{n}_kx"][v, i], g[f"seg{n}_ku"][v, i], int(g[f"seg{n}_kseg"][v, i]), float(g[f"seg{n}_kmargin"][v, i])))
    return pts


def oracle_error(oracle, g, name):
    """The oracle's error on a family, in the tests' metric; it must pick the restatement's segment and, where the margin decides
    it, its quaternion branch (a point on the wrong branch or segment is far outside any error worth the name: asserted here)."""
    err = 0.0
    for coeff, cum, tseg, fpt, t, x, u, seg, margin in family_points(g, name):
        pvaj, yaw = oracle.traj_point(coeff, cum, tseg, fpt, t)
        xo, uo = oracle.diff_flatness(pvaj, yaw)
        e = RC.point_err(xo[None], uo[None], x[None], u[None], np.array([margin]))
        assert e < 1e-6, (name, t, seg, e)
        err = max(err, e)
    return err


def check_conditions(g):
    """Conditions on the inputs (not measurements): asserted here and re-checked by tests/test_ref_point.py."""
    def nzx(x):
        """|z_b x x_c| of expected points: x_c is the unit horizontal vector in the plane of x_b and z_b"""
        R = RC.rot_of_q(x[..., 6:10])
        return np.abs(R[..., 2, 2]) / np.hypot(R[..., 2, 0], R[..., 2, 2])
    for name in RC.POINT_FAMILIES:
        low = int(np.count_nonzero(g[f"{name}_margin"] < RC.MARGIN))
        assert low <= (1 if name == "fixture" else 0), (name, low)
        assert name == "fixture" or np.min(nzx(g[f"{name}_x"])) >= NZX_MIN, (name, np.min(nzx(g[f"{name}_x"])))
    tn = g["attitude_u"][:, 3]
    tilt = np.degrees(np.arccos(np.clip(RC.rot_of_q(g["attitude_x"][:, 6:10])[:, 2, 2], -1, 1)))
    assert tn.min() < 0.0501 and tn.max() > 99.9 and tilt.max() > 169.9 and tilt.max() < 170.1
    br = g["attitude_branch"]
    assert all(np.count_nonzero(br == b) >= 16 for b in range(4)), np.bincount(br, minlength=4)
    for n in RC.N_SEGS:
        assert np.all(g[f"seg{n}_margin"] >= RC.MARGIN) and np.all(g[f"seg{n}_wmargin"] >= RC.MARGIN)
        assert all(np.min(RC.rot_of_q(g[f"seg{n}_{k}"][..., 6:10])[..., 2, 2]) > 0.3 for k in ("x", "wx"))       # flyable: tilt below 72 deg
        cum = g[f"seg{n}_tcum"]
        for v, t0 in enumerate(g[f"seg{n}_wt"]):
            tk = RC.node_times(float(t0), N_WIN, DT_WIN)
            assert np.min(np.abs(tk[1:, None] - cum[v][None, :])) >= 1e-9
        if n in RC.TICK_N_SEGS:
            assert np.all(g[f"seg{n}_kmargin"] >= RC.MARGIN)


def main():
    from oracle import oracle as O
    O.build()
    g = inputs()
    g.update(expected(g))
    check_conditions(g)
    for name in RC.POINT_FAMILIES + ("segments",):
        g[f"oracle_err_{name}"] = np.float64(oracle_error(O, g, name))
        print(name, "oracle error", g[f"oracle_err_{name}"], "bar", RC.bar(g[f"oracle_err_{name}"]))
    np.savez_compressed(RC.GOLDEN, **g)
    print("wrote", RC.GOLDEN, os.path.getsize(RC.GOLDEN), "bytes; attitude branches", np.bincount(g["attitude_branch"], minlength=4))


if __name__ == "__main__":
    main()
