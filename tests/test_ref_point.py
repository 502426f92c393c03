"""The reference point's 50-digit restatement (tests/ref_point_ref.py) and the fixture made with it (tests/golden/ref_point_golden.npz,
tests/golden/make_ref_point_golden.py): the restatement against what the reference's own code produced, the committed fixture
against the generator, the conditions the case families are built to, and the oracle's error on them -- which sets the bar the
device is held to in tests/test_ref_point_gpu.py."""
import os

import numpy as np
import pytest

from tests import ref_point_cases as RC  # noqa: E402
from tests import ref_point_ref as RP  # noqa: E402
from tests.golden import make_ref_point_golden as GEN  # noqa: E402

ROOT = RC.ROOT


@pytest.fixture(scope="module")
def g():
    return dict(RC.load())


@pytest.fixture(scope="module")
def flat():
    return np.load(os.path.join(ROOT, "tests", "golden", "flat_golden.npz"))


def _f(v):
    return np.array([[float(e) for e in row] for row in v]) if isinstance(v[0], list) else np.array([float(e) for e in v])


def test_restatement_against_the_reference_flatness_fixture(flat):
    """flat_golden.npz: R_wb, body rates, collective force and quaternion as the reference's own code computed them -- the bars of
    test_oracle_flatness_against_the_reference_code.  One of the 164 points sits on a tie between two quaternion branches (margin
    below 1e-6): its quaternion is compared through R(q)."""
    branches, ties = [], 0
    for p, y, R, w, F, q_xyzw in zip(flat["flat_pvaj"], flat["flat_yaw"], flat["flat_R"], flat["flat_rates"], flat["flat_force"], flat["flat_q"]):
        f = RP.flatness_mp([RP.mpf(float(v)) for v in p], RP.mpf(float(y[0])), RP.mpf(float(y[1])))
        np.testing.assert_allclose(_f(f["R"]), R, rtol=0, atol=1e-12)
        np.testing.assert_allclose(_f(f["rates"]), w, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(float(f["force"]), F, rtol=1e-13)
        x = _f(f["x"])
        np.testing.assert_array_equal(x[0:6], p[0:6])
        assert abs(np.linalg.norm(x[6:10]) - 1) < 1e-15
        if f["margin"] >= RC.MARGIN:
            np.testing.assert_allclose(_f(f["q_xyzw"]), q_xyzw, rtol=0, atol=1e-13)
        else:
            ties += 1
            np.testing.assert_allclose(RC.rot_of_q(x[6:10]), R, rtol=0, atol=1e-12)
        branches.append(f["branch"])
    assert ties <= 1
    assert np.bincount(branches, minlength=4)[RP.TRACE] >= 150 and np.bincount(branches, minlength=4)[1] == 0     # (why `attitude` exists)


def test_restatement_against_the_reference_trajectory_fixture():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ref_golden.npz"))
    for c in range(4):
        tseg, coeff, tq = gold[f"tseg_{c}"], gold[f"coeff_{c}"], gold[f"tq_{c}"]
        cum = np.concatenate([np.zeros((tseg.shape[0], 1)), np.cumsum(tseg, axis=1)], axis=1)
        for v in range(tseg.shape[0]):
            for s in range(0, tq.shape[1], 3):
                pvaj, yaw, yawd, _ = RP.traj_point_mp(coeff[v], cum[v], tseg[v], np.zeros(3), tq[v, s])
                want = gold[f"pvaj_{c}"][v, s]
                assert np.max(np.abs(_f(pvaj) - want) / (1.0 + np.abs(want))) < 1e-11
                np.testing.assert_allclose([float(yaw), float(yawd)], gold[f"yaw_{c}"][v, s], rtol=1e-11, atol=1e-12)


def test_segment_rule_and_quaternion_branches_of_the_restatement():
    cum = [0.5, 1.0, 1.5, 3.0]
    for t, want in ((-1.0, 0), (0.25, 0), (0.5, 0), (np.nextafter(1.0, 0), 0), (1.0, 1), (np.nextafter(1.5, 0), 1), (1.5, 2),
                    (np.nextafter(3.0, 0), 2), (3.0, -1), (4.0, -1)):
        assert RP.segment(cum, t) == want == RC.segment_of(cum, t), t
    # half turns about the three axes sit in the middle of the three diagonal branches, the identity on the trace branch
    for i, d in enumerate(([1, -1, -1], [-1, 1, -1], [-1, -1, 1])):
        q, br, mg = RP.quaternion_mp([[RP.mpf(d[r]) if r == c else RP.mpf(0) for c in range(3)] for r in range(3)])
        assert br == i and float(mg) == 1.0 and [float(v) for v in q] == [1.0 if k == i else 0.0 for k in range(4)]
    q, br, mg = RP.quaternion_mp([[RP.mpf(int(r == c)) for c in range(3)] for r in range(3)])
    assert br == RP.TRACE and float(mg) == 3.0 and [float(v) for v in q] == [0.0, 0.0, 0.0, 1.0]


def test_committed_fixture_is_what_the_generator_computes(g, flat):
    """The expected values from the stored inputs alone, exactly; the `fixture` family's inputs from flat_golden.npz, exactly."""
    want = GEN.expected(g)
    assert want and set(want) < set(g)
    for k, v in want.items():
        assert g[k].dtype == v.dtype and np.array_equal(g[k], v), k
    pts = [(p[0:3], p[3:6], p[6:9], p[9:12], y[0], y[1]) for p, y in zip(flat["flat_pvaj"], flat["flat_yaw"])]
    assert np.array_equal(g["fixture_coeff"], np.concatenate([RP.one_segment(*pt) for pt in pts]).reshape(164, 1, 28))
    # ... and its expected values are the reference code's, through the one-segment trajectory
    tie = g["fixture_margin"] < RC.MARGIN
    np.testing.assert_allclose(RC.rot_of_q(g["fixture_x"][:, 6:10]), flat["flat_R"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(g["fixture_x"][~tie][:, [7, 8, 9, 6]], flat["flat_q"][~tie], rtol=0, atol=1e-13)
    np.testing.assert_allclose(g["fixture_u"][:, 0:3], flat["flat_rates"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(g["fixture_u"][:, 3] * RP.MASS, flat["flat_force"], rtol=1e-13)


def test_case_families_are_complete_and_meet_their_conditions(g):
    GEN.check_conditions(g)                                   # margins, |z_b x x_c|, branch counts, node distances: see there
    assert g["fixture_t"].shape == (164,) and int(np.count_nonzero(g["fixture_margin"] < RC.MARGIN)) <= 1
    assert set(np.unique(g["fixture_branch"])) == {0, 2, RP.TRACE}
    # yaw: every k pi/2 + d, level and tilted, then the random ones
    d7 = (0.0, 1e-15, -1e-15, 1e-9, -1e-9, np.pi / 4 - 1e-9, -(np.pi / 4 - 1e-9))
    grid = np.array([k * (np.pi / 2) + d for k in range(-8, 9) for d in d7])
    yaw = g["yaw_coeff"][:, 0, 24]
    assert yaw.shape == (2 * (grid.size + 72),)
    for h in range(2):
        o = h * (grid.size + 72)
        assert np.array_equal(yaw[o:o + grid.size], grid)
        for i, lim in enumerate((50.0, 1e3, 1e5)):
            r = np.abs(yaw[o + grid.size + 24 * i:o + grid.size + 24 * (i + 1)])
            assert r.max() <= lim and r.max() > 0.8 * lim
    assert np.all(g["yaw_coeff"][:191, 0, 0:24] == 0.0) and np.all(g["yaw_coeff"][191:, 0, 2] != 0.0)       # level, then tilted
    assert np.all(g["yaw_coeff"][:, 0, 25] != 0.0)                                                          # yaw rates
    quadrants = np.rint(grid * (2 / np.pi)).astype(int)
    assert set(quadrants) == set(range(-8, 9))
    # poly: every (time_seg, s) pair, septic and cubic
    assert g["poly_t"].shape == (120,) and np.max(np.abs(g["poly_coeff"])) <= 100.0
    pairs = {(float(T), float(t)) for T, t in zip(g["poly_tseg"][:, 0], g["poly_t"])}
    assert pairs == {(T, s * T) for T in (1.0 / 16, 0.25, 3.75, 48.0) for s in (0.0, 2.0 ** -30, 0.5, 1.0 - 2.0 ** -20, np.nextafter(1.0, 0.0))}
    assert np.all(g["poly_t"] < g["poly_tseg"][:, 0])
    cubic = np.all(g["poly_coeff"][:, 0, [4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23]] == 0.0, axis=1)
    assert cubic.sum() == 60
    for fam in ("attitude", "yaw", "fixture"):                # T = 2, query time 0: the polynomial part is exact
        assert np.all(g[f"{fam}_t"] == 0.0) and np.all(g[f"{fam}_tseg"] == 2.0)
    # segments
    for n in RC.N_SEGS:
        cum, tseg, coeff, t = g[f"seg{n}_tcum"], g[f"seg{n}_tseg"], g[f"seg{n}_coeff"], g[f"seg{n}_t"]
        assert coeff.shape == (RC.N_VEH, n, 28) and t.shape == (RC.N_VEH, 3 * (n + 1) + 21)
        assert np.array_equal(tseg * 64, np.rint(tseg * 64)) and tseg.min() >= 1 / 16 and tseg.max() <= 2.0
        assert np.array_equal(cum, np.concatenate([np.zeros((RC.N_VEH, 1)), np.cumsum(tseg, axis=1)], axis=1))
        assert np.array_equal((cum - RC.T_HORIZON) + RC.T_HORIZON, cum)
        assert len({tuple(r) for r in tseg}) == (RC.N_VEH if n > 1 else len({tuple(r) for r in tseg}))        # per-vehicle lengths
        b = t[:, :3 * (n + 1)].reshape(RC.N_VEH, n + 1, 3)
        assert np.array_equal(b[:, :, 1], cum) and np.array_equal(b[:, :, 0], np.nextafter(cum, -np.inf)) and np.array_equal(b[:, :, 2], np.nextafter(cum, np.inf))
        assert np.all(t[:, 3 * (n + 1)] == -0.01) and np.all(t[:, 3 * (n + 1) + 1:] >= 0) and np.all(t[:, 3 * (n + 1) + 1:] < cum[:, -1:])
        # the tag is readable off every expected point and names the restatement's segment (-1: hover past the end)
        assert np.array_equal(RC.decode_tag(g[f"seg{n}_x"]), g[f"seg{n}_seg"])
        assert np.array_equal(RC.decode_tag(g[f"seg{n}_wx"]), g[f"seg{n}_wseg"])
        assert np.array_equal(g[f"seg{n}_seg"][:, :3 * (n + 1)].reshape(RC.N_VEH, n + 1, 3)[:, :, 1],
                              np.tile(np.concatenate([np.arange(n), [-1]]), (RC.N_VEH, 1)))
        assert np.all(g[f"seg{n}_seg"][:, 3 * (n + 1)] == 0)                                                  # t < 0: segment 0
        if n in RC.TICK_N_SEGS:
            for v in range(RC.N_VEH):
                kt, ktt = RC.tick_times(cum[v], v)
                assert np.array_equal(kt, g[f"seg{n}_kt"][v]) and np.array_equal(ktt, g[f"seg{n}_ktt"][v]) and np.array_equal(kt + RC.T_HORIZON, ktt)
                j = n - 2
                assert list(ktt[42:46]) == [cum[v, j], np.nextafter(cum[v, j], -np.inf), np.nextafter(cum[v, j], np.inf), np.nextafter(cum[v, -1], 0.0)]
                sg = g[f"seg{n}_kseg"][v]
                assert list(sg[42:47]) == [j, j - 1, j, n - 1, -1] and ktt[46] > cum[v, -1] and ktt[47] == ktt[48] == ktt[49]
                assert sg[30] >= sg[29] + 3 and sg[36] <= 1 and sg[47] == n // 2                               # the jumps
                assert np.all(np.abs(np.diff(kt[:30]) - 0.02) < 1e-12)
            assert np.array_equal(RC.decode_tag(g[f"seg{n}_kx"]), g[f"seg{n}_kseg"][:g[f"seg{n}_kx"].shape[0]])


@pytest.mark.parametrize("family", RC.POINT_FAMILIES + ("segments",))
def test_oracle_error_on_the_families_sets_the_device_bar(oracle, g, family):
    """oracle.traj_point + oracle.diff_flatness against the 50-digit values: the oracle picks the restatement's segment and quaternion
    branch everywhere (a point on another branch or of another segment is an O(1) error; `segments` also through the tag), and its error
    is what the fixture stores -- the device's bar is max(8 x that, 32 x 2^-53).  (Stored and measured may differ by the host's libm:
    held within a factor of two of each other.)"""
    err = GEN.oracle_error(oracle, g, family)                 # asserts < 1e-6 at every point
    stored = float(g[f"oracle_err_{family}"])
    print(f"{family}: oracle error {err:.3e} (stored {stored:.3e}), device bar {RC.bar(stored):.3e}")
    tiny = 2.0 ** -53
    assert err <= 2 * max(stored, tiny) and stored <= 2 * max(err, tiny)
    if family == "segments":
        for coeff, cum, tseg, fpt, t, x, u, seg, margin in GEN.family_points(g, family):
            xo, _ = oracle.diff_flatness(*oracle.traj_point(coeff, cum, tseg, fpt, t))
            assert int(RC.decode_tag(xo)) == seg


def _sincos_port(x):
    """sincos_n of csrc/ref_point.hpp, operation for operation; every fused multiply-add exact (one rounding), through mpmath."""
    from mpmath import mp, mpf

    def fma(a, b, c):
        with mp.workprec(400):
            return float(mpf(a) * mpf(b) + mpf(c))
    k = float(np.rint(x * 6.36619772367581382433e-01))
    r = fma(-k, 1.57079632673412561417e+00, x)
    r = fma(-k, 6.07710050630396597660e-11, r)
    r = fma(-k, 2.02226624871116645580e-21, r)
    z = r * r
    ps = fma(z, fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08), 2.75573137070700676789e-06),
                           -1.98412698298579493134e-04), 8.33333333332248946124e-03), -1.66666666666666324348e-01)
    s0 = fma(z * r, ps, r)
    pc = fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09), -2.75573143513906633035e-07),
                           2.48015872894767294178e-05), -1.38888888888741095749e-03), 4.16666666666666019037e-02)
    c0 = fma(z * z, pc, fma(-0.5, z, 1.0))
    q = int(k) & 3
    s1, c1 = (c0, s0) if q & 1 else (s0, c0)
    return (-s1 if q & 2 else s1), (-c1 if (q + 1) & 2 else c1)


def test_sincos_port_within_its_rounding_bound_up_to_1e8():
    """The arithmetic of sincos_n restated (not the compiled code: that is tests/test_ref_point_gpu.py, `yaw`, |x| <= 1e5) against
    50-digit sine and cosine on random arguments up to 1e3, 1e5, 1e8 and on the yaw grid k pi/2 + d.  Bound on the absolute error,
    from the operations: the reduced argument is rounded once at |r| <= pi/4 (2^-53 x 0.79 = 0.87e-16, passed on with a factor of
    at most 1), the fdlibm kernels stay under one ulp of a result of at most 1 (1.11e-16), what the three pieces of pi/2 leave out is
    below 1e-29 at k = 6.4e7: together under 2^-52 = 2.22e-16.  Measured on these arguments: 1.3e-16 up to 1e3, 1.5e-16 up to 1e5
    and up to 1e8 (1.9e-16 was the largest seen on 4 000 arguments per range).  In ulps of the RESULT that is 1.1 .. 1.5 on random
    arguments (2.1 seen) and 12 at cos(fl(pi/2)) = 6e-17, beside a zero: the routine is not correctly rounded and not "under 1 ulp"."""
    import math
    rng = np.random.default_rng(1)
    d7 = (0.0, 1e-15, -1e-15, 1e-9, -1e-9, np.pi / 4 - 1e-9, -(np.pi / 4 - 1e-9))
    grid = [k * (np.pi / 2) + d for k in range(-8, 9) for d in d7]
    for lim, xs in ((8 * np.pi, grid), (1e3, rng.uniform(-1e3, 1e3, 600)), (1e5, rng.uniform(-1e5, 1e5, 600)), (1e8, rng.uniform(-1e8, 1e8, 600))):
        ea = eu = 0.0
        for x in xs:
            s, c = _sincos_port(float(x))
            for got, want in ((s, RP.mp.sin(RP.mpf(float(x)))), (c, RP.mp.cos(RP.mpf(float(x))))):
                d = abs(RP.mpf(got) - want)
                ea, eu = max(ea, float(d)), max(eu, float(d / math.ulp(float(want))))
        print(f"|x| <= {lim:g}: absolute error {ea:.3e}, {eu:.2f} ulp of the result")
        assert ea <= 2.0 ** -52, (lim, ea)
