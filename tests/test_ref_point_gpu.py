"""The device's reference point (csrc/ref_point.hpp) at its edges, against 50-digit values (tests/golden/ref_point_golden.npz; families,
conditions and the oracle's own error: tests/golden/make_ref_point_golden.py, tests/test_ref_point.py):

  a. values of every family through ref_window, at most max(8 x the oracle's error on the family, 32 x 2^-53) away in the metric
     max |got - want| / max(1, |want|); quaternions with their sign on all four branches; the segment read off the yaw tag;
  b. the list's advance (segment hint), the control tick's in-launch point (segment cache; and tick_pre_kernel in a child process) and
     ref_window make the same point bit for bit over a clock that jumps forward, back, onto segment boundaries and past the end;
  c. ref_window_kernel's transposed output at row counts below, on and over multiples of its 64-row workgroup, horizons 2 .. 46.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ref_point_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return RC.load()


def _node0(g, name, lo, hi):
    """node 0 of ref_window for points lo..hi of a point family: every point is a vehicle with a trajectory of one segment"""
    import ndp_nmpc_qd_amd as ndp
    eng = ndp.BatchedNMPC(hi - lo, load_mlp=False)
    RC.set_traj(eng, g[f"{name}_coeff"][lo:hi], g[f"{name}_tcum"][lo:hi], g[f"{name}_tseg"][lo:hi], g[f"{name}_fpt"][lo:hi])
    xr, ur = eng.ref_window(np.ascontiguousarray(g[f"{name}_t"][lo:hi]))
    eng.close()
    return xr[:, 0], ur[:, 0]


@pytest.fixture(scope="module")
def device_points(g):
    """x, u of every point family on the device, computed once (batches of at most 200 vehicles)"""
    out = {}
    for name in RC.POINT_FAMILIES:
        P = g[f"{name}_t"].shape[0]
        parts = [_node0(g, name, lo, min(lo + 200, P)) for lo in range(0, P, 200)]
        out[name] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    return out


@pytest.mark.parametrize("family", RC.POINT_FAMILIES)
def test_values_of_the_point_families(g, device_points, family):
    """fixture: the reference's own 164 flatness points; attitude: tilts to 170 deg, thrust 0.05 .. 100 m/s^2, all four quaternion
    branches; yaw: every quadrant k = -8 .. 8 at the ends of the kernel polynomials' interval, |yaw| to 1e5; poly: time_seg 1/16 .. 48
    at s = 0 .. 1 - 2^-53.  Measured on the MI355X (device error / oracle error / bar): see DESIGN.md, "Reference point: measured errors"."""
    x, u = device_points[family]
    oerr = float(g[f"oracle_err_{family}"])
    err = RC.point_err(x, u, g[f"{family}_x"], g[f"{family}_u"], g[f"{family}_margin"])
    print(f"\n{family}: device error {err:.3e}, oracle error {oerr:.3e}, bar {RC.bar(oerr):.3e}, {x.shape[0]} points")
    assert np.all(g[f"{family}_seg"] == 0)
    assert err <= RC.bar(oerr), (family, err, RC.bar(oerr))


@pytest.mark.parametrize("branch", (0, 1, 2, RC.TRACE))
def test_quaternion_of_every_branch_with_its_sign(g, device_points, branch):
    """quaternion_from_matrix's four branches as the device's selects take them: q itself (no comparison through R(q), no sign
    freedom) on the `attitude` points of each branch -- at least 16 each, branch margins of at least 1e-6."""
    x, _ = device_points["attitude"]
    sel = (g["attitude_branch"] == branch) & (g["attitude_margin"] >= RC.MARGIN)
    assert sel.sum() >= 16
    err = RC.rel_err(x[sel][:, 6:10], g["attitude_x"][sel][:, 6:10])
    print(f"\nbranch {branch}: {int(sel.sum())} points, quaternion error {err:.3e}")
    assert err <= RC.bar(float(g["oracle_err_attitude"])), (branch, err)


@pytest.fixture(scope="module")
def segment_errors():
    return {}


@pytest.mark.parametrize("n", RC.N_SEGS)
def test_values_and_segment_of_the_tagged_trajectories(g, segment_errors, n):
    """`segments`: every time_cum entry with the doubles before and behind it, t < 0, the end, 20 random times, at node 0; the nodes
    1 .. N of windows that cross segments.  The segment read off the yaw tag is the restatement's at every time (exact), the values
    are within the family's bar."""
    import ndp_nmpc_qd_amd as ndp
    coeff, cum, tseg, fpt, t = (g[f"seg{n}_{k}"] for k in ("coeff", "tcum", "tseg", "fpt", "t"))
    eng = ndp.BatchedNMPC(RC.N_VEH, load_mlp=False)
    RC.set_traj(eng, coeff, cum, tseg, fpt)
    Q = t.shape[1]
    x, u = np.empty((RC.N_VEH, Q, 10)), np.empty((RC.N_VEH, Q, 4))
    for q in range(Q):
        xr, ur = eng.ref_window(np.ascontiguousarray(t[:, q]))
        x[:, q], u[:, q] = xr[:, 0], ur[:, 0]
    seg = RC.decode_tag(x)
    assert np.array_equal(seg, g[f"seg{n}_seg"]), np.argwhere(seg != g[f"seg{n}_seg"])[:8]
    err = RC.point_err(x, u, g[f"seg{n}_x"], g[f"seg{n}_u"], g[f"seg{n}_margin"])
    # nodes 1 .. N (the same doubles t + k dt whether or not the device fuses the product into the sum: a condition of the fixture)
    wt = g[f"seg{n}_wt"]
    tw = np.zeros(RC.N_VEH)
    tw[:wt.shape[0]] = wt
    xr, ur = eng.ref_window(tw)
    W = wt.shape[0]
    assert xr.shape[1] == g[f"seg{n}_wx"].shape[1]
    assert np.array_equal(RC.decode_tag(xr[:W]), g[f"seg{n}_wseg"])
    werr = max(RC.point_err(xr[:W, :-1], ur[:W], g[f"seg{n}_wx"][:, :-1], g[f"seg{n}_wu"], g[f"seg{n}_wmargin"][:, :-1]),
               RC.rel_err(xr[:W, -1], g[f"seg{n}_wx"][:, -1]))
    oerr = float(g["oracle_err_segments"])
    eng.close()
    segment_errors[n] = max(err, werr)
    print(f"\nsegments, n_seg {n}: device error node 0 {err:.3e}, nodes 1..N {werr:.3e}; family so far {max(segment_errors.values()):.3e}, "
          f"oracle error {oerr:.3e}, bar {RC.bar(oerr):.3e}")
    assert max(err, werr) <= RC.bar(oerr), (n, err, werr)


# ------------------------------------------------------------------------------------------------ b. three paths, one point
@pytest.fixture(scope="module")
def two_launch_form(g):
    """The tick sequences once more in a child process that runs the tick's two-launch form (tick_pre_kernel in front of the control
    step; the form is chosen once per process: NDP_TICK_FORM, as test_one_clock_for_all_vehicles_and_the_two_launch_form does)."""
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "ndp_ref_point_pre_%d.npz" % os.getpid())
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "from tests import ref_point_cases as RC\n"
            "g = RC.load()\n"
            "out = {}\n"
            "for n in RC.TICK_N_SEGS:\n"
            "    out['x%%d' %% n], out['u%%d' %% n], out['rows%%d' %% n] = RC.run_tick_sequence(g, n)\n"
            "np.savez(%r, **out)\n" % (RC.ROOT, path))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NDP_TICK_FORM="pre"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(np.load(path))
    os.remove(path)
    return out


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("n", RC.TICK_N_SEGS)
def test_list_advance_tick_and_window_make_the_same_point(g, two_launch_form, n):
    """Per-vehicle clocks: 30 ticks at 20 ms, a jump forward over three segments or more, 5 ticks, a jump back to the start, 5 ticks,
    t + T_horizon on a time_cum entry and one double before and behind it, one double before the end, past the end, back to the middle,
    the same time twice more.  The list's advance keeps a segment hint and the tick a two-slot segment cache across all of that, the
    window kernel searches afresh: the newest entry (x now, its u row five ticks later) is the same from all of them, and from the
    two-launch form, bit for bit; its tag names the restatement's segment on every vehicle and its values are within the bar of
    `segments` on the vehicles whose 50-digit values the fixture holds."""
    x, u, rows = RC.run_tick_sequence(g, n)
    # this process ran the one-launch tick (tick_new_point with its segment cache), the child the two-launch form (tick_pre_kernel)
    assert rows and all(r.endswith("_TICK") for r in rows), rows
    pre_rows = [str(r) for r in two_launch_form[f"rows{n}"]]
    assert pre_rows and not any(r.endswith("_TICK") for r in pre_rows), pre_rows
    T = x.shape[1]
    for i in range(T):
        assert _same(x[0, i], x[2, i]), ("list advance / ref_window", n, i, np.argwhere(x[0, i] != x[2, i])[:4])
        assert _same(x[1, i], x[2, i]), ("tick / ref_window", n, i, np.argwhere(x[1, i] != x[2, i])[:4])
        if i < T - 5:
            assert _same(u[0, i], u[2, i]) and _same(u[1, i], u[2, i]), ("u row", n, i)
    assert not np.isnan(x).any() and not np.isnan(u[2]).any() and not np.isnan(u[0:2, :T - 5]).any()
    assert _same(two_launch_form[f"x{n}"], x) and _same(two_launch_form[f"u{n}"], u)
    seg = RC.decode_tag(x[2])                                  # [T, B]
    assert np.array_equal(seg.T, g[f"seg{n}_kseg"]), np.argwhere(seg.T != g[f"seg{n}_kseg"])[:8]
    K = g[f"seg{n}_kx"].shape[0]
    err = RC.point_err(x[2][:, :K].transpose(1, 0, 2), u[2][:, :K].transpose(1, 0, 2), g[f"seg{n}_kx"], g[f"seg{n}_ku"], g[f"seg{n}_kmargin"])
    oerr = float(g["oracle_err_segments"])
    print(f"\ntick sequence, n_seg {n}: {T} ticks, device error {err:.3e}, oracle error (family) {oerr:.3e}, bar {RC.bar(oerr):.3e}")
    assert err <= RC.bar(oerr), (n, err)


# ------------------------------------------------------------------------------------------------ c. the window kernel's layout
@pytest.fixture(scope="module")
def layout_traj():
    rng = np.random.Generator(np.random.PCG64(77))
    coeff, cum, tseg, fpt = RC.tagged_trajectories(rng, 64, 9)
    t = rng.uniform(-0.2, 1.0, 64) * cum[:, -1]                # in front of the start, inside, past the end within the window
    t[5] = cum[5, -1] + 0.5                                    # ... and a whole window at final_pt
    return coeff, cum, tseg, fpt, t


@pytest.mark.parametrize("N,B", [(2, 1), (2, 21), (2, 22), (2, 43), (15, 4), (15, 5), (20, 1), (20, 3), (20, 4), (20, 61), (20, 64),
                                 (31, 2), (31, 3), (31, 5), (46, 1), (46, 2), (46, 64)])
def test_window_kernel_layout_at_other_horizons_and_row_counts(oracle, layout_traj, N, B):
    """ref_window_kernel stages 64 (vehicle, node) rows per workgroup in LDS and writes x rows and u rows (there is no u row of node N)
    with its own index arithmetic: B (N + 1) rows below, on and just over a multiple of 64, N + 1 dividing 64 and not.  Tagged
    trajectories: a misplaced row is an O(1) error.  Outputs go into views of tensors one vehicle longer: the spare rows keep their
    sentinel."""
    import torch
    import ndp_nmpc_qd_amd as ndp
    coeff, cum, tseg, fpt, t = (a[:B] for a in layout_traj)
    dt = 0.1
    eng = ndp.BatchedNMPC(B, N=N, dt=dt, load_mlp=False)
    RC.set_traj(eng, coeff, cum, tseg, fpt)
    dev = torch.device("cuda", 0)
    sentinel = -1.2345e300
    xr = torch.full((B + 1, N + 1, 10), sentinel, dtype=torch.float64, device=dev)
    ur = torch.full((B + 1, N, 4), sentinel, dtype=torch.float64, device=dev)
    eng.ref_window_device(torch.from_numpy(np.ascontiguousarray(t)).to(dev), xr[:B], ur[:B])
    eng.synchronize()
    xr, ur = xr.cpu().numpy(), ur.cpu().numpy()
    eng.close()
    xo, uo = oracle.ref_window(coeff, cum, tseg, fpt, t, N=N, dt=dt)
    np.testing.assert_allclose(xr[:B], xo, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(ur[:B], uo, rtol=1e-9, atol=1e-9)
    assert np.all(xr[B] == sentinel) and np.all(ur[B] == sentinel)
    assert np.array_equal(RC.decode_tag(xr[:B]), RC.decode_tag(xo))
