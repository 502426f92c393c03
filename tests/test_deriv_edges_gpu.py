"""The control step's derivative kernels on the device at the horizons where their passes change shape (tests/deriv_edges.py: DERIV_EDGE_N;
run with -m gpu): the adjoint with and without the model gradient, forward mode, the level-2 and the parameter sensitivities against the
dense fixed-set references (tests/fixed_set_ref.py), duality of forward mode against the adjoint, the facts that hold exactly, guard rows
behind a ragged batch; the recompute kernels (rti_mjvp_kernel among them) at lowered instances per workgroup against the default launch;
and every optional pointer of the recompute entries, the model forward mode's included.  CPU side (the list, the seeds, the ledger, the host emulator): tests/test_deriv_edges.py."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests.deriv_edges import DERIV_EDGE_N, DEVICE_B, device_case, pick, small_case
from tests.deriv_gpu import _dev, _jvp, _mjvp, _recorded_step, _t, _tangents, _tt, _vjp, ndp  # noqa: F401
from tests.fixed_set_ref import jvp_apply, jvp_system, model_grad_ref, psens_apply, scale, sens_ref, vjp_apply
from tests.test_kernel_table_gpu import SENS_BAR, geometry

pytestmark = pytest.mark.gpu

T, GUARD = 2, 2
SET_DUALITY_BAR, IPM_DUALITY_BAR = 1e-10, 1e-6     # test_duality_with_the_adjoint_on_the_device's

# The batch seed per horizon (tests/deriv_edges.py: device_case).  Chosen on the CPU as the first seed from SEED0 + 2000 + 100 N on for which
# the oracle's twin of the warm-up and the recorded step (oracle.step_batch_as, twice) finishes at least 6 of the 37 instances in the
# active set and at least MIN_PINNED[N] of those with an input on a bound -- with the supplied force and, at the fusable horizons, with
# the oracle's downwash network's force (there 7 and 3: one to spare).  tests/test_deriv_edges.py checks every entry by that rule.
# (The first seed tried held at every horizon; the twin's counts with the supplied force: 37 set finishes of 37 throughout, pinned 5, 7, 12, 8,
# 6, 6, 4, 5, 5, 5, 5, 3, 7 in the list's order.)
SEEDS = {2: synth.SEED0 + 2200, 3: synth.SEED0 + 2300, 4: synth.SEED0 + 2400, 6: synth.SEED0 + 2600, 10: synth.SEED0 + 3000,
         12: synth.SEED0 + 3200, 15: synth.SEED0 + 3500, 16: synth.SEED0 + 3600, 17: synth.SEED0 + 3700, 19: synth.SEED0 + 3900,
         21: synth.SEED0 + 4100, 25: synth.SEED0 + 4500, 27: synth.SEED0 + 4700}
# Pinned set finishes required among the checked ones: two at every horizon (N = 2 and N = 3 included: their seeds give 5 and 7).
MIN_PINNED = {N: 2 for N in DERIV_EDGE_N}

# The lowered-waves cases (N, instances per workgroup) and the batch seed of each; the optional-pointer cases' horizons and seeds.  By the
# oracle's twin every one of their B instances is a status-0 set finish (tests/test_deriv_edges.py checks that), so their bit-equality
# compares numbers and linearity has one bar.
LOWERED = {(20, 2): synth.SEED0 + 2320, (13, 1): synth.SEED0 + 2313, (27, 1): synth.SEED0 + 2327}
LOWERED_B = 5
POINTERS = {20: synth.SEED0 + 2420, 17: synth.SEED0 + 2417}
POINTERS_B = 8

# (kernel, instances per workgroup) -> the test of this module that launches it; tests/test_deriv_edges.py checks that this is every
# combination ndp_create can give and that the named tests still have the horizons the rows rest on.  N = 20 runs the <20> kernels; every
# other horizon the <0> ones, at 4 instances per workgroup up to N = 19 and at 2 from N = 21.  The two reference tests hold what they launch
# to the dense references (the <0> kernels at 4 and at 2).  The lowered-waves test holds a lowered launch to the default launch of the same
# horizon, bit for bit: (<20>, 2) to (<20>, 4) and (<0>, 1) to (<0>, 4) at N = 13 and to (<0>, 2) at N = 27.  For the (<20>, 4) rows it is
# that baseline only; the <20> kernels at their default 4 are held to the dense references by the older modules
# (test_step_vjp_gpu.test_full_trajectory_upstream_matches_the_dense_reference,
# test_model_grad_gpu.test_device_model_gradient_matches_the_dense_reference,
# test_step_jvp_gpu.test_three_directions_match_the_dense_reference and
# test_step_model_jvp_gpu.test_three_directions_match_the_dense_reference, each at N = 20; tests/test_deriv_edges.py checks that they are
# there).  rti_mjvp_kernel's reference rows (<0> at 4 and at 2) name a test of tests/test_step_model_jvp_edges_gpu.py (MJVP_MODULE), which
# runs the same list of horizons.
MJVP_MODULE = "tests.test_step_model_jvp_edges_gpu"
RECOMPUTE_CASES = {
    ("rti_vjp_kernel<20>", 4): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_wvjp_kernel<20>", 4): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_jvp_kernel<20>", 4): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_mjvp_kernel<20>", 4): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_vjp_kernel<20>", 2): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_wvjp_kernel<20>", 2): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_jvp_kernel<20>", 2): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_mjvp_kernel<20>", 2): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_vjp_kernel<0>", 4): "test_adjoint_and_model_gradient_match_the_dense_references",
    ("rti_wvjp_kernel<0>", 4): "test_adjoint_and_model_gradient_match_the_dense_references",
    ("rti_jvp_kernel<0>", 4): "test_forward_mode_matches_the_dense_reference_and_the_adjoint",
    ("rti_mjvp_kernel<0>", 4): "test_model_directions_match_the_dense_reference_at_the_edge_horizons",
    ("rti_vjp_kernel<0>", 2): "test_adjoint_and_model_gradient_match_the_dense_references",
    ("rti_wvjp_kernel<0>", 2): "test_adjoint_and_model_gradient_match_the_dense_references",
    ("rti_jvp_kernel<0>", 2): "test_forward_mode_matches_the_dense_reference_and_the_adjoint",
    ("rti_mjvp_kernel<0>", 2): "test_model_directions_match_the_dense_reference_at_the_edge_horizons",
    ("rti_vjp_kernel<0>", 1): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_wvjp_kernel<0>", 1): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_jvp_kernel<0>", 1): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
    ("rti_mjvp_kernel<0>", 1): "test_lowered_waves_equal_the_default_launch_bit_for_bit",
}


def _finishes(r):
    ok = (r["st"] == 0) & ((r["it"] & 0xffff) == 0)
    return ok, ok & r["act"].any(axis=(1, 2))


def _sens_step(ndp, b, f, level):
    """_recorded_step's two steps on an engine of its own with the initial-state sensitivities on for the second: its own linearisation
    point, status, kept set and Jacobians."""
    import torch
    B, N = b["x0"].shape[0], b["xr"].shape[1] - 1
    eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
    eng.reset(b["xr"], b["ur"])
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur")}
    ft = _t(f, torch.float32)
    u0 = torch.empty(B, 4, dtype=torch.float64, device=_dev())
    eng.update_device(t["x0"], t["xr"], t["ur"], u0, f=ft)
    eng.synchronize()
    eng.enable_sensitivity(level)
    Xp, Up = eng.get_iterate()
    eng.update_device(t["x0"], t["xr"], t["ur"], u0, f=ft)
    eng.synchronize()
    st, it = eng.status()
    _, act = eng.active_set()
    r = dict(Xp=Xp, Up=Up, st=st, it=it, act=act, sens=eng.sensitivity(), waves=eng.debug_rti_launched()[1])
    eng.close()
    return r


@pytest.fixture(scope="module")
def edge(ndp, oracle):
    """Per horizon, built when first asked for: B = 37 mixed with a supplied fp32 force, a warm-up step, the recorded step and its tape;
    from that engine the adjoint with random (gu0, gX, gU), with and without the model gradient, and forward mode with T = 2 in all four
    tangents, every output with two guard rows; a second engine with level-2 sensitivities; at the fusable horizons a third, fused with
    neighbour windows, with the parameter sensitivities.  Every engine is closed here.  The dense systems of the 6 checked instances are
    built once and shared by the tests."""
    cache = {}

    def get(N):
        if N in cache:
            return cache[N]
        waves, fused = geometry(N)[:2]
        b, f = device_case(N, SEEDS[N], fused)
        r = _recorded_step(ndp, b, f=f)
        eng, a = r["eng"], (r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"])
        assert eng.debug_rti_launched()[1] == waves
        rng = np.random.default_rng(SEEDS[N] + 2)
        g = (rng.normal(size=(DEVICE_B, 4)), rng.normal(size=(DEVICE_B, N + 1, 10)), rng.normal(size=(DEVICE_B, N, 4)))
        gt = dict(zip(("gu0", "gX", "gU"), (_t(x) for x in g)))
        tan = _tangents(SEEDS[N] + 3, DEVICE_B, N, T)
        c = dict(N=N, b=b, f=f, r=r, g=g, tan=tan)
        c["wvjp"] = _vjp(eng, *a, f=r["force"], model=True, guard=GUARD, **gt)
        c["vjp"] = _vjp(eng, *a, f=r["force"], guard=GUARD, **gt)
        c["jvp"] = _jvp(eng, *a, T, f=r["force"], guard=GUARD, **_tt(tan))
        Xl, Ul, _ = (v.cpu().numpy() for v in r["tape"])
        eng.close()
        ok, pinned = _finishes(r)
        assert ok.sum() >= 6 and pinned.sum() >= MIN_PINNED[N], (N, int(ok.sum()), int(pinned.sum()))
        c["idx"] = pick(ok, pinned)
        cfg = oracle.default_cfg(N=N, use_fd=True)
        c["sys"] = {i: jvp_system(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f[i].astype(np.float64), Xl[i], Ul[i], r["act"][i])
                    for i in c["idx"]}
        c["gm"] = {i: model_grad_ref(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f[i].astype(np.float64), Xl[i], Ul[i], r["act"][i],
                                     g[0][i], g[1][i], g[2][i]) for i in c["idx"]}
        c["sens"] = _sens_step(ndp, b, f, 2)
        if fused:
            p = _recorded_step(ndp, b, fused=True, params=True)
            assert p["eng"].debug_rti_launched()[1] == waves
            p["tape"] = [v.cpu().numpy() for v in p["tape"]]
            p["force"] = p["force"].cpu().numpy().astype(np.float64)
            p["eng"].close()
            c["psens"] = p
        cache[N] = c
        return c

    return get


def _guards_intact(out, B):
    return all((x[B:] == -7.0).all() for x in out if x.dtype == np.float64) and all((x[B:] == -1).all() for x in out if x.dtype == np.int32)


def _recompute_is_the_step(c, u0c, stc):
    """status_check equals the recorded step's; u0_check its u0 within 1e-12 (the unfused in-place form: the two kernels' compiled
    arithmetic differs in the last bits)."""
    r, B = c["r"], DEVICE_B
    assert np.array_equal(stc[:B], r["st"])
    ok = r["st"] == 0
    rel = np.abs(u0c[:B] - r["u0"]).max(axis=1) / np.maximum(1.0, np.abs(r["u0"]).max(axis=1))
    assert rel[ok].max() <= 1e-12, rel[ok].max()


@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_adjoint_and_model_gradient_match_the_dense_references(edge, N):
    """rti_wvjp_kernel<0> and rti_vjp_kernel<0> at horizon N: on 6 seeded status-0 set finishes (pinned ones among them) gx0, gxr, gur, gf
    within 1e-9 of max(1, |g|max) of vjp_ref and gmodel of model_grad_ref; the plain adjoint's outputs bit-equal to the model call's;
    gmodel[6] and gmodel[15] exactly 0, stage 0's reference row, f_N and pinned rows exactly 0; the recompute is the step; the guard rows
    behind the ragged batch keep their fill."""
    c = edge(N)
    B, r, out, plain = DEVICE_B, c["r"], c["wvjp"], c["vjp"]
    for x, y in zip(out[:6], plain):
        assert np.array_equal(x, y, equal_nan=True)
    assert _guards_intact(out, B) and _guards_intact(plain, B)
    _recompute_is_the_step(c, out[4], out[5])
    worst = worst_m = 0.0
    for i in c["idx"]:
        ref = vjp_apply(c["sys"][i], c["g"][0][i], c["g"][1][i], c["g"][2][i])
        s = max(scale(x) for x in ref)
        for got, x in zip(out[:4], ref):
            worst = max(worst, np.max(np.abs(got[i] - x)) / s)
        rm, rm2 = c["gm"][i]
        assert abs(rm[14] - rm2) <= 1e-9 * scale(rm)
        worst_m = max(worst_m, np.max(np.abs(out[6][i] - rm)) / scale(rm))
    print(f"N={N}: adjoint, worst distance from the dense reference {worst:.3e}; model gradient {worst_m:.3e}")
    assert worst <= SENS_BAR and worst_m <= SENS_BAR, (N, worst, worst_m)
    ok = r["st"] == 0
    gm = out[6][:B]
    assert np.isfinite(gm[ok]).all() and not gm[ok][:, 6].any() and not gm[ok][:, 15].any()
    assert not out[1][:B][ok][:, 0].any() and not out[3][:B][ok][:, N].any()
    fin = _finishes(r)[0]
    assert not out[2][:B][fin][r["act"][fin] != 0].any()


@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_forward_mode_matches_the_dense_reference_and_the_adjoint(edge, N):
    """rti_jvp_kernel<0> at horizon N, T = 2 directions in all four tangents: on the 6 checked instances du0, dX, dU within 1e-9 of
    max(1, |z'|max) of jvp_apply; on every status-0 instance dX_0 = tx0 and du0 = dU_0 exactly, on every set finish the pinned rows of dU
    exactly 0; duality <gz, JVP(t)> = <VJP(gz), t> against the adjoint of the same tape within 1e-10 on every status-0 set finish of
    the batch; the recompute is the step; guard rows intact."""
    c = edge(N)
    B, r, out, tan, g = DEVICE_B, c["r"], c["jvp"], c["tan"], c["g"]
    assert _guards_intact(out, B)
    _recompute_is_the_step(c, out[3], out[4])
    worst = 0.0
    for i in c["idx"]:
        for k in range(T):
            ref = jvp_apply(c["sys"][i], *(t[i, k] for t in tan))
            s = max(scale(x) for x in ref[:3])
            assert np.max(np.abs(np.concatenate([ref[1].ravel(), ref[2].ravel()]) - ref[3])) <= 1e-9 * s
            for got, x in zip(out[:3], ref[:3]):
                worst = max(worst, np.max(np.abs(got[i, k] - x)) / s)
    print(f"N={N}: forward mode, worst distance from the dense reference {worst:.3e}")
    assert worst <= SENS_BAR, (N, worst)
    du0, dX, dU = (x[:B] for x in out[:3])
    ok = r["st"] == 0
    fin, pinned = _finishes(r)
    assert np.array_equal(dX[ok][:, :, 0], tan[0][ok]) and np.array_equal(du0[ok], dU[ok][:, :, 0])
    assert not dU[fin][np.broadcast_to((r["act"][fin] != 0)[:, None], dU[fin].shape)].any()
    gap = _duality_gap(c["vjp"], out, g, tan, B)
    print(f"N={N}: duality gap on {int(fin.sum())} set finishes ({int(pinned.sum())} pinned) {gap[fin].max():.3e}")
    assert gap[fin].max() <= SET_DUALITY_BAR, (N, gap[fin].max())


def _duality_gap(a, j, g, tan, B):
    """|<gz, JVP(t)> - <VJP(gz), t>| per instance, worst over the directions, of the larger side's magnitude (the largest |term|, at
    least 1)."""
    gap = np.zeros(B)
    flat = lambda xs: np.concatenate([x.reshape(B, -1) for x in xs], axis=1)  # noqa: E731
    for k in range(tan[0].shape[1]):
        lhs = [g[0] * j[0][:B, k], g[1] * j[1][:B, k], g[2] * j[2][:B, k]]
        rhs = [x[:B] * t[:, k] for x, t in zip(a[:4], tan)]
        mag = np.maximum(1.0, np.abs(flat(lhs + rhs)).max(axis=1))
        gap = np.maximum(gap, np.abs(flat(lhs).sum(axis=1) - flat(rhs).sum(axis=1)) / mag)
    return gap


@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_level2_sensitivities_match_the_dense_reference(edge, oracle, N):
    """rti_sens_kernel at horizon N, level 2, on an engine of its own over the same two steps: on 6 status-0 set finishes (pinned ones
    among them) du0/dx0, dU/dx0 and dX/dx0 within 1e-9 of max(1, |value|max) of sens_ref; dX_0 = I, du0 = dU_0 and pinned rows exactly
    0 on every set finish."""
    c = edge(N)
    s2, b, f = c["sens"], c["b"], c["f"]
    assert s2["waves"] == geometry(N)[0]
    ok, pinned = _finishes(s2)
    assert ok.sum() >= 6 and pinned.sum() >= MIN_PINNED[N]
    du0, dU, dX = s2["sens"]
    cfg = oracle.default_cfg(N=N, use_fd=True)
    worst = 0.0
    for i in pick(ok, pinned):
        qp = oracle.linearize(cfg, b["x0"][i], b["xr"][i], b["ur"][i], f[i].astype(np.float64), s2["Xp"][i], s2["Up"][i])
        r0, rU, rX = sens_ref(qp, s2["act"][i])
        worst = max(worst, np.max(np.abs(du0[i] - r0)) / scale(rU), np.max(np.abs(dU[i] - rU)) / scale(rU),
                    np.max(np.abs(dX[i] - rX)) / scale(rX))
    print(f"N={N}: level-2 sensitivities, worst distance from the dense reference {worst:.3e}")
    assert worst <= SENS_BAR, (N, worst)
    assert np.array_equal(dX[ok][:, 0], np.broadcast_to(np.eye(10), (ok.sum(), 10, 10))) and np.array_equal(du0[ok], dU[ok][:, 0])
    assert not dU[ok][s2["act"][ok] != 0].any()


@pytest.mark.parametrize("N", [N for N in DERIV_EDGE_N if geometry(N)[1]])
def test_parameter_sensitivities_match_the_dense_reference(edge, oracle, N):
    """rti_psens_kernel at the fusable horizons (N >= 9: the fused step with neighbour windows, the force the network's): on 6 status-0
    set finishes (2 pinned among them) du0/dxr, du0/dur, du0/df within 1e-9 of max(1, |J|max) of psens_ref; stage 0's reference rows,
    f_N and pinned stage-0 rows exactly 0."""
    c = edge(N)
    p, b = c["psens"], c["b"]
    ok, pinned = _finishes(p)
    assert ok.sum() >= 6 and pinned.sum() >= 2
    assert 0 < (np.abs(p["force"]).max(axis=(1, 2)) > 0).sum()            # (a force that is there)
    Xl, Ul, _ = p["tape"]
    cfg = oracle.default_cfg(N=N, use_fd=True)
    worst = 0.0
    for i in pick(ok, pinned):
        ref = psens_apply(jvp_system(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], p["force"][i], Xl[i], Ul[i], p["act"][i]))
        s = max(scale(x) for x in ref)
        worst = max(worst, *(np.max(np.abs(got[i] - x)) / s for got, x in zip(p["J"], ref)))
    print(f"N={N}: parameter sensitivities, worst distance from the dense reference {worst:.3e}")
    assert worst <= SENS_BAR, (N, worst)
    dxr, dur, df = p["J"]
    good = p["st"] == 0
    assert not dxr[good][:, :, 0].any() and not df[good][:, :, N].any()
    p0 = p["act"][ok][:, 0] != 0
    assert not dxr[ok][p0].any() and not dur[ok][p0].any() and not df[ok][p0].any()


def test_unfused_parameter_sensitivities_at_a_run_time_horizon_are_refused(ndp):
    """N = 6 cannot fuse the network (the four-wave slice is smaller than its weights), and the unfused kernel of a run-time horizon has no
    parameter sensitivities: the step says so and writes nothing."""
    N = 6
    assert not geometry(N)[1]
    b, _ = device_case(N, SEEDS[N])
    eng = ndp.BatchedNMPC(DEVICE_B, N=N)
    eng.reset(b["xr"], b["ur"])
    eng.enable_sensitivity(1)
    eng.enable_param_sensitivity()
    X, U = eng.get_iterate()
    with pytest.raises(ndp.NdpError, match=r"\(-2\).*parameter sensitivities at N != 20 \(or 2 instances per workgroup\) need the fused step"):
        eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False)
    X2, U2 = eng.get_iterate()
    assert np.array_equal(X, X2) and np.array_equal(U, U2) and np.isnan(eng.param_sensitivity()[0]).all()
    eng.close()


@pytest.mark.parametrize("N", [3, 4])
def test_duality_on_interior_point_finishes_either_side_of_the_sweep_switch(ndp, N):
    """qp_mode 1 at N = 3 (the plain sweep after an interior-point finish) and N = 4 (the LDL sweep): every status-0 instance finishes in
    the interior-point loop; the adjoint's and forward mode's outputs are finite there, pinned rows of dU exactly 0, and duality holds
    within 1e-6 (the barrier-weighted system)."""
    B = DEVICE_B
    b, f = device_case(N, SEEDS[N])
    r = _recorded_step(ndp, b, f=f, qp_mode=1)
    a = (r["eng"], r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"])
    rng = np.random.default_rng(SEEDS[N] + 4)
    g = (rng.normal(size=(B, 4)), rng.normal(size=(B, N + 1, 10)), rng.normal(size=(B, N, 4)))
    tan = _tangents(SEEDS[N] + 5, B, N, T)
    v = _vjp(*a, f=r["force"], guard=GUARD, **dict(zip(("gu0", "gX", "gU"), (_t(x) for x in g))))
    j = _jvp(*a, T, f=r["force"], guard=GUARD, **_tt(tan))
    r["eng"].close()
    assert _guards_intact(v, B) and _guards_intact(j, B)
    assert np.array_equal(v[5][:B], r["st"]) and np.array_equal(j[4][:B], r["st"])
    ok = r["st"] == 0
    assert ok.sum() >= B // 2 and ((r["it"] & 0xffff)[ok] > 0).all()
    assert all(np.isfinite(x[:B][ok]).all() for x in v[:4] + j[:3])
    dU = j[2][:B]
    assert not dU[ok][np.broadcast_to((r["act"][ok] != 0)[:, None], dU[ok].shape)].any()
    gap = _duality_gap(v, j, g, tan, B)
    print(f"N={N}: duality gap on {int(ok.sum())} interior-point finishes {gap[ok].max():.3e}")
    assert gap[ok].max() <= IPM_DUALITY_BAR, (N, gap[ok].max())


# ---------------------------------------------------------------- the recompute kernels at other instances per workgroup
@pytest.mark.parametrize("N,waves", list(LOWERED))
def test_lowered_waves_equal_the_default_launch_bit_for_bit(ndp, monkeypatch, N, waves):
    """NDP_DEV_WAVES (read by ndp_create) lowers the instances per workgroup; the recompute kernels launch with the handle's count.  B = 5:
    the adjoint, the adjoint with the model gradient and forward mode of a lowered handle equal those of a default handle on the same
    inputs, tape and upstreams, bit for bit (an instance is one wave; the kernel binary is the same), and nothing is written behind the
    batch; so does forward mode with a seeded model direction beside the data tangents (rti_mjvp_kernel).  The default launch of N = 20 is
    the <20> kernels' four-wave case."""
    B = LOWERED_B
    b, f = small_case(N, LOWERED[N, waves], B)
    rng = np.random.default_rng(N)
    gt = dict(gu0=_t(rng.normal(size=(B, 4))), gX=_t(rng.normal(size=(B, N + 1, 10))), gU=_t(rng.normal(size=(B, N, 4))))
    tan = _tt(_tangents(N + 1, B, N, T))
    tm = np.random.default_rng(N + 5).normal(size=(B, T, 16))
    dflt = _recorded_step(ndp, b, f=f)
    assert dflt["eng"].debug_rti_launched()[1] == geometry(N)[0] > waves
    monkeypatch.setenv("NDP_DEV_WAVES", str(waves))
    low = _recorded_step(ndp, b, f=f)
    monkeypatch.delenv("NDP_DEV_WAVES")
    assert low["eng"].debug_rti_launched()[1] == waves
    outs = []
    for r in (dflt, low):                                  # (both on the default handle's tape)
        a = (r["eng"], r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], dflt["tape"])
        outs.append(_vjp(*a, f=r["force"], guard=GUARD, **gt) + _vjp(*a, f=r["force"], model=True, guard=GUARD, **gt)
                    + _jvp(*a, T, f=r["force"], guard=GUARD, **tan) + _mjvp(*a, tm, f=r["force"], guard=GUARD, **tan))
        r["eng"].close()
    assert len(outs[0]) == 6 + 7 + 5 + 5
    for x, y in zip(*outs):
        assert np.array_equal(x, y, equal_nan=True)
    assert _guards_intact(outs[1], B)
    assert _finishes(dflt)[0].all() and _finishes(low)[0].all()          # (as the twin has it: numbers are compared, not NaNs)
    assert all(np.isfinite(x[:B]).all() for x in outs[1] if x.dtype == np.float64)


# ---------------------------------------------------------------- optional pointers
def _sums_to(parts, whole, what):
    """Linearity: the parts sum to the whole within 1e-10 of max(1, |value|max), on every instance."""
    worst = 0.0
    for k, w in enumerate(whole):
        tot = sum(p[k] for p in parts)
        for i in range(w.shape[0]):
            err = np.max(np.abs(tot[i] - w[i])) / scale(w[i])
            assert err <= SET_DUALITY_BAR, (what, k, i, err)
            worst = max(worst, err)
    return worst


@pytest.mark.parametrize("N", list(POINTERS))
def test_every_optional_pointer_of_the_recompute_entries(ndp, N):
    """B = 8 at N = 20 and N = 17.  Outputs: a call with only one of gx0, gxr, gur, gf (du0, dX, dU) non-null writes what the full call
    writes there, bit for bit.  Inputs: the three calls with only gu0, only gX and only gU (the four with one tangent each) sum to the
    full call within 1e-10 of max(1, |value|max): the derivative is linear in them.  The model entry (ndp_step_jvp_model_device): du0, dX
    and dU alone equal the full call's, bit for bit; the call with tmodel alone plus the call with the data tangents alone (tmodel zero)
    sum to the mixed call, and the 15 unit columns of the model (two calls, of 8 and of 7 directions) weighted by the direction's entries
    sum to the call along the full model direction, both within 1e-10."""
    import torch
    B = POINTERS_B
    b, f = small_case(N, POINTERS[N], B)
    r = _recorded_step(ndp, b, f=f)
    eng, a = r["eng"], (r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"])
    rng = np.random.default_rng(N + 2)
    gt = dict(gu0=_t(rng.normal(size=(B, 4))), gX=_t(rng.normal(size=(B, N + 1, 10))), gU=_t(rng.normal(size=(B, N, 4))))
    tan = _tt(_tangents(N + 3, B, N, T))
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    full_v = _vjp(eng, *a, f=r["force"], **gt)
    full_j = _jvp(eng, *a, T, f=r["force"], **tan)
    for k, (name, shape) in enumerate((("gx0", (B, 10)), ("gxr", (B, N + 1, 10)), ("gur", (B, N, 4)), ("gf", (B, N + 1, 3)))):
        one = z(*shape)
        eng.step_vjp_device(*a, f=r["force"], **gt, **{name: one})
        torch.cuda.synchronize()
        assert np.array_equal(one.cpu().numpy(), full_v[k], equal_nan=True), name
    for k, (name, shape) in enumerate((("du0", (B, T, 4)), ("dX", (B, T, N + 1, 10)), ("dU", (B, T, N, 4)))):
        one = z(*shape)
        eng.step_jvp_device(*a, f=r["force"], **tan, **{name: one})
        torch.cuda.synchronize()
        assert np.array_equal(one.cpu().numpy(), full_j[k], equal_nan=True), name
    parts_v = [_vjp(eng, *a, f=r["force"], **{k: v})[:4] for k, v in gt.items()]
    parts_j = [_jvp(eng, *a, T, f=r["force"], **{k: v})[:3] for k, v in tan.items()]
    tm = rng.normal(size=(B, T, 16))
    full_m = _mjvp(eng, *a, tm, f=r["force"], **tan)
    for k, (name, shape) in enumerate((("du0", (B, T, 4)), ("dX", (B, T, N + 1, 10)), ("dU", (B, T, N, 4)))):
        one = z(*shape)
        eng.step_jvp_device(*a, f=r["force"], tmodel=_t(tm), **tan, **{name: one})
        torch.cuda.synchronize()
        assert np.array_equal(one.cpu().numpy(), full_m[k], equal_nan=True), name
    alone_m = _mjvp(eng, *a, tm, f=r["force"])
    parts_m = [alone_m[:3], _mjvp(eng, *a, np.zeros((B, T, 16)), f=r["force"], **tan)[:3]]
    eye = np.eye(16)
    cols = [_mjvp(eng, *a, np.ascontiguousarray(np.broadcast_to(eye[lo:hi][None], (B, hi - lo, 16))), f=r["force"])[:3]
            for lo, hi in ((0, 8), (8, 15))]
    unit = [np.concatenate([c[k] for c in cols], axis=1) for k in range(3)]          # [B,15,...]: the tangent along each unit column
    parts_c = [[np.einsum("btj,bj...->bt...", tm[:, :, :15], u) for u in unit]]
    eng.close()
    assert _finishes(r)[0].all()                                         # (as the twin has it: every instance is held, to the one bar)
    wv, wj = _sums_to(parts_v, full_v[:4], "adjoint"), _sums_to(parts_j, full_j[:3], "forward mode")
    wm, wc = _sums_to(parts_m, full_m[:3], "model and data directions"), _sums_to(parts_c, alone_m[:3], "the model's unit columns")
    print(f"N={N}: single upstreams / tangents against the full call, worst {wv:.3e} / {wj:.3e}; tmodel alone + data alone against the "
          f"mixed call {wm:.3e}; the 15 unit columns against the full model direction {wc:.3e}")
