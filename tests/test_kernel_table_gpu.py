"""Every row of the control-step kernel table (enum RtiId in csrc/rti_table.hpp / k_rti in csrc/rti_kernels.hip) on the device, at every horizon (run with -m gpu).

Each row is an instantiation of its own (slots, instances per workgroup, fused or unfused downwash, compile-time or run-time horizon,
work-list phase, tick form, precision), with its own register allocation and lane predicates.  Every case below launches the rows it
names -- ndp_debug_rti_launched says which rows a handle really launched, and the case asserts that set exactly -- and compares what
they computed with a reference:
  * the oracle's plain-C twin of the active-set iterations (status, sweeps, kept sets identical, X and U within 1e-8);
  * the QP's KKT certificate (tests/kkt_certificate.py): 1e-9 for active-set answers, 3e5 tol for interior-point ones;
  * the dense fixed-set references of the sensitivities (tests/fixed_set_ref.py), 1e-9;
  * the oracle's interior-point loop where a row runs that algorithm, or a form the twin does not restate.
CASES maps every launched row to the case that launches it; UNREACHABLE lists the rows no configuration reaches, with the reason
tests/test_kernel_table.py checks on the CPU."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests.kkt_certificate import certify_batch, worst

MIXED = dict(pos_sigma=0.5, vel_sigma=1.0, quat_sigma=0.15)        # bench.py's `mixed` workload
AS_BAR, IPM_BAR, SENS_BAR, TWIN_BAR = 1e-9, 3e5, 1e-9, 1e-8
PREC_BOUND = {1: 1e-3, 2: 1.0, 3: 1e-3, 4: 1.0, 5: 0.3, 6: 0.3}    # include/ndp_nmpc.h, next to NDP_PREC_* (1 / 2: as 3 / 4)
EDGE_N = (2, 8, 9, 10, 18, 19, 20, 21, 27, 28, 31, 32, 37, 38, 40, 41, 42, 46)


def geometry(N):
    """(instances per workgroup, downwash fusable, row without downwash, row with it) of a default handle at horizon N, n_rti 1, fp64:
    ndp_create halves the waves from 4 while they need more than 160 KB of LDS, slots_for(N) = ceil((7N - 3) / 64), and the network
    runs inside the step when N + 1 <= 32, at most 3 slots and a workgroup slice of at least FR_TOTAL floats (tests/test_kernel_table.py
    derives the same table from the rules)."""
    if N <= 8:
        return 4, False, "K3_4", "K3_4"           # (the four-wave slice is smaller than the network's weights)
    if N <= 19:
        return 4, True, "K3_4", "K3F_4"
    if N == 20:
        return 4, True, "K20", "K20F"
    if N <= 27:
        return 2, True, "K3_2", "K3F_2"
    if N <= 41:
        return 2, False, "K5_2", "K5_2"
    return 1, False, "K5_1", "K5_1"


# rows no configuration launches, and why (tests/test_kernel_table.py checks each reason by arithmetic)
UNREACHABLE = {
    "K3F_1": "can_fuse needs a workgroup slice of FR_TOTAL floats: at one wave no N with at most 3 slots has one",
    "K5_4": "N with more than 3 slots needs more than 40 KB of LDS per instance: ndp_create never keeps 4 waves there",
}

# every other row -> the test that launches it and checks its result (the hook's mask is asserted inside)
CASES = {
    "K3_4": "test_horizon_sweep", "K20": "test_horizon_sweep", "K3_2": "test_horizon_sweep", "K5_2": "test_horizon_sweep",
    "K5_1": "test_horizon_sweep",
    "K3F_4": "test_edge_downwash_with_active_bounds", "K20F": "test_edge_downwash_with_active_bounds",
    "K3F_2": "test_edge_downwash_with_active_bounds",
    "K3_1": "test_rows_that_need_fewer_waves", "K20_W2": "test_rows_that_need_fewer_waves", "K20F_W2": "test_rows_that_need_fewer_waves",
    "SF_2": "test_sensitivities_at_two_waves", "S_2": "test_sensitivities_at_two_waves", "PF_2": "test_sensitivities_at_two_waves",
    "K20_PROD": "test_work_list_rows", "K20F_PROD": "test_work_list_rows", "K20_CONS": "test_work_list_rows",
    "K40_PROD": "test_edge_two_and_three_rti_iterations", "K40_CONS": "test_edge_two_and_three_rti_iterations",
    "K40": "test_config5_shape_in_place",
    "K20_LATE": "test_late_force_row",
    "K20F_TICK": "test_tick_rows", "K20_TICK": "test_tick_rows", "K20F_PROD_TICK": "test_tick_rows", "K20_PROD_TICK": "test_tick_rows",
    "KPREC1": "test_precision_study_rows", "KPREC2": "test_precision_study_rows", "KPREC3": "test_precision_study_rows",
    "KPREC4": "test_precision_study_rows", "KPREC5": "test_precision_study_rows", "KPREC6": "test_precision_study_rows",
    "K40_F32": "test_config5_precision_rows", "K40_BF16": "test_config5_precision_rows",
    "S20F_PROD": "test_n20_sensitivity_rows", "S20_PROD": "test_n20_sensitivity_rows", "S20_CONS": "test_n20_sensitivity_rows",
    "S20F": "test_n20_sensitivity_rows", "S20": "test_n20_sensitivity_rows",
    "SF_4": "test_four_wave_run_time_sensitivity_rows", "S_4": "test_four_wave_run_time_sensitivity_rows",
    "P20F_PROD": "test_n20_sensitivity_rows", "P20_PROD": "test_n20_sensitivity_rows", "P20_CONS": "test_n20_sensitivity_rows",
    "P20F": "test_n20_sensitivity_rows", "P20": "test_n20_sensitivity_rows", "PF_4": "test_four_wave_run_time_sensitivity_rows",
}


@pytest.fixture(scope="module")
def ndp():
    import ndp_nmpc_qd_amd
    return ndp_nmpc_qd_amd


def _rel(u, uo):
    return float(np.max(np.abs(u - uo) / np.maximum(1.0, np.abs(uo)))) if np.size(uo) else 0.0


def _launched(eng, rows, waves=None, fusable=None):
    got, w, fu = eng.debug_rti_launched()
    assert got == set(rows), (sorted(got), sorted(rows))
    if waves is not None:
        assert w == waves, (w, waves)
    if fusable is not None:
        assert fu == fusable, (fu, fusable)


def _twin_cfg(oracle, N, n_rti=1, use_fd=False, cfg=None):
    c = (cfg or oracle.default_cfg)(N=N, n_rti=n_rti, use_fd=use_fd)
    c.qp_mode = 0
    return c


def _against_twin(oracle, b, Xp, Up, acto, out, f=None, n_rti=1, tol=None, cfg=None, stats=None):
    """The step `out` = (u0, X, U, st, it, sw, act) of a device handle against the twin started from the same iterate and kept sets
    (acto is advanced in place); for one RTI iteration also the certificate of every status-0 instance.  Returns the number of
    instances the certificate flagged (a velocity within 1e-6 of its bound: held to the twin only).  cfg: what builds the oracle's
    cfg from (N, n_rti, use_fd) -- oracle.default_cfg unless the handle runs another model (tests/model_cases.py).  stats: a dict
    that keeps the largest figures seen (twin: |X, U - twin's| on set finishes; set / ipm: certificate residuals), for printing."""
    u0, X, U, st, it, sw, act = out
    N = b["xr"].shape[1] - 1
    Xo, Uo = Xp.copy(), Up.copy()
    _, sto, ito, swo = oracle.step_batch_as(_twin_cfg(oracle, N, n_rti, f is not None, cfg), b["x0"], b["xr"], b["ur"], f, Xo, Uo, acto)
    assert np.array_equal(st, sto) and np.array_equal(it, ito), (np.flatnonzero(st != sto), np.flatnonzero(it != ito))
    assert np.array_equal(sw, swo) and np.array_equal(act, acto), (np.flatnonzero(sw != swo),)
    a = it == 0                     # (an interior-point answer: 1e-6 on u0, test_interior_point_always_is_untouched's bar)

    def note(key, v):
        if stats is not None:
            stats[key] = max(stats.get(key, 0.0), float(v))
    note("twin", max(np.abs(X[a] - Xo[a]).max(initial=0.0), np.abs(U[a] - Uo[a]).max(initial=0.0)))
    np.testing.assert_allclose(X[a], Xo[a], rtol=0, atol=TWIN_BAR)
    np.testing.assert_allclose(U[a], Uo[a], rtol=0, atol=TWIN_BAR)
    assert _rel(U[~a][:, 0], Uo[~a][:, 0]) < 1e-6
    assert np.array_equal(u0, U[:, 0])
    if n_rti != 1:
        return 0
    i = np.flatnonzero(st == 0)
    ocfg = (cfg or oracle.default_cfg)(N=N, use_fd=f is not None)
    cs = certify_batch(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], None if f is None else f[i], Xp[i], Up[i], X[i], U[i])
    tol = ocfg.tol if tol is None else tol
    flagged = 0
    for j, c in zip(i, cs):
        if c["flag"]:
            flagged += 1
        elif it[j] == 0:
            note("set", worst(c))
            assert worst(c) <= AS_BAR, (N, j, worst(c))
        else:
            note("ipm", worst(c))
            assert worst(c) <= IPM_BAR * tol, (N, j, worst(c))
    return flagged


def _step(eng, b, downwash=False, f=None):
    """One host-array step with everything it returns: (u0, X, U, st, it, sweeps, kept set) and the force it used (or None)."""
    extra = dict(other=b["other"], ego_xy=b["ego_xy"]) if downwash else dict(f=f) if f is not None else {}
    u0, X, U, st, it = eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False, full=True, **extra)
    sw, act = eng.active_set()
    fo = eng.device_force().cpu().numpy().astype(np.float64) if downwash else f
    return (u0, X, U, st, it, sw, act), fo


def _ticks_against_twin(ndp, oracle, N, B, n_ticks, rows, seed, waves=None, fusable=None, downwash=False, n_rti=1, cfg=None, **eng_kw):
    """n_ticks steps of one handle (the kept sets carried) against the twin; asserts the rows launched.  Returns (flagged, the last
    step's outputs, its force, its batch).  cfg: as _against_twin's, for a handle whose eng_kw set another model (a dt among them
    also spaces the batch's reference windows)."""
    eng = ndp.BatchedNMPC(B, N=N, n_rti=n_rti, disturbance=downwash, **eng_kw)
    bkw = dict(MIXED, dt=eng_kw["dt"]) if "dt" in eng_kw else MIXED
    b = synth.make_batch(B, N=N, seed=seed, downwash=downwash, **bkw)
    eng.reset(b["xr"], b["ur"])
    Xp, Up = eng.get_iterate()
    acto = np.zeros((B, N, 4), dtype=np.int8)
    flagged = 0
    for t in range(n_ticks):
        b = synth.make_batch(B, N=N, seed=seed, downwash=downwash, t0=0.02 * t, **bkw)
        out, f = _step(eng, b, downwash)
        flagged += _against_twin(oracle, b, Xp, Up, acto, out, f, n_rti, cfg=cfg)
        Xp, Up = out[1], out[2]
    _launched(eng, rows, waves, fusable)
    eng.close()
    return flagged, out, f, b


# ---------------------------------------------------------------- a. every horizon
@pytest.mark.gpu
def test_horizon_sweep(ndp, oracle):
    """Every N the API accepts (2 .. 46), B = 257 (the last workgroup of a 2- or 4-wave launch is ragged), mixed workload, two ticks with
    the kept sets carried: device = twin on every instance and every status-0 instance certified; the handle's waves and the one row it
    launched are the table's.  N = 47 is refused."""
    B, flagged, active = 257, {}, 0
    for N in range(2, 47):
        waves, fusable, row, _ = geometry(N)
        flagged[N], out, _, _ = _ticks_against_twin(ndp, oracle, N, B, 2, {row}, synth.SEED0 + 300 + N, waves, fusable)
        active += int(out[6].any(axis=(1, 2)).sum())
    assert active > 0.05 * B * 45                      # inputs on their bounds, on average over the horizons
    print(f"instances flagged by the certificate (held to the twin only): {sum(flagged.values())} of {B * 2 * 45}",
          {N: n for N, n in flagged.items() if n})
    assert sum(flagged.values()) <= 0.05 * B * 2 * 45, flagged
    with pytest.raises(ndp.NdpError, match="2 <= N <= 46"):
        ndp.BatchedNMPC(4, N=47)


# ---------------------------------------------------------------- b. the horizons where the geometry changes
@pytest.mark.gpu
@pytest.mark.parametrize("N", EDGE_N)
def test_edge_downwash_with_active_bounds(ndp, oracle, mlp_blob, N):
    """Downwash on, mixed workload, two ticks: fused where fusable, else mlp_kernel and the unfused step.  The twin is given the device's
    own force; the force itself is held to the oracle's network (1e-5, the fp16-split layers' bar)."""
    waves, fusable, _, row = geometry(N)
    B = 61
    _, out, f, b = _ticks_against_twin(ndp, oracle, N, B, 2, {row}, synth.SEED0 + 400 + N, waves, fusable, downwash=True)
    fo = oracle.downwash_batch(mlp_blob, b["other"], b["xr"], b["ego_xy"])
    assert np.all(np.abs(f - fo) <= 1e-5 * np.maximum(1.0, np.abs(fo))), N
    assert 0 < (np.abs(fo).max(axis=(1, 2)) > 0).sum() < B          # gates open and shut in one batch


@pytest.mark.gpu
@pytest.mark.parametrize("N", EDGE_N)
def test_edge_interior_point_always(ndp, oracle, N):
    """qp_mode 1 at tol 1e-11 (every instance through the interior-point loop, the bounds read from LDS in the five-slot kernels) against
    the oracle's interior-point loop at the same tolerance (1e-6 on u0), and certified (3e5 tol)."""
    waves, fusable, row, _ = geometry(N)
    B, tol = 61, 1e-11
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 500 + N, **MIXED)
    eng = ndp.BatchedNMPC(B, N=N, qp_mode=1, tol=tol)
    eng.reset(b["xr"], b["ur"])
    u0, X, U, st, it = eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False, full=True)
    _launched(eng, {row}, waves, fusable)
    eng.close()
    cfg = oracle.default_cfg(N=N)
    cfg.tol = tol
    Xo, Uo = b["xr"].copy(), b["ur"].copy()
    uo, sto, _ = oracle.step_batch(cfg, b["x0"], b["xr"], b["ur"], None, Xo, Uo)
    ok = st == 0
    assert np.array_equal(st, sto) and ok.mean() > 0.9 and (it > 0).all()
    assert _rel(u0[ok], uo[ok]) < 1e-6, N
    i = np.flatnonzero(ok)
    cs = certify_batch(oracle, oracle.default_cfg(N=N), b["x0"][i], b["xr"][i], b["ur"][i], None, b["xr"][i], b["ur"][i], X[i], U[i])
    assert max(worst(c) for c in cs if not c["flag"]) <= IPM_BAR * tol, N


@pytest.mark.gpu
@pytest.mark.parametrize("N,n_rti", [(N, 2) for N in EDGE_N] + [(18, 3), (38, 3)])
def test_edge_two_and_three_rti_iterations(ndp, oracle, N, n_rti):
    """Two (three) RTI iterations per step, mixed workload: the twin restates the automatic rule per iteration (status, sweeps, sets
    identical, X and U within 1e-8).  N = 20 takes the run-time-horizon kernels (the compile-time ones are for one iteration), N = 40
    the work list's producer and consumer (config 5's shape)."""
    waves, fusable, row, _ = geometry(N)
    if N == 20:
        row = "K3_4"
    rows = {"K40_PROD", "K40_CONS"} if (N, n_rti) == (40, 2) else {row}
    _ticks_against_twin(ndp, oracle, N, 61, 1, rows, synth.SEED0 + 600 + N, waves, fusable, n_rti=n_rti)


# ---------------------------------------------------------------- c. ragged batches
@pytest.mark.gpu
@pytest.mark.parametrize("N,downwash,rows", [(13, False, {"K3_4"}), (24, True, {"K3F_2"}), (39, False, {"K5_2"}), (44, False, {"K5_1"})])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_ragged_batches_write_nothing_past_the_batch(ndp, oracle, N, downwash, rows, B):
    """B in {1, 3, 5}: the last workgroup has idle waves, which stage their share of the weights and meet every barrier but write
    nothing.  u0 goes to the first B rows of a NaN-filled buffer with 64 rows more: those stay bit-identical NaNs; u0 equals the
    host-array path's bit for bit; the iterate matches the twin."""
    import torch
    dev = torch.device("cuda", 0)
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 700 + N + B, downwash=downwash, **MIXED)
    d = {k: torch.from_numpy(v).to(dev) for k, v in b.items() if k in ("x0", "xr", "ur", "other", "ego_xy")}
    buf = torch.full((B + 64, 4), float("nan"), dtype=torch.float64, device=dev)
    bits0 = buf[B:].view(torch.int64).cpu().clone()
    eng = ndp.BatchedNMPC(B, N=N, disturbance=downwash)
    eng.reset(b["xr"], b["ur"])
    Xp, Up = eng.get_iterate()
    extra = dict(other=d["other"], ego_xy=d["ego_xy"]) if downwash else {}
    eng.update_device(d["x0"], d["xr"], d["ur"], buf[:B], **extra)
    eng.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(buf[B:].view(torch.int64).cpu(), bits0) and bool(torch.isnan(buf[B:]).all())
    u0 = buf[:B].cpu().numpy()
    X, U = eng.get_iterate()
    st, it = eng.status()
    sw, act = eng.active_set()
    f = eng.device_force().cpu().numpy().astype(np.float64) if downwash else None
    _launched(eng, rows)
    eng.close()
    host = ndp.BatchedNMPC(B, N=N, disturbance=downwash)
    host.reset(b["xr"], b["ur"])
    uh = host.update(b["x0"], b["xr"], b["ur"], raise_on_status=False, **({k: b[k] for k in ("other", "ego_xy")} if downwash else {}))
    _launched(host, rows)
    host.close()
    assert np.array_equal(u0, uh)
    _against_twin(oracle, b, Xp, Up, np.zeros((B, N, 4), dtype=np.int8), (u0, X, U, st, it, sw, act), f)


# ---------------------------------------------------------------- d. sensitivities at two waves
def _sens_case(ndp, oracle, b, level, params, fused, **eng_kw):
    """One step of a fresh handle with sensitivities on; every checked instance (40 seeded status-0 active-set instances and 8 with
    pinned inputs) against the dense fixed-set references.  Returns the handle's launched rows."""
    from tests.fixed_set_ref import psens_ref, scale, sens_ref
    B, N = b["x0"].shape[0], b["xr"].shape[1] - 1
    eng = ndp.BatchedNMPC(B, N=N, disturbance=fused, **eng_kw)
    eng.reset(b["xr"], b["ur"])
    Xp, Up = eng.get_iterate()
    eng.enable_sensitivity(level)
    if params:
        eng.enable_param_sensitivity()
    extra = dict(other=b["other"], ego_xy=b["ego_xy"]) if fused else {}
    u0, X, U, st, it = eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False, full=True, **extra)
    _, act = eng.active_set()
    du0, dU, dX = eng.sensitivity()
    ps = eng.param_sensitivity() if params else None
    f = eng.device_force().cpu().numpy().astype(np.float64) if fused else None
    rows = eng.debug_rti_launched()
    eng.close()
    idx = np.flatnonzero((st == 0) & (it == 0))
    pin = [i for i in idx if act[i].any()]
    assert idx.size >= 0.9 * B and len(pin) >= 8
    rng = np.random.default_rng(5)
    pick = sorted(set(rng.choice(idx, 40, replace=False).tolist()) | set(pin[:8]))
    cfg = oracle.default_cfg(N=N, use_fd=fused)
    w = 0.0
    for i in pick:
        fi = None if f is None else f[i]
        qp = oracle.linearize(cfg, b["x0"][i], b["xr"][i], b["ur"][i], fi, Xp[i], Up[i])
        r0, rU, rX = sens_ref(qp, act[i])
        s = scale(rU)
        w = max(w, np.max(np.abs(du0[i] - r0)) / s)
        if level == 2:
            w = max(w, np.max(np.abs(dU[i] - rU)) / s, np.max(np.abs(dX[i] - rX)) / max(1.0, np.max(np.abs(rX))))
        if params:
            ref = psens_ref(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], fi, Xp[i], Up[i], act[i])
            sp = max(scale(r) for r in ref)
            w = max(w, *(np.max(np.abs(g[i] - r)) / sp for g, r in zip(ps, ref)))
    assert w <= SENS_BAR, w
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("level,params,fused,row", [(2, False, True, "SF_2"), (2, False, False, "S_2"), (1, True, True, "PF_2")])
def test_sensitivities_at_two_waves(ndp, oracle, level, params, fused, row):
    """N = 24 (two instances per workgroup), mixed workload, B = 257: level-2 sensitivities fused and unfused, parameter sensitivities
    fused, against the dense references."""
    b = synth.make_batch(257, N=24, seed=synth.SEED0 + 800, downwash=fused, **MIXED)
    got, waves, fusable = _sens_case(ndp, oracle, b, level, params, fused)
    assert got == {row} and waves == 2 and fusable


@pytest.mark.gpu
@pytest.mark.parametrize("level,params,fused,row", [(2, False, True, "SF_4"), (2, False, False, "S_4"), (1, True, True, "PF_4")])
def test_four_wave_run_time_sensitivity_rows(ndp, oracle, level, params, fused, row):
    """The same at N = 13 (four instances per workgroup, run-time horizon)."""
    b = synth.make_batch(129, N=13, seed=synth.SEED0 + 810, downwash=fused, **MIXED)
    got, waves, _ = _sens_case(ndp, oracle, b, level, params, fused)
    assert got == {row} and waves == 4


@pytest.mark.gpu
@pytest.mark.parametrize("params", [False, True])
@pytest.mark.parametrize("fused,wq", [(True, 2), (False, 2), (True, 1), (False, 1)])
def test_n20_sensitivity_rows(ndp, oracle, params, fused, wq):
    """N = 20's sensitivity kernels: in place (S20F / S20, P20F / P20) and the work list's producer and consumer (S20F_PROD / S20_PROD +
    S20_CONS, and the P20 rows), level 1, against the dense references."""
    b = synth.make_batch(129, seed=synth.SEED0 + 820, downwash=fused, **MIXED)
    got, waves, _ = _sens_case(ndp, oracle, b, 1, params, fused, work_queue=wq)
    p = "P" if params else "S"
    want = {f"{p}20F" if fused else f"{p}20"} if wq == 2 else {f"{p}20F_PROD" if fused else f"{p}20_PROD", f"{p}20_CONS"}
    assert got == want and waves == 4


# ---------------------------------------------------------------- e. rows that need NDP_DEV_WAVES
@pytest.mark.gpu
@pytest.mark.parametrize("N,waves,downwash,row", [(20, 2, False, "K20_W2"), (20, 2, True, "K20F_W2"), (13, 1, False, "K3_1"),
                                                  (27, 1, False, "K3_1"), (13, 1, True, "K3_1"), (27, 1, True, "K3_1")])
def test_rows_that_need_fewer_waves(ndp, oracle, mlp_blob, monkeypatch, N, waves, downwash, row):
    """NDP_DEV_WAVES (read by ndp_create) lowers the instances per workgroup: the same program at another launch geometry.  Against the
    twin and the certificate, and bit-equal with the default launch of the same inputs.  At one wave the downwash cannot be fused
    (K3F_1 is not launched): the force comes from mlp_kernel, whose rounding differs from the fused tile's -- there the step is held
    to the twin given that force, and the force to the oracle's network."""
    B = 61
    monkeypatch.setenv("NDP_DEV_WAVES", str(waves))
    _, out, f, b = _ticks_against_twin(ndp, oracle, N, B, 2, {row}, synth.SEED0 + 900 + N, waves, waves == 2, downwash=downwash)
    monkeypatch.delenv("NDP_DEV_WAVES")
    dflt_waves, _, plain, fused_row = geometry(N)
    _, ref, fr, _ = _ticks_against_twin(ndp, oracle, N, B, 2, {fused_row if downwash else plain}, synth.SEED0 + 900 + N, dflt_waves,
                                        downwash=downwash)
    if downwash and waves == 1:
        fo = oracle.downwash_batch(mlp_blob, b["other"], b["xr"], b["ego_xy"])
        assert np.all(np.abs(f - fo) <= 1e-5 * np.maximum(1.0, np.abs(fo)))
        return
    for a, c in zip(out, ref):
        assert np.array_equal(a, c)
    if downwash:
        assert np.array_equal(f, fr)


# ---------------------------------------------------------------- f. every other row
@pytest.mark.gpu
@pytest.mark.parametrize("downwash", [False, True])
def test_work_list_rows(ndp, oracle, downwash):
    """N = 20, the work list forced on: producer (K20_PROD / K20F_PROD) and consumer (K20_CONS) against the twin, two ticks."""
    _ticks_against_twin(ndp, oracle, 20, 257, 2, {"K20F_PROD" if downwash else "K20_PROD", "K20_CONS"}, synth.SEED0 + 1000,
                        4, True, downwash=downwash, work_queue=1)


@pytest.mark.gpu
def test_config5_shape_in_place(ndp, oracle):
    """N = 40, two RTI iterations, the work list off: config 5's compile-time in-place kernel (K40) against the twin."""
    _ticks_against_twin(ndp, oracle, 40, 61, 2, {"K40"}, synth.SEED0 + 1010, 2, False, n_rti=2, work_queue=2)


@pytest.mark.gpu
def test_late_force_row(ndp, oracle, mlp_blob):
    """The downwash one tick ahead: the late-force step (K20_LATE) takes a force a second launch predicted, against the oracle fed the
    oracle's network (1e-6, test_downwash_one_tick_ahead_on_the_second_stream's bar)."""
    import torch
    B = 61
    dev = torch.device("cuda", 0)
    b = synth.make_batch(B, seed=synth.SEED0 + 1020, downwash=True)
    d = {k: torch.from_numpy(b[k]).to(dev) for k in ("x0", "xr", "ur", "other", "ego_xy")}
    eng = ndp.BatchedNMPC(B, disturbance=True)
    u0 = torch.empty(B, 4, dtype=torch.float64, device=dev)
    eng.reset(b["xr"], b["ur"])
    torch.cuda.synchronize()
    eng.downwash_prefetch_device(d["other"], d["xr"], ego_xy=d["ego_xy"])
    eng.update_device_prefetched(d["x0"], d["xr"], d["ur"], u0)
    eng.prefetch_join()
    eng.synchronize()
    torch.cuda.synchronize()
    st, _ = eng.status()
    _launched(eng, {"K20_LATE"}, 4, True)
    eng.close()
    f0 = oracle.downwash_batch(mlp_blob, b["other"], b["xr"], b["ego_xy"])
    Xo, Uo = b["xr"].copy(), b["ur"].copy()
    uo, sto, _ = oracle.step_batch(oracle.default_cfg(use_fd=True), b["x0"], b["xr"], b["ur"], f0, Xo, Uo)
    assert not st.any() and not sto.any()
    assert _rel(u0.cpu().numpy(), uo) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("neighbours", [True, False])
@pytest.mark.parametrize("wq", [2, 1])
def test_tick_rows(ndp, oracle, mlp_blob, neighbours, wq):
    """The one-launch control tick (list advance, estimator and step in one kernel), in place and as the work list's producer, with and
    without neighbours: three ticks against the oracle (smoke()'s bar, 1e-5)."""
    B = 16
    tr = synth.figure_eight_traj(B, seed=2, n_seg=16, t_seg=0.25, pairs=True)
    tk = ndp.BatchedNMPC(B, disturbance=neighbours, work_queue=wq)
    tk.ref_set_trajectory(tr["coeff_x"], tr["coeff_y"], tr["coeff_z"], tr["coeff_yaw"], tr["time_cum"], tr["time_seg"], tr["final_pt"])
    tk.ref_list_reset()
    oi = np.arange(B, dtype=np.int32) ^ 1
    if neighbours:
        tk.tick_config(oi, gate=True)
    tk.tick_reset()
    Xo, Uo = tk.get_iterate()
    cfg = oracle.default_cfg(use_fd=neighbours)
    err = 0.0
    for i in range(3):
        x0 = tk.ref_list_window(None)[0][:, 0, :].copy()
        x0[:, 0:3] += 0.05
        _, u0t, st, _ = tk.tick(x0, t=0.02 * (i + 1), full=True)
        xr, ur = tk.ref_list_window(None)
        ft = oracle.downwash_batch(mlp_blob, xr[oi].copy(), xr, x0[:, 0:2].copy()) if neighbours else None
        u_or, st_o, _ = oracle.step_batch(cfg, x0, xr, ur, ft, Xo, Uo)
        assert not st.any() and not st_o.any()
        err = max(err, _rel(u0t, u_or))
    assert err <= 1e-5, err
    row = ("K20F" if neighbours else "K20") + ("_PROD_TICK" if wq == 1 else "_TICK")
    _launched(tk, {row} | ({"K20_CONS"} if wq == 1 else set()), 4, True)
    tk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [1, 2, 3, 4, 5, 6])
def test_precision_study_rows(ndp, oracle, prec):
    """qp_precision 1 .. 6 at N = 20 (one instance per workgroup, whatever the handle's waves): every status-0 step within its mode's
    certificate bound, nominal starts."""
    B = 61
    b = synth.make_batch(B, seed=synth.SEED0 + 1030)
    eng = ndp.BatchedNMPC(B, qp_precision=prec)
    eng.reset(b["xr"], b["ur"])
    Xp, Up = eng.get_iterate()
    _, X, U, st, it = eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False, full=True)
    _launched(eng, {f"KPREC{prec}"})
    eng.close()
    ok = np.flatnonzero(st == 0)
    assert ok.size >= 0.9 * B
    cs = certify_batch(oracle, oracle.default_cfg(), b["x0"][ok], b["xr"][ok], b["ur"][ok], None, Xp[ok], Up[ok], X[ok], U[ok])
    assert not any(c["flag"] for c in cs)
    assert max(worst(c) for c in cs) <= PREC_BOUND[prec], prec


@pytest.mark.gpu
@pytest.mark.parametrize("prec,row,lo,hi", [(3, "K40_F32", 0.0, 1e-5), (4, "K40_BF16", 1e-4, 0.5)])
def test_config5_precision_rows(ndp, oracle, prec, row, lo, hi):
    """Config 5's own shape (N = 40, two RTI iterations, two instances per workgroup) on the fp32 / bf16 matrix instructions, nominal
    starts, against the oracle (test_config5_qp_on_the_fp32_and_bf16_matrix_instructions' bars)."""
    B = 61
    b = synth.make_batch(B, N=40, seed=20231213 + 5)
    eng = ndp.BatchedNMPC(B, N=40, n_rti=2, qp_precision=prec)
    eng.reset(b["xr"], b["ur"])
    u0 = eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False)
    st, _ = eng.status()
    _launched(eng, {row}, 2)
    eng.close()
    Xo, Uo = b["xr"].copy(), b["ur"].copy()
    uo, sto, _ = oracle.step_batch(oracle.default_cfg(N=40, n_rti=2), b["x0"], b["xr"], b["ur"], None, Xo, Uo)
    assert not st.any() and not sto.any()
    assert lo <= _rel(u0, uo) < hi
