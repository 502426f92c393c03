"""The formation rollout on the device: plant_force_kernel against the public network call (bit for bit) and the oracle, the rollout
against its own composition from the host (bit for bit), the physics against the CPU reference loop (tests/formation_ref.py), and the
refusals."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from ndp_nmpc_qd_amd.params import downwash_params as DP
from ndp_nmpc_qd_amd.params import nmpc_params as CP
from tests import formation_ref as F

pytestmark = pytest.mark.gpu

# Device rollout against the CPU reference loop, logged positions over all 200 ticks, both controllers, dz = 0.5 and 1.0.
# Expected from the project's own numbers: the network bar (1e-5 N) times the blind controller's closed-loop gain (0.33 m per 4.4 N =
# 0.075 m/N) = about 1e-6 m; above 1e-5 m something other than fp32 rounding would differ.  POS_MEASURED is the worst absolute
# difference of the first device run (NDP at dz = 0.5; NMPC 8.8e-8, dz = 1.0: 1.3e-7 / 1.5e-7; the forces differed by at most 5.7e-6 N),
# POS_BAR ten times that (DESIGN.md section 9 records both).
POS_MEASURED = 2.17e-7
POS_BAR = 10 * POS_MEASURED


def _states(B, rng):
    """Plant states whose pairwise differences lie inside the network's training envelope (|dxy| <= 1.5 m, |dz| <= 1 m, |dv| ~ 1 m/s)."""
    x = np.zeros((B, 10))
    x[:, 0:2] = rng.uniform(-0.75, 0.75, (B, 2))
    x[:, 2] = rng.uniform(0.5, 1.5, B)
    x[:, 3:6] = rng.normal(0, 0.5, (B, 3))
    q = rng.normal(0, 0.1, (B, 4)) + np.array([1.0, 0, 0, 0])
    x[:, 6:10] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return x


def _via_downwash(eng, x, idx, gate):
    """Row 0 of ndp_downwash on windows made by repeating x[idx] and x along the horizon (ego_xy = x[:, :2]); 0 where idx < 0."""
    B = x.shape[0]
    o = np.where(idx >= 0, idx, np.arange(B))
    other = np.ascontiguousarray(np.repeat(x[o][:, None, :], eng.N + 1, axis=1))
    ego = np.ascontiguousarray(np.repeat(x[:, None, :], eng.N + 1, axis=1))
    f = eng.downwash(other, ego, np.ascontiguousarray(x[:, 0:2]) if gate else None)
    assert np.array_equal(f, np.repeat(f[:, :1], eng.N + 1, axis=1))
    return np.where((idx >= 0)[:, None], f[:, 0, :].astype(np.float64), 0.0)


@pytest.mark.parametrize("B", [1, 2, 31, 32, 33, 129, 257])
def test_plant_force_equals_the_public_network_call_bit_for_bit(B):
    import torch
    import ndp_nmpc_qd_amd as ndp
    rng = np.random.default_rng(100 + B)
    eng = ndp.BatchedNMPC(B, load_mlp=True)
    x = _states(B, rng)
    perm = rng.permutation(B).astype(np.int32)
    mixed = perm.copy()
    mixed[rng.permutation(B)[:B // 3]] = -1
    cases = {"none": np.full(B, -1, np.int32), "perm": perm, "mixed": mixed, "self": np.arange(B, dtype=np.int32),
             "far": ((np.arange(B) + 128) % B).astype(np.int32)}              # (B = 257: the neighbour sits in another workgroup)
    seen_open = seen_closed = 0
    for name, idx in cases.items():
        for gate in (True, False):
            want = _via_downwash(eng, x, idx, gate)
            got = eng.plant_force(x, idx, gate=gate)
            assert got.dtype == np.float64 and np.array_equal(got, want), (name, gate, np.abs(got - want).max())
            seen_open += int(np.any(want != 0.0)); seen_closed += int(np.any((want == 0.0).all(axis=1) & (idx >= 0)))
    if B > 2:
        assert seen_open and seen_closed                                     # the states exercise both sides of the gate
    # self index: the input is exactly 0, the force net(0) -- the same for every vehicle, and not 0
    f_self = eng.plant_force(x, cases["self"])
    assert np.array_equal(f_self, np.repeat(f_self[:1], B, axis=0)) and np.any(f_self != 0.0)
    # scale multiplies the fp64 value
    assert np.array_equal(eng.plant_force(x, mixed, gate=False, scale=0.7), 0.7 * _via_downwash(eng, x, mixed, False))
    # no index at all: zeros, and the device form still writes xy; with an index the device form equals the host form
    assert np.array_equal(eng.plant_force(x, None), np.zeros((B, 3)))
    dev = torch.device("cuda", 0)
    xd, fd, xyd = torch.from_numpy(x).to(dev), torch.full((B, 3), 7.0, dtype=torch.float64, device=dev), torch.full((B, 2), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.plant_force_device(xd, None, fd, xy_out=xyd)
    eng.synchronize()
    assert np.array_equal(fd.cpu().numpy(), np.zeros((B, 3))) and np.array_equal(xyd.cpu().numpy(), x[:, 0:2])
    xyd.fill_(7.0)
    torch.cuda.synchronize()
    eng.plant_force_device(xd, torch.from_numpy(mixed).to(dev), fd, xy_out=xyd, scale=1.3)
    eng.synchronize()
    assert np.array_equal(fd.cpu().numpy(), eng.plant_force(x, mixed, scale=1.3)) and np.array_equal(xyd.cpu().numpy(), x[:, 0:2])


def test_plant_force_gate_is_strict_at_the_rim():
    """distance^2 == r_horiz^2 exactly: closed; one ulp inside: open; gate=False: open everywhere."""
    import ndp_nmpc_qd_amd as ndp
    B = 6
    eng = ndp.BatchedNMPC(B, load_mlp=True)
    x = _states(B, np.random.default_rng(5))
    r = DP.r_horiz
    assert r == 1.0
    x[0, 0:3], x[1, 0:3] = (0.25, -0.5, 1.0), (0.25 + r, -0.5, 1.5)                       # on the rim: dx = r exactly, dy = 0
    x[2, 0:3], x[3, 0:3] = (0.25, 0.5, 1.0), (np.nextafter(0.25 + r, 0.0), 0.5, 1.5)      # one ulp inside
    x[4, 0:3], x[5, 0:3] = (-0.5, 0.0, 1.0), (-0.5, 0.25, 1.5)                            # well inside
    assert (x[1, 0] - x[0, 0]) ** 2 == r * r and (x[3, 0] - x[2, 0]) ** 2 < r * r
    idx = np.arange(B, dtype=np.int32) ^ 1
    f = eng.plant_force(x, idx, gate=True)
    assert np.array_equal(f[0:2], np.zeros((2, 3))) and np.all(np.any(f[2:] != 0.0, axis=1))
    assert np.array_equal(f, _via_downwash(eng, x, idx, True))
    f_open = eng.plant_force(x, idx, gate=False)
    assert np.all(np.any(f_open != 0.0, axis=1)) and np.array_equal(f_open[2:], f[2:])
    assert np.array_equal(f_open, _via_downwash(eng, x, idx, False))


def test_plant_force_against_the_oracle_network(oracle, mlp_blob):
    """257 random relative states inside the training envelope against oracle.mlp_forward on the same fp32 inputs, within the
    project's network bar (1e-5, relative above 1 N: test_downwash_mlp_against_reference_fixture)."""
    import ndp_nmpc_qd_amd as ndp
    B = 257
    rng = np.random.default_rng(11)
    eng = ndp.BatchedNMPC(B, load_mlp=True)
    x = _states(B, rng)
    idx = np.roll(rng.permutation(B), 1).astype(np.int32)
    z = (x[idx] - x)[:, 0:6].astype(np.float32)
    want = oracle.mlp_forward(mlp_blob, z).astype(np.float64)
    got = eng.plant_force(x, idx, gate=False)
    err = np.abs(got - want)
    print(f"plant force against the oracle: max |diff| {err.max():.3e} N, max |f| {np.abs(want).max():.2f} N")
    assert np.abs(want).max() > 1.0
    assert np.all(err <= 1e-5 * np.maximum(1.0, np.abs(want))), err.max()


def _host_composition(eng, tr, x_init, ticks, t0, compensate, scale):
    """ref_window -> plant_force -> update -> plant_step made tick by tick from the host; -> states, u0, force, status per tick."""
    import torch
    B = eng.B
    idx = tr["other_index"]
    dev = torch.device("cuda", 0)
    idx_t = torch.from_numpy(idx).to(dev)
    u0_t = torch.empty(B, 4, dtype=torch.float64, device=dev)
    xr0, ur0 = eng.ref_window(np.full(B, t0))
    eng.reset(xr0, ur0)
    xs = x_init.copy()
    out = ([], [], [], [])
    for k in range(ticks):
        xr, ur = eng.ref_window(np.full(B, t0 + k * CP.ts_nmpc))
        f = eng.plant_force(xs, idx, gate=True, scale=scale)
        if compensate:
            xt, xrt, urt, xyt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xs, xr, ur, xs[:, 0:2]))
            torch.cuda.synchronize()
            eng.update_device(xt, xrt, urt, u0_t, other=xrt, ego_xy=xyt, other_index=idx_t)
            eng.synchronize()
            u0 = u0_t.cpu().numpy()
        else:
            u0 = eng.update(xs, xr, ur, raise_on_status=False)
        st = eng.status()[0].copy()
        xs = eng.plant_step(xs, u0, f, CP.ts_nmpc, 4)
        for o, v in zip(out, (xs.copy(), u0.copy(), f, st)):
            o.append(v)
    return tuple(np.stack(o) for o in out)


def _device_rollout(eng, x_init, idx, ticks, t0=0.0, **kw):
    import torch
    B = eng.B
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(x_init).to(dev)
    idx_t = None if idx is None else torch.from_numpy(idx).to(dev)
    log, log_u, log_f = (torch.empty(ticks, B, n, dtype=torch.float64, device=dev) for n in (10, 4, 3))
    worst = torch.full((B,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.rollout_formation_device(ticks, xd, idx_t, log=log, log_u=log_u, log_f=log_f, worst_status=worst, t0=t0, **kw)
    eng.synchronize()
    return xd.cpu().numpy(), log.cpu().numpy(), log_u.cpu().numpy(), log_f.cpu().numpy(), worst.cpu().numpy()


@pytest.mark.parametrize("compensate", [True, False])
def test_rollout_equals_its_host_composition_bit_for_bit(compensate):
    """B = 66: 33 pairs, so a pair straddles the 32-vehicle tile; 40 ticks; plant_scale 1.3 so that the scale travels too."""
    import ndp_nmpc_qd_amd as ndp
    P, K, t0, scale = 33, 40, 0.4, 1.3
    tr = F.workload(P, dz=0.5, seed=21)
    B = 2 * P
    engs = [ndp.BatchedNMPC(B, disturbance=compensate, load_mlp=True) for _ in range(2)]
    for e in engs:
        F.set_trajectory(e, tr)
    assert engs[0].disturbance == compensate                                  # (compensate=None below: the handle's own default)
    x_init = engs[0].ref_window(np.full(B, t0))[0][:, 0].copy()
    x_init[:, 0:3] += np.random.default_rng(9).normal(0, 0.03, (B, 3))
    states, u0s, fs, sts = _host_composition(engs[0], tr, x_init, K, t0, compensate, scale)
    x_end, log, log_u, log_f, worst = _device_rollout(engs[1], x_init, tr["other_index"], K, t0=t0, plant_scale=scale)
    assert np.abs(fs[:, 0::2, 2]).max() > 1.0                                 # the lower vehicles do fly through newtons of downwash
    assert np.array_equal(log_f, fs)
    assert np.array_equal(log_u, u0s)
    assert np.array_equal(log, states) and np.array_equal(x_end, states[-1])
    assert np.array_equal(worst, sts.max(axis=0))
    # the logs are optional: without them the same final state
    import torch
    xd = torch.from_numpy(x_init).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    engs[1].rollout_formation_device(K, xd, torch.from_numpy(tr["other_index"]).to(xd.device), t0=t0, plant_scale=scale)
    engs[1].synchronize()
    assert np.array_equal(xd.cpu().numpy(), states[-1])


def test_rollout_with_nobody_nearby_is_the_plain_rollout():
    """other_index all -1 (and None): the states are rollout_device's on the same kind of handle, bit for bit; the force log is 0."""
    import torch
    import ndp_nmpc_qd_amd as ndp
    P, K, t0 = 33, 40, 0.4
    tr = F.workload(P, dz=0.5, seed=22)
    B = 2 * P
    engs = [ndp.BatchedNMPC(B, load_mlp=True) for _ in range(3)]
    for e in engs:
        F.set_trajectory(e, tr)
    x_init = engs[0].ref_window(np.full(B, t0))[0][:, 0].copy()
    x_init[:, 0:3] += np.random.default_rng(10).normal(0, 0.03, (B, 3))
    dev = torch.device("cuda", 0)
    xd, log0 = torch.from_numpy(x_init).to(dev), torch.empty(K, B, 10, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    engs[0].rollout_device(K, xd, log0, t0=t0)
    engs[0].synchronize()
    for e, idx in ((engs[1], np.full(B, -1, np.int32)), (engs[2], None)):
        x_end, log, _, log_f, worst = _device_rollout(e, x_init, idx, K, t0=t0)
        assert np.array_equal(log, log0.cpu().numpy()) and np.array_equal(x_end, xd.cpu().numpy())
        assert not log_f.any() and not worst.any()


@pytest.mark.parametrize("dz", [0.5, 1.0])
def test_device_rollout_reproduces_the_downwash_effect(oracle, dz):
    """Test 1's workload on the device: the lower vehicle's NDP z-RMSE is at most a fifth of its NMPC z-RMSE, every status is 0, and
    states and RMSEs agree with the CPU reference loop within POS_BAR (the RMSE is 1-Lipschitz in the positions)."""
    import ndp_nmpc_qd_amd as ndp
    r = F.reference(dz)
    tr, B = r["tr"], 2 * F.PAIRS
    x_init = r["xr"][0][:, 0].copy()
    rmse = {}
    for name, comp in (("nmpc", False), ("ndp", True)):
        eng = ndp.BatchedNMPC(B, disturbance=comp, load_mlp=True)
        F.set_trajectory(eng, tr)
        _, log, _, log_f, worst = _device_rollout(eng, x_init, tr["other_index"], F.TICKS)
        assert not worst.any()
        cpu_states, _, cpu_f, _ = r[name]
        dpos = np.abs(log[:, :, 0:3] - cpu_states[:, :, 0:3]).max()
        rmse[name] = F.z_rmse(log, r["xr"])
        drmse = np.abs(rmse[name] - F.z_rmse(cpu_states, r["xr"])).max()
        print(f"dz {dz} {name}: max |position - CPU loop| {dpos:.3e} m, max |force - CPU loop| {np.abs(log_f - cpu_f).max():.3e} N, "
              f"max |z-RMSE - CPU loop| {drmse:.3e} m, lower z-RMSE {rmse[name][0::2]}, upper {rmse[name][1::2]}")
        assert dpos <= POS_BAR, dpos
        assert drmse <= POS_BAR, drmse
        d = log[:, 0::2, 0:2] - log[:, 1::2, 0:2]
        assert np.sqrt((d * d).sum(-1)).max() < 0.5 * DP.r_horiz             # no gate anywhere near flipping
    assert np.all(rmse["ndp"][0::2] <= rmse["nmpc"][0::2] / 5.0), (rmse["ndp"][0::2], rmse["nmpc"][0::2])


@pytest.mark.parametrize("case", ["compensate_on_nmpc_handle", "no_weights", "no_trajectory", "sensitivity_handle"])
def test_rollout_refusals_leave_the_handle_usable(case):
    import torch
    import ndp_nmpc_qd_amd as ndp
    B = 4
    tr = F.workload(B // 2, dz=0.5)
    kw = dict(compensate_on_nmpc_handle=dict(load_mlp=True), no_weights=dict(disturbance=True, load_mlp=False),
              no_trajectory=dict(load_mlp=True), sensitivity_handle=dict(load_mlp=True))[case]
    reason = dict(compensate_on_nmpc_handle="NDP_FORM_COMPENSATE needs use_fd = 1", no_weights="ndp_set_mlp_weights was never called",
                  no_trajectory="ndp_ref_set_trajectory was never called", sensitivity_handle="sensitivities are enabled")[case]

    def make():
        e = ndp.BatchedNMPC(B, **kw)
        if case != "no_trajectory":
            F.set_trajectory(e, tr)
        if case == "sensitivity_handle":
            e.enable_sensitivity(1)
        return e
    eng, fresh = make(), make()
    dev = torch.device("cuda", 0)
    b = synth.make_batch(B, seed=3)
    xd, idx = torch.from_numpy(b["x0"]).to(dev), torch.from_numpy(tr["other_index"]).to(dev)
    torch.cuda.synchronize()
    with pytest.raises(ndp.NdpError, match=reason) as ei:
        eng.rollout_formation_device(5, xd, idx, compensate=True if case == "compensate_on_nmpc_handle" else None)
    assert ("(-2)" if case == "sensitivity_handle" else "(-8)") in str(ei.value)
    eng.synchronize()
    assert np.array_equal(xd.cpu().numpy(), b["x0"])                          # nothing was enqueued
    for e in (eng, fresh):
        e.reset(b["xr"], b["ur"])
    assert np.array_equal(eng.update(b["x0"], b["xr"], b["ur"]), fresh.update(b["x0"], b["xr"], b["ur"]))
