"""Downwash from several neighbours on the device: mlp_multi_kernel (the controller's prediction) and plant_force_multi_kernel (the force
on the plant) against the slot-ordered sum of K single-neighbour calls (bit for bit), against the oracle network (the project's bar,
once per slot), at the gate's rim per slot, and the refusals."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from ndp_nmpc_qd_amd.params import downwash_params as DP

pytestmark = pytest.mark.gpu

R2 = DP.r_horiz ** 2
KS = [1, 2, 3, 8]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _index_cases(B, K, rng):
    """int32[B, K] index sets: nobody, a permutation per slot, a third of the entries empty, one neighbour in two slots, oneself."""
    perm = np.stack([rng.permutation(B) for _ in range(K)], axis=1).astype(np.int32)
    mixed = perm.copy()
    flat = rng.permutation(B * K)[:(B * K + 2) // 3]
    mixed.reshape(-1)[flat] = -1
    dup = perm.copy()
    dup[:, K - 1] = dup[:, 0]                                                 # (K = 1: the permutation itself)
    return {"none": np.full((B, K), -1, np.int32), "perm": perm, "mixed": mixed, "dup": dup,
            "self": np.repeat(np.arange(B, dtype=np.int32)[:, None], K, axis=1)}


# ------------------------------------------------------------------------------------------------ the controller's prediction
def _windows(B, N, rng):
    """Neighbour windows other[B, N+1, 10], ego windows ego_ref[B, N+1, 10] and ego odometry ego_xy[B, 2]: differences inside the
    network's training envelope (|dxy| <= 1.5 m, dz 0.3 .. 1 m, |dv| ~ 1 m/s); node-0 distances on both sides of r_horiz."""
    def win(z0):
        w = np.zeros((B, N + 1, 10))
        p0 = np.concatenate([rng.uniform(-0.75, 0.75, (B, 2)), z0], axis=1)
        v = rng.normal(0, 0.4, (B, 3))
        t = 0.1 * np.arange(N + 1)[None, :, None]
        w[:, :, 0:3] = p0[:, None, :] + 0.2 * v[:, None, :] * t
        w[:, :, 3:6] = v[:, None, :] + rng.normal(0, 0.05, (B, N + 1, 3))
        w[:, :, 6] = 1.0
        return w
    ego = win(rng.uniform(0.5, 0.8, (B, 1)))
    other = win(rng.uniform(1.1, 1.5, (B, 1)))
    ego_xy = ego[:, 0, 0:2] + rng.normal(0, 0.02, (B, 2))
    return other, ego, np.ascontiguousarray(ego_xy)


def _slot_open(other, idx1, ego_xy):
    """The gate of one slot as the kernels evaluate it: individually rounded, strict."""
    o = np.where(idx1 >= 0, idx1, 0)
    if ego_xy is None:
        return idx1 >= 0
    dx, dy = other[o, 0, 0] - ego_xy[:, 0], other[o, 0, 1] - ego_xy[:, 1]
    return (idx1 >= 0) & (dx * dx + dy * dy < R2)


def _slots_single(eng, other, idx, ego, ego_xy):
    """Per slot, ndp_downwash_device on the gathered windows, zeros for an empty slot: list of float32 [B, N+1, 3]."""
    import torch
    B, N = eng.B, eng.N
    et, xyt = _t(ego), None if ego_xy is None else _t(ego_xy)
    out = []
    for k in range(idx.shape[1]):
        o = np.where(idx[:, k] >= 0, idx[:, k], 0)
        g = np.zeros((B, N + 1, 10))
        g[:, :, :other.shape[2]] = other[o]
        f = torch.empty(B, N + 1, 3, dtype=torch.float32, device=_dev())
        torch.cuda.synchronize()
        eng.downwash_device(_t(g), et, f, ego_xy=xyt)
        eng.synchronize()
        out.append(np.where((idx[:, k] >= 0)[:, None, None], f.cpu().numpy(), np.float32(0.0)).astype(np.float32))
    return out


def _sum32(parts):
    acc = parts[0]
    for p in parts[1:]:
        acc = (acc + p).astype(np.float32)
    return acc


def _multi_device(eng, other, idx, ego, ego_xy):
    """downwash_multi_device into the front of a longer buffer: (f [B, N+1, 3], the untouched tail)."""
    import torch
    n = eng.B * (eng.N + 1) * 3
    buf = torch.full((n + 96,), 7.0, dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    eng.downwash_multi_device(_t(other), _t(idx), _t(ego), buf[:n].view(eng.B, eng.N + 1, 3), ego_xy=None if ego_xy is None else _t(ego_xy))
    eng.synchronize()
    out = buf.cpu().numpy()
    return out[:n].reshape(eng.B, eng.N + 1, 3).copy(), out[n:]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N,B", [(20, 1), (20, 5), (20, 7), (20, 49), (13, 5)])
def test_prediction_equals_the_slot_ordered_sum_of_single_calls(oracle, mlp_blob, N, B, K):
    """B = 1: one tile; 5: a partial last tile; 7: a second workgroup with one wave; 49, and N = 13: instance boundaries inside tiles."""
    import ndp_nmpc_qd_amd as ndp
    rng = np.random.default_rng(1000 * N + 10 * B + K)
    eng = ndp.BatchedNMPC(B, N=N, load_mlp=True)
    other, ego, ego_xy = _windows(B, N, rng)
    mixed_gate = False
    worst = 0.0
    for name, idx in _index_cases(B, K, rng).items():
        for xy in (ego_xy, None):
            for stride in (10, 6):
                oth = np.ascontiguousarray(other[:, :, :stride])
                parts = _slots_single(eng, oth, idx, ego, xy)
                got, tail = _multi_device(eng, oth, idx, ego, xy)
                assert got.dtype == np.float32 and np.array_equal(got, _sum32(parts)), (name, xy is None, stride)
                assert np.all(tail == 7.0)                                    # nothing behind the last row is written
                if K == 1:
                    assert np.array_equal(got, parts[0])
            opens = np.stack([_slot_open(other, idx[:, k], xy) for k in range(K)], axis=1)
            if xy is not None:                                                # (among the slots that do hold a neighbour)
                mixed_gate |= bool(np.any(opens.any(axis=1) & ((idx >= 0) & ~opens).any(axis=1)))
            # against the oracle network summed in float64 over the open slots: the project's bar, once per slot
            want, fmax = np.zeros((B, N + 1, 3)), np.zeros((B, N + 1, 3))
            for k in range(K):
                o = np.where(idx[:, k] >= 0, idx[:, k], 0)
                z = (other[o] - ego)[:, :, 0:6].astype(np.float32)
                fk = oracle.mlp_forward(mlp_blob, z).astype(np.float64).reshape(B, N + 1, 3) * opens[:, k][:, None, None]
                want += fk
                fmax = np.maximum(fmax, np.abs(fk))
            err = np.abs(got - want)
            worst = max(worst, float((err / np.maximum(1.0, fmax)).max()))
            assert np.all(err <= K * 1e-5 * np.maximum(1.0, fmax)), (name, err.max())
    print(f"N {N} B {B} K {K}: max |prediction - oracle| / max(1, max_k |f_k|) = {worst:.3e} (bar {K}e-5)")
    if B > 2 and K > 1:
        assert mixed_gate                                                     # open and closed slots met in one instance
    # the host form is the device form
    idx = _index_cases(B, K, rng)["mixed"]
    assert np.array_equal(eng.downwash_multi(other, idx, ego, ego_xy), _multi_device(eng, other, idx, ego, ego_xy)[0])


def test_prediction_gate_is_strict_at_the_rim_per_slot():
    """distance^2 == r_horiz^2 exactly: that slot is closed; one ulp inside: open -- with the instance's other slot on the opposite side."""
    import ndp_nmpc_qd_amd as ndp
    B, N = 4, 20
    eng = ndp.BatchedNMPC(B, N=N, load_mlp=True)
    other, ego, ego_xy = _windows(B, N, np.random.default_rng(3))
    r = DP.r_horiz
    assert r == 1.0
    ego_xy[:] = (0.25, -0.5)
    other[0, 0, 0:2] = (0.25 + r, -0.5)                                       # on the rim: dx = r exactly, dy = 0
    other[1, 0, 0:2] = (np.nextafter(0.25 + r, 0.0), -0.5)                    # one ulp inside
    other[2:, 0, 0:2] = (0.5, -0.25)                                          # well inside
    assert (other[0, 0, 0] - 0.25) ** 2 == r * r and (other[1, 0, 0] - 0.25) ** 2 < r * r
    idx = np.array([[0, 1], [1, 0], [0, 0], [1, 1]], np.int32)
    parts = _slots_single(eng, other, idx, ego, ego_xy)
    got = _multi_device(eng, other, idx, ego, ego_xy)[0]
    assert np.array_equal(got, _sum32(parts))
    open_part = [parts[1][0], parts[0][1]]                                    # instance 0 hears slot 1 only, instance 1 slot 0 only
    assert np.array_equal(got[0], open_part[0]) and np.array_equal(got[1], open_part[1]) and np.any(got[0] != 0) and np.any(got[1] != 0)
    assert not got[2].any() and not parts[0][0].any() and not parts[1][1].any()
    assert np.array_equal(got[3], (parts[0][3] + parts[1][3]).astype(np.float32)) and np.any(got[3] != 0)
    # gate off: every slot counts
    wide = _multi_device(eng, other, idx, ego, None)[0]
    assert np.array_equal(wide, _sum32(_slots_single(eng, other, idx, ego, None))) and np.all(np.any(wide != 0, axis=(1, 2)))


# ------------------------------------------------------------------------------------------------ the force on the plant
def _states(B, rng):
    """Plant states whose pairwise differences lie inside the network's training envelope (tests/test_formation_rollout_gpu.py)."""
    x = np.zeros((B, 10))
    x[:, 0:2] = rng.uniform(-0.75, 0.75, (B, 2))
    x[:, 2] = rng.uniform(0.5, 1.5, B)
    x[:, 3:6] = rng.normal(0, 0.5, (B, 3))
    q = rng.normal(0, 0.1, (B, 4)) + np.array([1.0, 0, 0, 0])
    x[:, 6:10] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return x


def _sum64(eng, x, idx, gate, scale=1.0):
    acc = None
    for k in range(idx.shape[1]):
        f = eng.plant_force(x, idx[:, k], gate=gate, scale=scale)
        acc = f if acc is None else acc + f
    return acc


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", [1, 2, 31, 32, 33, 129, 257])
def test_plant_force_equals_the_slot_ordered_sum_of_single_calls(oracle, mlp_blob, B, K):
    import torch
    import ndp_nmpc_qd_amd as ndp
    rng = np.random.default_rng(100 * B + K)
    eng = ndp.BatchedNMPC(B, load_mlp=True)
    x = _states(B, rng)
    cases = _index_cases(B, K, rng)
    cases["far"] = np.stack([(np.arange(B) + 128 + k) % B for k in range(K)], axis=1).astype(np.int32)   # (B = 257: another workgroup)
    beyond = cases["perm"].copy()
    beyond[:, K // 2] = B + np.arange(B)                                      # an index >= B: exactly 0, never read
    cases["beyond"] = beyond
    mixed_gate = False
    for name, idx in cases.items():
        for gate in (True, False):
            want = _sum64(eng, x, idx, gate)
            got = eng.plant_force_multi(x, idx, gate=gate)
            assert got.dtype == np.float64 and np.array_equal(got, want), (name, gate, np.abs(got - want).max())
            if K == 1:
                assert np.array_equal(got, eng.plant_force(x, idx[:, 0], gate=gate))
        d = x[np.clip(idx, 0, B - 1), 0:2] - x[:, None, 0:2]
        has = (idx >= 0) & (idx < B)
        opens = has & ((d * d).sum(-1) < R2)
        mixed_gate |= bool(np.any(opens.any(axis=1) & (has & ~opens).any(axis=1)))
    if B > 2 and K > 1:
        assert mixed_gate
    assert not eng.plant_force_multi(x, cases["beyond"][:, K // 2:K // 2 + 1]).any()
    # scale multiplies every slot's fp64 value
    mixed = cases["mixed"]
    assert np.array_equal(eng.plant_force_multi(x, mixed, gate=False, scale=0.7), _sum64(eng, x, mixed, False, 0.7))
    # the device form, with xy_out, equals the host form
    xd, fd, xyd = _t(x), torch.full((B, 3), 7.0, dtype=torch.float64, device=_dev()), torch.full((B, 2), 7.0, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    eng.plant_force_multi_device(xd, _t(mixed), fd, xy_out=xyd, scale=1.3)
    eng.synchronize()
    assert np.array_equal(fd.cpu().numpy(), eng.plant_force_multi(x, mixed, scale=1.3)) and np.array_equal(xyd.cpu().numpy(), x[:, 0:2])
    # against the oracle network summed in float64 over the slots (gate off): the project's bar, once per slot
    idx = cases["perm"]
    want, fmax = np.zeros((B, 3)), np.zeros((B, 3))
    for k in range(K):
        fk = oracle.mlp_forward(mlp_blob, (x[idx[:, k]] - x)[:, 0:6].astype(np.float32)).astype(np.float64)
        want += fk
        fmax = np.maximum(fmax, np.abs(fk))
    err = np.abs(eng.plant_force_multi(x, idx, gate=False) - want)
    print(f"B {B} K {K}: max |plant force - oracle| / max(1, max_k |f_k|) = {(err / np.maximum(1.0, fmax)).max():.3e} (bar {K}e-5)")
    assert np.all(err <= K * 1e-5 * np.maximum(1.0, fmax)), err.max()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("K", [0, 9])
def test_a_neighbour_count_outside_the_limit_is_refused(K):
    import torch
    import ndp_nmpc_qd_amd as ndp
    B, N = 4, 20
    eng, fresh = (ndp.BatchedNMPC(B, disturbance=True, load_mlp=True) for _ in range(2))
    rng = np.random.default_rng(4)
    other, ego, ego_xy = _windows(B, N, rng)
    x = _states(B, rng)
    idx = np.zeros((B, K), np.int32)
    fd = torch.full((B, N + 1, 3), 7.0, dtype=torch.float32, device=_dev())
    pd, xyd = (torch.full((B, n), 7.0, dtype=torch.float64, device=_dev()) for n in (3, 2))
    idx_t = torch.zeros((B, K), dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    calls = [lambda: eng.downwash_multi_device(_t(other), idx_t, _t(ego), fd, ego_xy=_t(ego_xy)),
             lambda: eng.downwash_multi(other, idx, ego, ego_xy),
             lambda: eng.plant_force_multi_device(_t(x), idx_t, pd, xy_out=xyd),
             lambda: eng.plant_force_multi(x, idx)]
    for call in calls:
        with pytest.raises(ndp.NdpError, match="K must be 1..8") as ei:
            call()
        assert "(-2)" in str(ei.value)
    eng.synchronize()
    assert np.all(fd.cpu().numpy() == 7.0) and np.all(pd.cpu().numpy() == 7.0) and np.all(xyd.cpu().numpy() == 7.0)   # nothing was enqueued
    b = synth.make_batch(B, seed=3)
    for e in (eng, fresh):
        e.reset(b["xr"], b["ur"])
    assert np.array_equal(eng.update(b["x0"], b["xr"], b["ur"]), fresh.update(b["x0"], b["xr"], b["ur"]))
