"""The derivatives of the downwash force on the plant on the device (run with -m gpu): ndp_plant_force_vjp_device,
ndp_plant_force_jvp_device and their multi forms, bit for bit against the existing derivative of the prediction on windows packed from the
states, single against multi, repeatability, against the float64 reference (tests/plant_force_deriv_ref.py), the edge cases, the refusals,
and two ticks of plant_force -> plant_step in one autograd graph.  CPU side: tests/test_plant_force_deriv.py.

Bars (the project's 1e-5 for this network, BAR in tests/test_downwash_multi_deriv_gpu.py): every parameter group of g_w max|err| <= 1e-5
max|reference group|; |g_z - ref| and |df - ref| <= 1e-5 max(1, max|ref| of the row).  No slot is dropped from a reference comparison:
failing slots are redrawn (plant_force_deriv_ref.shared_case)."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag
from tests import mlp_vjp_ref as R
from tests import plant_force_deriv_ref as F
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401

pytestmark = pytest.mark.gpu

N = 20
BAR = 1e-5
# the chain's bar: ten times the measured maximum (see test_two_ticks_of_plant_force_and_plant_step_in_one_graph)
CHAIN_BAR = 10 * 2.6e-7
# (B, K, N): a tile of one row; 40 rows in one workgroup of two busy waves; a one-row second tile twice over (66 rows); 192 rows, a second
# workgroup with two busy waves; 257 vehicles, a one-row ninth tile in forward mode; and N = 2, the shortest horizon: 512 rows are 4
# workgroups of work on the 2 the workspace has rows for -- the reverse launch's grid-stride loop runs a second round
SHAPES = [(1, 1, N), (5, 8, N), (33, 2, N), (64, 3, N), (257, 1, N), (64, 8, 2)]
REF_SHAPES = [(7, 3), (64, 3), (2048, 2)]


@pytest.fixture(scope="module")
def engines(ndp):
    made = {}

    def get(B, n=N, **kw):
        key = (B, n, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = ndp.BatchedNMPC(B, N=n, disturbance=True, **kw)
            assert made[key].cfg.r_horiz == F.R_HORIZ
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def blob():
    return _lib.load_weights()


_ref = {}


def _ref_case(blob, B, K):
    """plant_force_deriv_ref.shared_case, made once per (B, K) and shared (nothing changes it)."""
    if (B, K) not in _ref:
        _ref[B, K] = F.shared_case(2000 + 10 * B + K, blob, B, K)
    return _ref[B, K]


def _mixed_case(seed, B, K):
    """Device against device only (nothing is drawn for a reference): random neighbours, the vehicle itself among them, about 15 % of the
    slots empty as -1 and a few as an index past the batch; positions U(+-0.75), so a mix of open and closed gates."""
    rng = np.random.default_rng(seed)
    x = F.draw_states(rng, B)
    idx = rng.integers(0, B, (B, K)).astype(np.int32)
    idx[rng.random((B, K)) < 0.15] = -1
    idx[rng.random((B, K)) < 0.05] = B + 3
    if B == 1:
        idx[:] = 0
    return x, idx


def _vjp(eng, x, idx, gf, gate=True, scale=1.0, want_gz=True, want_gw=True, single=False, stream=None):
    """plant_force[_multi]_vjp_device into buffers filled with -7.0; numpy (gz [B,K,6], gw)."""
    import torch
    B, K = idx.shape
    gz = torch.full((B, 6) if single else (B, K, 6), -7.0, dtype=torch.float64, device=_dev()) if want_gz else None
    gw = torch.full((mlp_frag.NPARAM,), -7.0, dtype=torch.float32, device=_dev()) if want_gw else None
    if single:
        eng.plant_force_vjp_device(_t(x), _t(idx[:, 0]), _t(gf), gz=gz, gw=gw, gate=gate, scale=scale, stream=stream)
    else:
        eng.plant_force_multi_vjp_device(_t(x), _t(idx), _t(gf), gz=gz, gw=gw, gate=gate, scale=scale, stream=stream)
    eng.synchronize()
    torch.cuda.synchronize()
    return None if gz is None else gz.cpu().numpy().reshape(B, K, 6), None if gw is None else gw.cpu().numpy()


def _jvp(eng, x, idx, tx, tw, T, gate=True, scale=1.0, check=True, single=False):
    """plant_force[_multi]_jvp_device into buffers filled with -7.0; numpy (df [B,T,3], f_check [B,3] or None)."""
    import torch
    B = idx.shape[0]
    df = torch.full((B, T, 3), -7.0, dtype=torch.float64, device=_dev())
    fc = torch.full((B, 3), -7.0, dtype=torch.float64, device=_dev()) if check else None
    call = eng.plant_force_jvp_device if single else eng.plant_force_multi_jvp_device
    call(_t(x), _t(idx[:, 0] if single else idx), tx=None if tx is None else _t(tx), tw=None if tw is None else _t(tw), n_tan=T, df=df,
         f_check=fc, gate=gate, scale=scale)
    eng.synchronize()
    torch.cuda.synchronize()
    return df.cpu().numpy(), None if fc is None else fc.cpu().numpy()


def _force(eng, x, idx, gate=True, scale=1.0):
    import torch
    f = torch.full((idx.shape[0], 3), -7.0, dtype=torch.float64, device=_dev())
    eng.plant_force_multi_device(_t(x), _t(idx), f, gate=gate, scale=scale)
    eng.synchronize()
    torch.cuda.synchronize()
    return f.cpu().numpy()


def _directions(seed, blob, B, T):
    rng = np.random.default_rng(seed)
    tx = rng.normal(size=(B, T, 10))
    tw = (np.asarray(blob, dtype=np.float64)[None] * 0.1 * rng.normal(size=(T, mlp_frag.NPARAM))).astype(np.float32)
    return tx, tw


# ---------------------------------------------------------------- bit-equality with the existing derivative, on packed windows
@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("B,K,n", SHAPES)
def test_bit_equal_to_the_prediction_derivative_on_windows_packed_from_the_states(engines, blob, B, K, n, gate):
    """Windows other[o][node] = x[o], ego_ref[v][node] = x[v], ego_xy = x[v][0:2]; upstream scale * gf[v] at node 0 and zero elsewhere; tz at
    node 0 = tx[o] - tx[v].  Then d_gz[v][k] is node 0 of ndp_downwash_multi_vjp_device's d_gz, d_df (scale 1) is node 0 of
    ndp_downwash_multi_jvp_device's, and d_f_check is ndp_plant_force_multi_device's force, all bit for bit."""
    import torch
    eng = engines(B, n)
    x, idx = _mixed_case(10 * B + K, B, K)
    has = (idx >= 0) & (idx < B)
    op = F.gather(x, idx, gate)[1]
    if B > 1:
        assert op.any() and (gate is False or (has & ~op).any()) and (~has).any()
    rng = np.random.default_rng(B * K)
    gf = rng.normal(size=(B, 3))
    scale = 0.7
    gz, gw = _vjp(eng, x, idx, gf, gate, scale)
    assert not gz[~op].any() and np.abs(gz[op]).max(axis=1).min() > 0 and np.isfinite(gw).all() and np.abs(gw).max() > 0
    win = _t(np.ascontiguousarray(np.broadcast_to(x[:, None], (B, n + 1, 10))))
    idw = _t(np.where(has, idx, -1).astype(np.int32))           # (the windowed calls read any index >= 0)
    exy = _t(x[:, :2]) if gate else None
    up = np.zeros((B, n + 1, 3))
    up[:, 0] = scale * gf
    wz = torch.full((B, K, n + 1, 6), -7.0, dtype=torch.float64, device=_dev())
    eng.downwash_multi_vjp_device(win, idw, win, _t(up), ego_xy=exy, gz=wz)
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(gz, wz.cpu().numpy()[:, :, 0])
    T = 2
    tx, tw = _directions(7 + B + K, blob, B, T)
    df, fc = _jvp(eng, x, idx, tx, tw, T, gate, 1.0)
    tz = np.zeros((B, T, K, n + 1, 6))
    o = np.where(has, idx, np.arange(B)[:, None])
    tz[:, :, :, 0] = (tx[o][..., :6] - tx[:, None, :, :6]).transpose(0, 2, 1, 3)
    wd = torch.full((B, T, n + 1, 3), -7.0, dtype=torch.float64, device=_dev())
    eng.downwash_multi_jvp_device(win, idw, win, tz=_t(tz), tw=_t(tw), ego_xy=exy, n_tan=T, df=wd)
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(df, wd.cpu().numpy()[:, :, 0])
    assert not df[~op.any(axis=1)].any()
    assert np.array_equal(fc, _force(eng, x, idx, gate, 1.0))
    assert np.array_equal(_jvp(eng, x, idx, tx, tw, T, gate, scale)[1], _force(eng, x, idx, gate, scale))


# ---------------------------------------------------------------- single against multi, repeatability
@pytest.mark.parametrize("B,K", [(33, 1), (5, 8), (64, 3)])
def test_single_equals_multi_and_calls_repeat_bit_for_bit(engines, blob, B, K):
    eng = engines(B)
    x, idx = _mixed_case(50 + B + K, B, K)
    rng = np.random.default_rng(B + K)
    gf = rng.normal(size=(B, 3))
    scale, T = 0.7, 4
    gz, gw = _vjp(eng, x, idx, gf, True, scale)
    gz2, gw2 = _vjp(eng, x, idx, gf, True, scale)
    assert np.array_equal(gz, gz2) and np.array_equal(gw, gw2)                  # two calls
    gz_only, _ = _vjp(eng, x, idx, gf, True, scale, want_gw=False)
    _, gw_only = _vjp(eng, x, idx, gf, True, scale, want_gz=False)
    assert np.array_equal(gz_only, gz) and np.array_equal(gw_only, gw)          # an output does not depend on which others are asked for
    tx, tw = _directions(B * K, blob, B, T)
    df, fc = _jvp(eng, x, idx, tx, tw, T, True, scale)
    df2, _ = _jvp(eng, x, idx, tx, tw, T, True, scale, check=False)
    assert np.array_equal(df, df2)
    for t in range(T):                                                           # T directions in one call = T calls
        one, _ = _jvp(eng, x, idx, tx[:, t:t + 1], tw[t:t + 1], 1, True, scale)
        assert np.array_equal(one[:, 0], df[:, t]), t
    dz, _ = _jvp(eng, x, idx, tx, None, T, True, scale)                          # one kind of direction alone
    dw, _ = _jvp(eng, x, idx, None, tw, T, True, scale)
    assert np.abs(dz).max() > 0 and np.abs(dw).max() > 0
    assert np.abs(dz + dw - df).max() <= 1e-3 * max(1.0, np.abs(df).max())      # (linear in the direction, up to fp32 rounding)
    if K == 1:
        sz, sw = _vjp(eng, x, idx, gf, True, scale, single=True)
        sd, sf = _jvp(eng, x, idx, tx, tw, T, True, scale, single=True)
        assert np.array_equal(sz, gz) and np.array_equal(sw, gw) and np.array_equal(sd, df) and np.array_equal(sf, fc)
        d1, _ = _jvp(eng, x, idx, tx, tw, T, True, 1.0)
        assert np.array_equal(df, scale * d1)                                    # df(scale) is the fp64 product scale * df(1)


# ---------------------------------------------------------------- against the float64 reference
@pytest.mark.parametrize("gate,scale", [(True, 1.0), (True, 0.7), (False, 1.0), (False, 0.7)])
@pytest.mark.parametrize("B,K", REF_SHAPES)
def test_against_the_float64_reference(engines, blob, B, K, gate, scale):
    """g_w (every parameter group), g_z per slot and df (T = 2: the states' direction alone, then states and weights) on shared-state
    inputs; (2048, 2) is 32 workgroups of reverse work.  Measured maxima: DESIGN 9."""
    c = _ref_case(blob, B, K)
    x, idx = c["x"], c["index"]
    eng = engines(B)
    rng = np.random.default_rng(3 * B + K)
    gf = rng.normal(size=(B, 3))
    gz, gw = _vjp(eng, x, idx, gf, gate, scale)
    T = 2
    tx, tw = _directions(11 + B + K, blob, B, T)
    tw[0] = 0.0
    df, fc = _jvp(eng, x, idx, tx, tw, T, gate, scale)
    rz, _, rw, margin = F.vjp64(blob, x, idx, gf, gate, scale)
    op = F.gather(x, idx, gate)[1]
    assert margin[idx >= 0].min() >= R.MARGIN and op.any()      # nothing to drop: failing slots were redrawn
    ge = R.group_errors(gw, rw)
    err_z = float((np.abs(gz - rz).max(axis=2) / np.maximum(1.0, np.abs(rz).max(axis=2))).max())
    err_d = 0.0
    for t in range(T):
        rd = F.jvp64(blob, x, idx, tx[:, t], tw[t], gate, scale)
        err_d = max(err_d, float((np.abs(df[:, t] - rd).max(axis=1) / np.maximum(1.0, np.abs(rd).max(axis=1))).max()))
    rf = F.force64(blob, x, idx, gate, scale)
    err_f = float((np.abs(fc - rf).max(axis=1) / np.maximum(1.0, np.abs(rf).max(axis=1))).max())
    print(f"B = {B} K = {K} gate {gate} scale {scale}: {int(op.sum())} of {B * K} slots open, {c['redrawn']} states redrawn in {c['rounds']} "
          f"rounds; g_z {err_z:.3e}, df {err_d:.3e}, f {err_f:.3e}; groups " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert max(ge.values()) <= BAR, ge
    assert err_z <= BAR and err_d <= BAR and err_f <= BAR


# ---------------------------------------------------------------- edge cases
@pytest.mark.parametrize("how", ["empty", "closed", "past"])
def test_every_slot_closed_or_empty_gives_exact_zeros(engines, blob, how):
    B, K = 7, 3
    x, idx = _mixed_case(3, B, K)
    if how == "empty":
        idx = np.full((B, K), -1, dtype=np.int32)
    elif how == "past":
        idx = np.full((B, K), B, dtype=np.int32)
    else:
        x[:, 0] = 5.0 * np.arange(B)                           # every pair further apart than r_horiz
        idx = ((np.arange(B)[:, None] + 1 + np.arange(K)[None]) % B).astype(np.int32)
    gf = np.random.default_rng(1).normal(size=(B, 3))
    gz, gw = _vjp(engines(B), x, idx, gf)
    tx, tw = _directions(2, blob, B, 2)
    df, fc = _jvp(engines(B), x, idx, tx, tw, 2)
    assert not gz.any() and not gw.any() and not df.any() and not fc.any()


def test_no_index_gives_exact_zeros_without_weights(ndp):
    import torch
    B = 7
    e = ndp.BatchedNMPC(B, N=N, disturbance=True, load_mlp=False)
    x = _t(F.draw_states(np.random.default_rng(0), B))
    gf = _t(np.ones((B, 3)))
    tx = _t(np.ones((B, 2, 10)))
    for single in (True, False):
        gz = torch.full((B, 6) if single else (B, 3, 6), -7.0, dtype=torch.float64, device=_dev())
        gw = torch.full((mlp_frag.NPARAM,), -7.0, dtype=torch.float32, device=_dev())
        df = torch.full((B, 2, 3), -7.0, dtype=torch.float64, device=_dev())
        fc = torch.full((B, 3), -7.0, dtype=torch.float64, device=_dev())
        (e.plant_force_vjp_device if single else e.plant_force_multi_vjp_device)(x, None, gf, gz=gz, gw=gw)
        (e.plant_force_jvp_device if single else e.plant_force_multi_jvp_device)(x, None, tx=tx, df=df, f_check=fc)
        e.synchronize()
        torch.cuda.synchronize()
        assert not gz.any() and not gw.any() and not df.any() and not fc.any()
    # ... and with an index the missing weights are named
    idx = torch.zeros(B, 1, dtype=torch.int32, device=_dev())
    with pytest.raises(Exception, match="never called"):
        e.plant_force_multi_vjp_device(x, idx, gf, gz=torch.empty(B, 1, 6, dtype=torch.float64, device=_dev()))
    with pytest.raises(Exception, match="never called"):
        e.plant_force_jvp_device(x, idx[:, 0].contiguous(), tx=tx, df=torch.empty(B, 2, 3, dtype=torch.float64, device=_dev()))
    e.close()


def test_an_index_past_the_batch_is_an_empty_slot(engines, blob):
    """o >= B is never read: the state tensor has exactly B rows, and the results are those of the same call with -1 in these slots."""
    B, K = 33, 2
    x, idx = _mixed_case(8, B, K)
    idx[::3, 1] = B
    idx[1::5, 0] = 2 ** 31 - 1
    clean = np.where(idx >= B, -1, idx).astype(np.int32)
    assert (idx >= B).sum() >= 10
    gf = np.random.default_rng(2).normal(size=(B, 3))
    tx, tw = _directions(3, blob, B, 2)
    for a, b in zip(_vjp(engines(B), x, idx, gf) + _jvp(engines(B), x, idx, tx, tw, 2),
                    _vjp(engines(B), x, clean, gf) + _jvp(engines(B), x, clean, tx, tw, 2)):
        assert np.array_equal(a, b)


def test_the_same_index_in_two_slots_counts_twice(engines, blob):
    B = 7
    x, one = _mixed_case(4, B, 1)
    one[:, 0] = (np.arange(B) + 1) % B
    x[:, :2] *= 0.3                                             # every gate open
    two = np.concatenate([one, one], axis=1)
    pad = np.concatenate([one, np.full_like(one, -1)], axis=1)
    gf = np.random.default_rng(3).normal(size=(B, 3))
    tx, tw = _directions(4, blob, B, 2)
    e = engines(B)
    gz1, gw1 = _vjp(e, x, pad, gf, scale=0.7)
    gz2, gw2 = _vjp(e, x, two, gf, scale=0.7)
    assert np.array_equal(gz2[:, 0], gz1[:, 0]) and np.array_equal(gz2[:, 1], gz1[:, 0]) and not gz1[:, 1].any()
    assert np.abs(gw2 - 2.0 * gw1).max() <= 1e-5 * np.abs(gw1).max()           # (the same terms twice, summed in another order)
    d1, f1 = _jvp(e, x, pad, tx, tw, 2, scale=0.7)
    d2, f2 = _jvp(e, x, two, tx, tw, 2, scale=0.7)
    assert np.array_equal(d2, d1 + d1) and np.array_equal(f2, f1 + f1) and np.abs(f1).min(axis=1).max() > 0


def test_a_vehicle_that_is_its_own_neighbour_gets_an_exactly_zero_state_gradient(engines, blob):
    import torch
    from ndp_nmpc_qd_amd.torch_layer import plant_force
    B = 7
    x, idx = _mixed_case(6, B, 2)
    idx[:] = -1
    idx[2, 1] = 2
    idx[5, 0] = 5
    xt = _t(x).requires_grad_(True)
    f = plant_force(engines(B), xt, _t(idx))
    assert f[2].abs().max() > 0 and f[5].abs().max() > 0 and not f[0].any()     # the network at z = 0 is not zero
    (gx,) = torch.autograd.grad(f, (xt,), torch.ones_like(f))
    assert not gx.any()


def test_non_finite_rows_stay_out_of_the_weights_and_get_nan_themselves(engines, blob):
    B, K = 64, 3
    c = _ref_case(blob, B, K)
    x, idx = c["x"], c["index"]
    e = engines(B)
    op = F.gather(x, idx, True)[1]
    v = int(np.flatnonzero(op.any(axis=1) & ~op.all(axis=1))[0])               # a vehicle with an open and a closed slot
    gf = np.random.default_rng(4).normal(size=(B, 3))
    bad, zeroed = gf.copy(), gf.copy()
    bad[v, 1] = np.nan
    zeroed[v] = 0.0
    gz, gw = _vjp(e, x, idx, bad)
    gz0, gw0 = _vjp(e, x, idx, zeroed)
    assert np.isfinite(gw).all() and np.array_equal(gw, gw0)
    assert np.isnan(gz[v, op[v]]).all() and not gz[v, ~op[v]].any()
    gz[v], gz0[v] = 0.0, 0.0
    assert np.isfinite(gz).all() and np.array_equal(gz, gz0)
    # a state that is not finite (a velocity: the gates stay as they are): every open slot it is part of, as ego or as neighbour
    xb = x.copy()
    xb[v, 4] = np.inf
    hit = op & ((np.arange(B)[:, None] == v) | (idx == v))
    assert hit[v].any()
    without = np.where(hit, -1, idx).astype(np.int32)
    gz, gw = _vjp(e, xb, idx, gf)
    gz0, gw0 = _vjp(e, x, without, gf)
    assert np.isfinite(gw).all() and np.array_equal(gw, gw0)
    assert np.isnan(gz[hit]).all()
    gz[hit] = 0.0
    assert np.isfinite(gz).all() and np.array_equal(gz, gz0)


def test_the_engine_is_untouched(ndp, blob):
    import torch
    B, K = 64, 2
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    state = lambda: [v.clone() for v in e.device_iterate()] + [e.device_force().clone(), torch.as_tensor(e.active_set()[1]),  # noqa: E731
                                                                 *(torch.as_tensor(a) for a in e.debug_mlp_fragments())]
    before = state()
    x, idx = _mixed_case(9, B, K)
    gf = np.random.default_rng(5).normal(size=(B, 3))
    tx, tw = _directions(6, blob, B, 2)
    gz, gw = _vjp(e, x, idx, gf)
    df, _ = _jvp(e, x, idx, tx, tw, 2)
    assert np.abs(gw).max() > 0 and np.abs(df).max() > 0
    for a, b in zip(before, state()):
        assert torch.equal(a.cpu(), b.cpu())
    e.close()


def test_refusals_name_their_reason_and_leave_the_outputs_untouched(ndp, blob):
    import torch
    B, K = 5, 2
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    x = _t(F.draw_states(np.random.default_rng(0), B))
    idx = torch.zeros(B, 9, dtype=torch.int32, device=_dev())
    gf = torch.zeros(B, 3, dtype=torch.float64, device=_dev())
    gz = torch.full((B, 9, 6), -7.0, dtype=torch.float64, device=_dev())
    tw = torch.zeros(9, mlp_frag.NPARAM, dtype=torch.float32, device=_dev())
    df = torch.full((B, 9, 3), -7.0, dtype=torch.float64, device=_dev())
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    L, h = e._lib, e._h
    mvjp = lambda xx, k, g, z: L.ndp_plant_force_multi_vjp_device(h, p(xx), p(idx), k, 1, 1.0, p(g), p(z), None, None)  # noqa: E731
    svjp = lambda xx, g, z: L.ndp_plant_force_vjp_device(h, p(xx), p(idx), 1, 1.0, p(g), p(z), None, None)  # noqa: E731
    mjvp = lambda xx, k, T, w, d: L.ndp_plant_force_multi_jvp_device(h, p(xx), p(idx), k, 1, 1.0, T, None, p(w), p(d), None, None)  # noqa: E731
    sjvp = lambda xx, T, w, d: L.ndp_plant_force_jvp_device(h, p(xx), p(idx), 1, 1.0, T, None, p(w), p(d), None, None)  # noqa: E731
    assert mvjp(None, K, gf, gz) == -1 and svjp(None, gf, gz) == -1 and mjvp(None, K, 1, tw, df) == -1 and sjvp(None, 1, tw, df) == -1
    for args, why in (((x, 0, gf, gz), b"K must be"), ((x, 9, gf, gz), b"K must be"), ((x, K, None, gz), b"d_gf"), ((x, K, gf, None), b"no output")):
        assert mvjp(*args) == -2 and why in L.ndp_last_error(h), why
    for args, why in (((x, None, gz), b"d_gf"), ((x, gf, None), b"no output")):
        assert svjp(*args) == -2 and why in L.ndp_last_error(h) and b"ndp_plant_force_vjp_device" in L.ndp_last_error(h), why
    for args, why in (((x, 0, 1, tw, df), b"K must be"), ((x, 9, 1, tw, df), b"K must be"), ((x, K, 9, tw, df), b"n_tan"), ((x, K, 0, tw, df), b"n_tan"),
                      ((x, K, 1, None, df), b"no tangent"), ((x, K, 1, tw, None), b"d_df")):
        assert mjvp(*args) == -2 and why in L.ndp_last_error(h), why
    for args, why in (((x, 9, tw, df), b"n_tan"), ((x, 1, None, df), b"no tangent"), ((x, 1, tw, None), b"d_df")):
        assert sjvp(*args) == -2 and why in L.ndp_last_error(h), why
    e.synchronize()
    torch.cuda.synchronize()
    assert (gz == -7.0).all() and (df == -7.0).all()
    e.close()
    e = ndp.BatchedNMPC(B, N=N, disturbance=True, load_mlp=False)
    L, h = e._lib, e._h
    for rc in (mvjp(x, K, gf, gz), svjp(x, gf, gz), mjvp(x, K, 1, tw, df), sjvp(x, 1, tw, df)):
        assert rc == -6 and b"never called" in L.ndp_last_error(h)
    e.synchronize()
    torch.cuda.synchronize()
    assert (gz == -7.0).all() and (df == -7.0).all()
    e.close()


# ---------------------------------------------------------------- the chain
def test_two_ticks_of_plant_force_and_plant_step_in_one_graph(engines, blob):
    """B = 7, K = 2, two ticks of f = plant_force(x); x = plant_step(x, u, f) in one autograd graph on a non-default stream, the loss <g, x
    after the second tick>.  The leaf gradients of x0, u and the weights and a tangent chained by hand (plant_force_jvp, plant_rollout_jvp)
    against the float64 reference composed with tests/plant_deriv_ref.py.  Measured (this seed): the final state 3.5e-8, g_x0 4.0e-8, g_u 1.1e-9
    and the tangent 8.4e-8 of max(1, max|ref| of the row), the weights' groups at most 2.6e-7 of max|reference group| (W2); the bar is ten
    times the largest, 2.6e-6, which leaves room for other seeds and stays under the network's 1e-5.  A second backward gives the same bits; with only the weights requiring grad the weights' gradient is the same
    bits again."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import plant_force, plant_force_jvp, plant_rollout_jvp, plant_step
    B, K, ticks = 7, 2, 2
    c = F.chain_case(300, blob, B, K, ticks)
    x0, idx, u = c["x"], c["index"], c["u"]
    e = engines(B)
    rng = np.random.default_rng(12)
    g = rng.normal(size=(B, 10))
    tx0, tu = rng.normal(size=(B, 10)), rng.normal(size=u.shape)
    tw = (np.asarray(blob, dtype=np.float64) * 0.1 * rng.normal(size=mlp_frag.NPARAM)).astype(np.float32)
    it = _t(idx)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(s):
        def run(need_x, need_u):
            xt, ut = _t(x0).requires_grad_(need_x), _t(u).requires_grad_(need_u)
            wt = _t(blob).requires_grad_(True)
            x = xt
            for k in range(ticks):
                f = plant_force(e, x, it, weights=wt)
                x = plant_step(e, x, ut[k], f)
            return x, xt, ut, wt
        x, xt, ut, wt = run(True, True)
        loss = (x * _t(g)).sum()
        first = [t.clone() for t in torch.autograd.grad(loss, (xt, ut, wt), retain_graph=True)]
        again = torch.autograd.grad(loss, (xt, ut, wt))
        x2, _, _, wt2 = run(False, False)
        (gw_only,) = torch.autograd.grad((x2 * _t(g)).sum(), (wt2,))
        # the tangent, chained by hand
        dx, xk = _t(tx0), _t(x0)
        for k in range(ticks):
            f, df = plant_force_jvp(e, xk, it, (dx, _t(tw)), weights=wt.detach())
            xs, dxs = plant_rollout_jvp(e, xk, _t(u[k:k + 1]), (dx, _t(tu[k:k + 1]), df[None]), f=f[None])
            xk, dx = xs[0], dxs[0]
        s.synchronize()
    e.synchronize()
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert torch.equal(gw_only, first[2]) and torch.equal(x2, x.detach()) and torch.equal(xk, x.detach())
    gx0, gu, gw = (t.cpu().numpy() for t in first)
    xs_ref, _ = F.chain_forward(blob, x0, u, idx)
    assert F.chain_ok(blob, xs_ref, idx)
    rx0, ru, rw = F.chain_vjp(blob, x0, u, idx, g)
    rd = F.chain_jvp(blob, x0, u, idx, tx0, tu, tw.astype(np.float64))
    rel = lambda a, b: float((np.abs(a - b).max(axis=-1) / np.maximum(1.0, np.abs(b).max(axis=-1))).max())  # noqa: E731
    ge = R.group_errors(gw, rw)
    errs = dict(x=rel(x.detach().cpu().numpy(), xs_ref[-1]), gx0=rel(gx0, rx0), gu=rel(gu, ru), tangent=rel(dx.cpu().numpy(), rd),
                gw=max(ge.values()))
    print(f"seed {c['seed']}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()) + "; groups " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert np.abs(rx0).max() > 0 and np.abs(rw).max() > 0 and np.abs(gx0[:, :6]).max() > 0
    assert max(errs.values()) <= CHAIN_BAR, errs
