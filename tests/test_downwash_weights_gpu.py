"""The downwash network on the device at weights other than the shipped blob (run with -m gpu): the families of tests/mlp_families.py --
power-of-two rescalings that move half of a layer into the fp16-subnormal range without changing the function, a pruned network, a
perturbed one, a fresh initialisation, a table of conversion edge cases -- through the forward tile (stand-alone and fused into the control
step), both fragment builders and the backward pass, each against float64 (tests/mlp_vjp_ref.py).  CPU side, including the proof that
these inputs can fail: tests/test_downwash_weights.py.

Bars.  Forward: e = max |f - truth| / max(1, |truth|) <= max(1e-5, 2.5 e_fp32), truth the float64 network on the rows the device sees
((other - xr) rounded to float32), e_fp32 the error of a plain numpy fp32 evaluation of the same rows.  Backward: those of
tests/test_downwash_vjp_gpu.py.  A forward failure on tiny2 / tiny3 / big2 with `shipped` green means fp16 subnormal operands are lost
somewhere; test_fragment_builders_* tells the conversions from the tile."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag, synth
from tests import mlp_families as F
from tests import mlp_vjp_ref as R
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401
from tests.test_downwash_vjp_gpu import BAR, _case, _device_vjp, _reference

pytestmark = pytest.mark.gpu

N = F.N


def _engine(ndp, B, blob=None, device_form=False):
    """An engine that never saw the shipped weights: `blob` installed by the host form, or from device memory."""
    e = ndp.BatchedNMPC(B, N=N, disturbance=True, load_mlp=False)
    if blob is not None:
        if device_form:
            e.set_mlp_weights_device(_t(blob))
            e.synchronize()
        else:
            e.set_mlp_weights(blob)
    return e


@pytest.fixture(scope="module")
def pair(ndp):
    """Two engines of the forward tests' batch: weights set from the host on one, from device memory on the other."""
    a, b = _engine(ndp, F.FORWARD_B), _engine(ndp, F.FORWARD_B)
    yield a, b
    a.close()
    b.close()


@pytest.fixture(scope="module")
def rows():
    return F.forward_inputs()


@pytest.fixture(scope="module")
def shipped_force(pair, rows):
    other, xr, _ = rows
    pair[0].set_mlp_weights(F.family("shipped"))
    return pair[0].downwash(other, xr).reshape(-1, 3).astype(np.float64)


@pytest.mark.parametrize("name", F.FORWARD)
def test_forward_against_float64(pair, rows, shipped_force, name):
    """1 029 rows (32 full tiles and one of 5 rows), gate open, weights set by the host form and from device memory."""
    other, xr, z = rows
    blob = F.family(name)
    host, dev = pair
    host.set_mlp_weights(blob)
    dev.set_mlp_weights_device(_t(blob))
    f_host, f_dev = host.downwash(other, xr), dev.downwash(other, xr)
    truth = F.forward64(blob, z)
    f = f_host.reshape(-1, 3).astype(np.float64)
    e_dev, e_f32 = F.rel_err(f, truth), F.rel_err(F.forward32(blob, z), truth)
    print(f"forward {name}: device {e_dev:.2e}, numpy fp32 {e_f32:.2e}, max |force| {np.abs(truth).max():.3g}")
    assert np.isfinite(f_host).all()
    assert np.array_equal(f_host.view(np.uint32), f_dev.view(np.uint32))
    assert e_dev <= F.forward_bar(e_f32)
    if name in F.RESCALED:                                     # the same function: the same force, to twice the bar
        d = np.abs(f - shipped_force) / np.maximum(1.0, np.abs(shipped_force))
        print(f"forward {name}: against the shipped blob's device force {d.max():.2e}")
        assert d.max() <= 2e-5


def test_forward_cap_at_a_thousand_times_the_envelope(pair):
    """big2 with inputs 1000x the envelope: layer-2 activations pass 65 000 and are capped there.  Finite forces, equal to the float64
    network with the two hidden layers that feed a split capped at 65 000."""
    other, xr, z = F.forward_inputs(scale=F.CAP_SCALE)
    blob = F.family("big2")
    pair[0].set_mlp_weights(blob)
    f = pair[0].downwash(other, xr).reshape(-1, 3).astype(np.float64)
    assert np.isfinite(f).all()
    truth = F.forward64(blob, z, cap=True)
    e_dev, e_f32 = F.rel_err(f, truth), F.rel_err(F.forward32(blob, z, cap=True), truth)
    print(f"cap: device {e_dev:.2e}, numpy fp32 {e_f32:.2e}, against the uncapped network {F.rel_err(f, F.forward64(blob, z)):.2e}, "
          f"max |force| {np.abs(truth).max():.3g}")
    assert e_dev <= F.forward_bar(e_f32)


@pytest.mark.parametrize("name", F.ALL)
def test_fragment_builders_against_the_numpy_image(pair, name):
    """Both device images after ndp_set_mlp_weights, word for word: dFrag = mlp_frag.frag_words(blob), dFragT = blob[fragt_source()];
    after ndp_set_mlp_weights_device the same bits.  `edges` holds values of 65504 and above, which the host form refuses: it takes the
    table with those pulled just inside the range, the device form (which does not check) takes both tables."""
    host, dev = pair
    full = F.family(name)
    blob = F.in_host_range(full)
    assert (name == "edges") == (not np.array_equal(blob, full))
    host.set_mlp_weights(blob)
    fr, frt = host.debug_mlp_fragments()
    want = mlp_frag.frag_words(blob)
    bad = np.flatnonzero(fr != want)
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[:8]}: {fr[bad[:8]]} against {want[bad[:8]]}"
    assert np.array_equal(frt.view(np.uint32), blob[mlp_frag.fragt_source()].view(np.uint32))
    for b in ((blob, full) if name == "edges" else (blob,)):
        dev.set_mlp_weights(np.zeros_like(blob))
        dev.set_mlp_weights_device(_t(b))
        dev.synchronize()
        dfr, dfrt = dev.debug_mlp_fragments()
        want = mlp_frag.frag_words(b)
        bad = np.flatnonzero(dfr != want)
        assert bad.size == 0, f"device form: {bad.size} words differ, first at {bad[:8]}: {dfr[bad[:8]]} against {want[bad[:8]]}"
        assert np.array_equal(dfrt.view(np.uint32), b[mlp_frag.fragt_source()].view(np.uint32))
        if b is blob:
            assert np.array_equal(fr, dfr) and np.array_equal(frt.view(np.uint32), dfrt.view(np.uint32))


def test_host_form_refuses_values_outside_the_range_and_keeps_the_weights(ndp, pair, rows):
    other, xr, _ = rows
    e = pair[0]
    good = F.family("pert")
    e.set_mlp_weights(good)
    before, f_before = e.debug_mlp_fragments(), e.downwash(other, xr)
    off = mlp_frag.offsets()
    cases = []
    for group, value, why in (("W2", 65504.0, "of W2 is not"), ("W3", -65504.0, "of W3 is not"), ("W3", 7e4, "of W3 is not"),
                              ("W2", np.nan, "not finite"), ("b3", np.inf, "not finite"), ("W1", -np.inf, "not finite"),
                              ("b4", np.nan, "not finite")):
        bad = good.copy()
        bad[off[group][0] + 1] = value
        cases.append((bad, why))
    cases.append((F.family("edges"), "of W[23] is not"))
    for bad, why in cases:
        with pytest.raises(ndp.batched.NdpError, match=why) as ei:
            e.set_mlp_weights(bad)
        assert "(-2)" in str(ei.value)
        after = e.debug_mlp_fragments()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    assert np.array_equal(f_before, e.downwash(other, xr))
    ok = good.copy()                                           # the largest values inside the range, and large fp32 values outside layers 2 / 3
    ok[off["W2"][0] + 5], ok[off["W3"][0] + 5] = np.nextafter(np.float32(65504.0), np.float32(0.0)), -65472.0
    ok[off["W4"][0] + 5], ok[off["b2"][0] + 5] = 1e9, -1e9
    e.set_mlp_weights(ok)
    assert np.array_equal(e.debug_mlp_fragments()[0], mlp_frag.frag_words(ok))
    fresh = _engine(ndp, 4)                              # a refusal installs nothing
    with pytest.raises(ndp.batched.NdpError, match="not finite"):
        fresh.set_mlp_weights(cases[3][0])
    with pytest.raises(ndp.batched.NdpError, match="never called"):
        fresh.downwash(np.zeros((4, N + 1, 10)), np.zeros((4, N + 1, 10)))
    fresh.close()


@pytest.mark.parametrize("B", [8, 128])
@pytest.mark.parametrize("first, second", [("tiny2", "pert"), ("pert", "big2")])
def test_fused_step_under_other_weights_and_a_weight_change_on_the_stream(ndp, oracle, B, first, second):
    """The network inside the control step's launch: the force a fused step leaves is bit-equal to the stand-alone kernel's under the same
    weights, u0 agrees with the oracle fed the float64 network's forces; then new weights from device memory and a second step, enqueued
    back to back with no synchronisation in between -- that step's force is the stand-alone force under the NEW weights (a stale LDS or
    L2 image of the old ones would show)."""
    import torch
    b = synth.make_batch(B, seed=synth.SEED0 + 60 + B, downwash=True)
    w1, w2 = F.family(first), F.family(second)
    alone = _engine(ndp, B, w1)
    f1 = alone.downwash(b["other"], b["xr"], b["ego_xy"])
    alone.set_mlp_weights(w2)
    f2 = alone.downwash(b["other"], b["xr"], b["ego_xy"])
    alone.close()
    d = b["other"][:, 0, :2] - b["ego_xy"]
    live = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < float(_lib.default_cfg().r_horiz) ** 2
    assert 0 < live.sum() < B and not f1[~live].any() and f1[live].any(axis=(1, 2)).all()
    assert np.abs(f1 - f2).max() > 1e-3                        # (the two families are different functions)
    e = _engine(ndp, B, w1)
    e.reset(b["xr"], b["ur"])
    assert e.debug_rti_launched()[2]                           # the network can run inside the step's launch at this shape
    u0 = e.update(b["x0"], b["xr"], b["ur"], other=b["other"], ego_xy=b["ego_xy"])
    force = e.device_force().cpu().numpy()
    assert np.array_equal(force.view(np.uint32), f1.view(np.uint32))
    z = (b["other"][:, :, :6] - b["xr"][:, :, :6]).astype(np.float32).astype(np.float64)
    f64 = F.forward64(w1, z.reshape(-1, 6)).reshape(B, N + 1, 3) * live[:, None, None]
    cfg = oracle.default_cfg(N=N, use_fd=True)
    X, U = b["xr"].copy(), b["ur"].copy()
    u0o, sto, _ = oracle.step_batch(cfg, b["x0"], b["xr"], b["ur"], f64, X, U)
    err = np.abs(u0 - u0o) / np.maximum(1.0, np.abs(u0o))
    print(f"fused B = {B} {first}: {int(live.sum())} gates open, u0 against the oracle under the float64 force {err.max():.2e}")
    assert not sto.any() and not e.status()[0].any()
    assert err.max() <= 1e-6
    # new weights and the next step, nothing in between
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur", "other", "ego_xy")}
    w2_t = _t(w2)
    u0_t = torch.empty(B, 4, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    e.set_mlp_weights_device(w2_t)
    e.update_device(t["x0"], t["xr"], t["ur"], u0_t, other=t["other"], ego_xy=t["ego_xy"])
    e.synchronize()
    force2 = e.device_force().cpu().numpy()
    e.close()
    assert np.array_equal(force2.view(np.uint32), f2.view(np.uint32))


@pytest.fixture(scope="module")
def engines(ndp):
    es = {B: _engine(ndp, B) for B in F.BACKWARD_B}
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("B", F.BACKWARD_B)
@pytest.mark.parametrize("form", F.BACKWARD_FORMS)
@pytest.mark.parametrize("name", F.BACKWARD)
def test_backward_against_float64(engines, name, form, B):
    """ndp_downwash_vjp_device against vjp64 of the family's blob: 5 376 rows, and 105 rows (a partial tile, padding rows).  Margin rule:
    mlp_families.drop_rows (the rescaled families under the shipped blob's margin -- the same ReLU pattern, the same rows)."""
    e = engines[B]
    blob = F.family(name)
    e.set_mlp_weights(blob)
    c = _case(form, F.backward_seed(form, B), B=B)
    drop = F.drop_rows(name, blob, c["z"])
    assert float(drop.mean()) <= R.MAX_DROPPED and c["live"].any()
    gf = c["gf"] * ~drop[:, :, None]
    gz, gw = _device_vjp(e, c, gf)
    gz2, gw2 = _device_vjp(e, c, gf)
    rz, rw, _ = _reference(c, gf, blob)
    err = np.abs(gz - rz).max(axis=2) / np.maximum(1.0, np.abs(rz).max(axis=2))
    ge = R.group_errors(gw, rw)
    print(f"backward {name} {form} B = {B}: {int(c['live'].sum())} live, {float(drop.mean()):.4f} of the rows below the margin, "
          f"g_z error {err.max():.3e}; groups " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert np.array_equal(gz, gz2) and np.array_equal(gw, gw2)
    assert err.max() <= BAR
    assert max(ge.values()) <= BAR, ge
    assert not gz[~c["live"]].any()                            # closed and neighbour-less instances: exactly 0
