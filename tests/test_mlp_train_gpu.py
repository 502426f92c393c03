"""Training the downwash network on the device (run with -m gpu): the spectral norms, one optimiser step from arbitrary states, steps
enqueued back to back, the skipped step, the installed weights and a 40-step fit through the torch optimiser, each against the float64
reference of tests/mlp_train_ref.py.  CPU side (the reference held to torch.optim.Adam, the same fit on the reference alone):
tests/test_mlp_train.py.

Bars.  Norms: |sigma / sigma64 - 1| <= 1e-12 (the fp64 Gram matrix and eigenvalue solve carry O(64 x 2^-53); two decades of room), exactly
0 on a zero matrix.  State: m, v and p within ONE float32 ulp of step64, the ulp taken at the larger of the old and the new magnitude --
both sides round a float64 value of relative error about 2^-50, so they can differ only across a rounding boundary; the share of values
that differ at all is printed.  The norms a step reports are held to sigma64 of the weights the DEVICE left (a weight one ulp off moves a
norm by more than 1e-12)."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import mlp_frag
from tests import mlp_train_ref as T
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401

pytestmark = pytest.mark.gpu

NP = mlp_frag.NPARAM
SIGMA_BAR = 1e-12


@pytest.fixture(scope="module")
def eng(ndp):
    e = ndp.BatchedNMPC(T.FIT_B, N=T.FIT_N, disturbance=True)
    yield e
    e.close()


def _sigma_err(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return np.where(want > 0, np.abs(got / np.where(want > 0, want, 1.0) - 1.0), np.abs(got) / 1e-300 * SIGMA_BAR)


@pytest.mark.parametrize("name", T.FAMILIES)
def test_norms_against_the_svd(eng, name):
    import torch
    blob = T.family(name)
    want = T.sigmas64(blob)
    sig = torch.full((4,), -7.0, dtype=torch.float64, device=_dev())
    w = _t(blob)
    torch.cuda.synchronize()
    eng.mlp_spectral_norms_device(w, sig)
    eng.synchronize()
    got, host = sig.cpu().numpy(), eng.mlp_spectral_norms(blob)
    err = _sigma_err(got, want)
    print(f"norms {name}: sigma64 {want}, relative error {err}")
    assert np.array_equal(got, host)
    assert np.array_equal(w.cpu().numpy().view(np.uint32), blob.view(np.uint32))     # the weights are only read
    if name == "zero":
        assert not got.any()
    assert (err <= SIGMA_BAR).all()


# ---------------------------------------------------------------------------------------------------------------- one step
def _state(seed, gfam, blob):
    """(g, m, v) float32 and the betas of a gradient family."""
    rng = np.random.default_rng(seed)
    g = (1e-2 * rng.normal(size=NP)).astype(np.float32)
    m = (1e-2 * rng.normal(size=NP)).astype(np.float32)
    v = ((1e-2 * (0.1 + rng.uniform(size=NP))) ** 2).astype(np.float32)
    betas = (0.9, 0.999)
    if gfam == "zero":                       # a zero gradient on a fresh optimiser: p unchanged, nothing NaN
        g, m, v = (np.zeros(NP, dtype=np.float32) for _ in range(3))
    elif gfam == "tiny":                     # |g| ~ 1e-22 on a v in the float32 subnormal range
        g = (1e-22 * (1.0 + 0.5 * rng.uniform(size=NP)) * rng.choice([-1.0, 1.0], size=NP)).astype(np.float32)
        m = (1e-22 * rng.normal(size=NP)).astype(np.float32)
        v = rng.uniform(0.0, 1e-39, size=NP).astype(np.float32)
        assert (v < np.finfo(np.float32).tiny).all() and v.any()
    elif gfam == "tiny_fresh":               # ... and a fresh optimiser whose v is g^2 / 2 itself: a few float32 subnormal steps
        g = (1e-22 * (1.0 + 0.5 * rng.uniform(size=NP)) * rng.choice([-1.0, 1.0], size=NP)).astype(np.float32)
        m, v = np.zeros(NP, dtype=np.float32), np.zeros(NP, dtype=np.float32)
        betas = (0.9, 0.5)
    elif gfam == "layer_zero":               # one layer's gradient zero (W2 and b2)
        o = mlp_frag.offsets()
        g[o["W2"][0]:o["W3"][0]] = 0.0
    return g, m, v, betas


def _device_step(eng, p, g, m, v, step, cap=0.0, betas=(0.9, 0.999), calls=1, install=False):
    """`calls` ndp_mlp_adam_sn_device calls enqueued back to back on the engine's stream; the state they leave, as numpy."""
    import torch
    w, gt, mt, vt = (_t(a) for a in (p, g, m, v))
    st = torch.tensor([step], dtype=torch.int64, device=_dev())
    sig = torch.full((4,), -7.0, dtype=torch.float64, device=_dev())
    info = torch.full((4,), -1, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    for _ in range(calls):
        eng.mlp_adam_sn_device(w, gt, mt, vt, st, betas=betas, sn=cap, sigma=sig, info=info, install=install)
    eng.synchronize()
    assert np.array_equal(gt.cpu().numpy().view(np.uint32), np.asarray(g, dtype=np.float32).view(np.uint32))
    return dict(p=w.cpu().numpy(), m=mt.cpu().numpy(), v=vt.cpu().numpy(), step=int(st.item()), sigma=sig.cpu().numpy(),
                info=info.cpu().numpy())


def _hold(tag, dev, ref, old):
    """The device's state against step64's: one ulp; the share of differing values printed."""
    shares = []
    for k in ("m", "v", "p"):
        u = T.ulps(dev[k], ref[k], old[k])
        shares.append(f"{k} {float((u > 0).mean()):.2e} (max {u.max():.2f} ulp)")
        assert np.isfinite(dev[k]).all(), (tag, k)
        assert u.max() <= 1.0, (tag, k, float(u.max()), int(np.argmax(u)))
    err = _sigma_err(dev["sigma"], T.sigmas64(dev["p"]))
    print(f"{tag}: share of values that differ: " + ", ".join(shares) + f"; sigma {dev['sigma']}, error {err.max():.1e}")
    assert dev["step"] == ref["step"]
    assert list(dev["info"]) == [ref["skipped"], ref["mask"], 0, 0], (tag, dev["info"])
    assert (err <= SIGMA_BAR).all(), (tag, err)


SETTINGS = {"nocap": ("shipped", 0.0, 0), "cap3": ("shipped", 3.0, 15), "mixed": ("mixed", 5.0, 5)}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("gfam", ["normal", "zero", "tiny", "tiny_fresh", "layer_zero"])
def test_one_step_from_an_arbitrary_state(eng, gfam, setting):
    family, cap, mask = SETTINGS[setting]
    blob = T.family(family)
    for step in (0, 1, 999, 10 ** 6):
        g, m, v, betas = _state(1000 + step % 997, gfam, blob)
        ref = T.step64(blob, g, m, v, step, betas=betas, cap=cap)             # (asserts every sigma clear of the cap)
        assert ref["mask"] == mask
        dev = _device_step(eng, blob, g, m, v, step, cap=cap, betas=betas)
        _hold(f"{setting} {gfam} step {step}", dev, ref, dict(p=blob, m=m, v=v))
        if gfam == "zero" and cap == 0.0:
            assert np.array_equal(dev["p"].view(np.uint32), blob.view(np.uint32)) and not dev["m"].any() and not dev["v"].any()
        if gfam.startswith("tiny"):                                          # subnormals survive the stores
            sub = (dev["v"] > 0) & (dev["v"] < np.finfo(np.float32).tiny)
            assert sub.mean() > 0.9 and np.array_equal(dev["v"] > 0, ref["v"] > 0)
        if cap > 0:
            assert (dev["sigma"] <= cap * (1.0 + T.REL_BAR)).all()
            off = mlp_frag.offsets()
            for b in ("b1", "b2", "b3", "b4"):                               # biases: Adam's value, never scaled
                o, shp = off[b]
                assert (T.ulps(dev["p"][o:o + shp[0]], T.adam64(blob, g, m, v, step, betas=betas)[0][o:o + shp[0]]) <= 1.0).all()


def test_two_calls_back_to_back_are_two_steps(eng):
    blob = T.family("shipped")
    g, m, v, betas = _state(7, "normal", blob)
    k, cap = 41, 3.0
    one = _device_step(eng, blob, g, m, v, k, cap=cap)
    two = _device_step(eng, blob, g, m, v, k, cap=cap, calls=2)
    again = _device_step(eng, blob, g, m, v, k, cap=cap, calls=2)
    assert one["step"] == k + 1 and two["step"] == k + 2
    for key in ("p", "m", "v", "sigma", "info"):
        assert np.array_equal(two[key], again[key]), key                      # a repeat from the same state is bit-identical
    ref = T.step64(one["p"], g, one["m"], one["v"], k + 1, cap=cap)           # the device's own intermediate state
    _hold("second of two", two, ref, one)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_gradient_skips_the_step(eng, bad):
    blob = T.family("shipped")
    g, m, v, _ = _state(9, "normal", blob)
    gb = g.copy()
    gb[-1] = bad                                                             # the last layer's bias: every workgroup has to find it
    dev = _device_step(eng, blob, gb, m, v, 17, cap=3.0)
    for key, old in (("p", blob), ("m", m), ("v", v)):
        assert np.array_equal(dev[key].view(np.uint32), old.view(np.uint32)), key
    assert dev["step"] == 17 and list(dev["info"]) == [1, 0, 0, 0]
    assert (_sigma_err(dev["sigma"], T.sigmas64(blob)) <= SIGMA_BAR).all()
    ref = T.step64(blob, gb, m, v, 17, cap=3.0)
    assert ref["skipped"] == 1 and ref["step"] == 17
    nxt = _device_step(eng, blob, g, m, v, 17, cap=3.0)                       # the next clean call proceeds normally
    _hold("after a skipped step", nxt, T.step64(blob, g, m, v, 17, cap=3.0), dict(p=blob, m=m, v=v))


def test_refused_hyperparameters_launch_nothing(eng, ndp):
    import torch
    blob = T.family("shipped")
    w, z = _t(blob), torch.zeros(NP, dtype=torch.float32, device=_dev())
    m, v, st = z.clone(), z.clone(), torch.zeros(1, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    for kw, why in ((dict(lr=float("inf")), "lr"), (dict(lr=float("nan")), "lr"), (dict(betas=(1.0, 0.999)), "beta"),
                    (dict(betas=(0.9, -0.1)), "beta"), (dict(eps=0.0), "eps")):
        with pytest.raises(ndp.batched.NdpError, match=why) as ei:
            eng.mlp_adam_sn_device(w, z + 1.0, m, v, st, **kw)
        assert "(-2)" in str(ei.value)
    eng.synchronize()
    assert int(st.item()) == 0 and not m.any() and np.array_equal(w.cpu().numpy(), blob)


def test_install_builds_the_host_forms_images(eng, ndp):
    blob = T.family("shipped")
    g, m, v, _ = _state(11, "normal", blob)
    assert T.step64(blob, g, m, v, 3, cap=3.0)["mask"] == 15                  # (asserts every sigma clear of the cap)
    fresh = ndp.BatchedNMPC(T.FIT_B, N=T.FIT_N, disturbance=True, load_mlp=False)
    try:
        for grad in (g, np.where(np.arange(NP) == 5, np.float32(np.nan), g)):      # also after a skipped step
            eng.set_mlp_weights(np.zeros(NP, dtype=np.float32))
            dev = _device_step(eng, blob, grad, m, v, 3, cap=3.0, install=True)
            assert dev["info"][0] == int(not np.isfinite(grad).all())
            fresh.set_mlp_weights(dev["p"])
            for a, b in zip(eng.debug_mlp_fragments(), fresh.debug_mlp_fragments()):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert np.array_equal(eng.debug_mlp_fragments()[0], mlp_frag.frag_words(dev["p"]))
    finally:
        fresh.close()
        eng.set_mlp_weights(blob)


def test_fit_through_the_optimiser(eng, ndp):
    """B = 4, N = 20, gates open, targets from the shipped blob, start = shipped (1 + 0.02 N(0, 1)); 40 steps of downwash -> MSE -> backward ->
    DownwashAdamSN(sn = 5) on a side stream.  tests/test_mlp_train.py runs the same fit on the float64 reference alone."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import DownwashAdamSN, downwash
    z, target, start = T.fit_case()
    other = torch.zeros(T.FIT_B, T.FIT_N + 1, 10, dtype=torch.float64, device=_dev())
    other[:, :, :6] = _t(z.reshape(T.FIT_B, T.FIT_N + 1, 6))
    ego = torch.zeros_like(other)
    tgt = _t(target.reshape(T.FIT_B, T.FIT_N + 1, 3).astype(np.float32))
    w = torch.nn.Parameter(_t(start))
    opt = DownwashAdamSN(w, eng, sn=T.FIT_CAP)
    side = torch.cuda.Stream(device=_dev())
    torch.cuda.synchronize()
    losses, sigmas = [], []
    with torch.cuda.stream(side):
        for it in range(T.FIT_STEPS):
            v0 = w._version
            loss = ((downwash(eng, other, ego, weights=w) - tgt) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            assert w._version > v0
            losses.append(loss.detach())
            sigmas.append(opt.state[w]["sigma"].clone())
        with torch.no_grad():
            f_last = downwash(eng, other, ego, weights=w)
            losses.append(((f_last - tgt) ** 2).mean())
    side.synchronize()
    eng.synchronize()
    losses = [float(x) for x in losses]
    sig = torch.stack(sigmas).cpu().numpy()
    st = opt.state[w]
    print(f"device fit: loss {losses[0]:.4e} -> {losses[-1]:.4e}, ratio {losses[-1] / losses[0]:.4f}; sigma max {sig.max(axis=0)}")
    assert int(st["step"].item()) == T.FIT_STEPS and list(st["info"].cpu().numpy()) == [0, 0, 0, 0]
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    T.assert_clear_of_cap(sig, T.FIT_CAP)                                    # (no step came near the branch)
    assert (sig > 0).all() and (sig <= T.FIT_CAP * (1.0 + T.REL_BAR)).all()
    assert losses[-1] != losses[-2]                                          # the forward after the last step is not the stale weights'
    fresh = ndp.BatchedNMPC(T.FIT_B, N=T.FIT_N, disturbance=True, load_mlp=False)
    try:
        fresh.set_mlp_weights(w.detach().cpu().numpy())
        f_host = fresh.downwash(other.cpu().numpy(), ego.cpu().numpy())
    finally:
        fresh.close()
        eng.set_mlp_weights(T.family("shipped"))
    assert np.array_equal(f_last.cpu().numpy().view(np.uint32), f_host.view(np.uint32))
    assert (_sigma_err(sig[-1], T.sigmas64(w.detach().cpu().numpy())) <= SIGMA_BAR).all()
