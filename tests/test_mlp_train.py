"""Training the downwash network, CPU side: the exports and their bindings, properties of the kernels' ISA, the float64 reference
(tests/mlp_train_ref.py) held to torch.optim.Adam and to the cap's bound, the device test's 40-step fit run on the reference alone, and the
optimiser's bookkeeping on a stub engine.  GPU side: tests/test_mlp_train_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag
from tests import mlp_train_ref as T
from tests import mlp_vjp_ref as R
from tests.test_downwash_vjp import _StubNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ndp_nmpc.h")).read()
    lib = _lib.load()
    for name, nargs in (("ndp_mlp_spectral_norms_device", 4), ("ndp_mlp_spectral_norms", 3), ("ndp_mlp_adam_sn_device", 15)):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs
    fn = lib.ndp_mlp_adam_sn_device
    assert all(fn.argtypes[i] is C.c_double for i in range(6, 11)) and fn.argtypes[13] is C.c_int      # lr .. sn_cap, install
    # a null handle is refused before anything is touched
    assert lib.ndp_mlp_spectral_norms_device(None, None, None, None) == -1
    assert lib.ndp_mlp_spectral_norms(None, None, None) == -1
    assert fn(None, None, None, None, None, None, 1e-4, 0.9, 0.999, 1e-8, 4.0, None, None, 1, None) == -1
    m = re.search(r"#define\s+NDP_ABI_VERSION\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == lib.ndp_abi_version() == 9
    from ndp_nmpc_qd_amd.batched import BatchedNMPC
    assert all(callable(getattr(BatchedNMPC, n)) for n in ("mlp_spectral_norms", "mlp_spectral_norms_device", "mlp_adam_sn_device"))
    from ndp_nmpc_qd_amd import build
    assert "mlp_train.hip" in build.UNITS and "mlp_train.hip" not in build.HOST_ONLY


def test_train_kernels_isa_properties():
    """The two instantiations of mlp_train_kernel (norms only; Adam + cap) sit alone in a code object of their own, use no scratch and
    spill nothing, form the Gram matrix on the f64 matrix instruction, and only the optimiser step has a global atomic (its ticket)."""
    from ndp_nmpc_qd_amd import build, isa_inspect
    build.build()
    co = isa_inspect.CodeObject(_lib.LIB_PATH)
    k = co.kernels()
    train = sorted(n for n in k if "mlp_train_kernel" in n)
    assert len(train) == 2, train
    homes = {co.code_object_of(n) for n in train}
    assert len(homes) == 1
    assert sorted(n for n in k if co.code_object_of(n) in homes) == train          # nothing else lives there
    for n in train:
        assert k[n]["scratch"] == 0 and k[n]["spill"] == 0 and k[n]["sgpr_spill"] == 0, (n, k[n])
        assert 0 < k[n]["lds"] <= 64 * 1024
        ins = co.disassemble(n)
        assert sum(s.startswith("v_mfma_f64_16x16x4") for s in ins) >= 4, n
        atomics = [s for s in ins if re.match(r"(global|flat|buffer)_atomic", s)]
        assert bool(atomics) == ("ILb1E" in n), (n, atomics)


def test_adam64_is_torch_adam():
    """adam64 without its float32 rounding points against torch.optim.Adam on the CPU in float64: one step from a random state at step
    0, 1, 999 and 10^6, to 1e-12 of the largest parameter."""
    import torch
    rng = np.random.default_rng(31)
    n = 257
    for step in (0, 1, 999, 10 ** 6):
        p0, g, m0 = rng.normal(size=n), rng.normal(size=n), 0.1 * rng.normal(size=n)
        v0 = rng.uniform(0.0, 1.0, size=n) ** 2
        p = torch.nn.Parameter(torch.tensor(p0))
        opt = torch.optim.Adam([p], lr=1e-4)
        opt.state[p] = dict(step=torch.tensor(float(step)), exp_avg=torch.tensor(m0), exp_avg_sq=torch.tensor(v0))
        p.grad = torch.tensor(g)
        opt.step()
        pn, mn, vn = T.adam64(p0, g, m0, v0, step, round32=False)
        st = opt.state[p]
        assert float(st["step"]) == step + 1
        for got, want in ((pn, p.detach().numpy()), (mn, st["exp_avg"].numpy()), (vn, st["exp_avg_sq"].numpy())):
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), step
        assert np.abs(pn - p0).max() > 1e-6                                       # (the step moved something)
    # the rounding points: m, v, p are float32, and p is a function of the ROUNDED m and v
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    p32, m32, v32 = T.adam64(f32(p0), f32(g), f32(m0), f32(v0), 5)
    assert p32.dtype == m32.dtype == v32.dtype == np.float32
    m64, v64 = m32.astype(np.float64), v32.astype(np.float64)
    want = f32(f32(p0).astype(np.float64) - 1e-4 / (1.0 - 0.9 ** 6) * (m64 / (np.sqrt(v64) / np.sqrt(1.0 - 0.999 ** 6) + 1e-8)))
    assert np.array_equal(p32, want)


@pytest.mark.parametrize("cap", [3.5, 4.5, 0.5])      # (no family has a layer within 1e-6 of these)
def test_project64_keeps_sigma_under_the_bar(cap):
    for name in T.FAMILIES:
        blob = T.family(name)
        out, mask, before = T.project64(blob, cap)
        after = T.sigmas64(out)
        assert mask == sum(1 << l for l in range(4) if before[l] > cap), name
        assert (after <= cap * (1.0 + T.REL_BAR)).all(), (name, after)
        off = mlp_frag.offsets()
        for b in ("b1", "b2", "b3", "b4"):                                        # biases are never scaled
            o, shp = off[b]
            assert np.array_equal(out[o:o + shp[0]], blob[o:o + shp[0]])
        for l, (W0, W1) in enumerate(zip(T.weights(blob), T.weights(out))):
            if not mask >> l & 1:
                assert np.array_equal(W0, W1), (name, l)
            else:
                assert not np.array_equal(W0, W1) and abs(after[l] / cap - 1.0) <= T.REL_BAR, (name, l)


def test_families_are_what_they_claim():
    sv = lambda W: np.linalg.svd(W.astype(np.float64), compute_uv=False)  # noqa: E731
    s = T.sigmas64(T.family("shipped"))
    assert np.abs(s - [3.99999928, 3.99999565, 4.00002304, 3.99999944]).max() < 1e-8
    for cap in (3.0, 5.0):
        T.assert_clear_of_cap(s, cap)
    for W in T.weights(T.family("equal")):
        assert np.ptp(sv(W)) <= 1e-5
    for W in T.weights(T.family("cluster")):
        top = sv(W)[:min(8, min(W.shape))]
        assert np.ptp(top) <= 1e-5 and top[0] > 2.99
    for W in T.weights(T.family("rank1")):
        assert sv(W)[1] <= 1e-6 and abs(sv(W)[0] - 5.0) < 1e-5
    assert not any(W.any() for W in T.weights(T.family("zero")))
    for W in T.weights(T.family("wide")):
        assert abs(sv(W)[0] - 1e3) < 1e-2
    sm = T.sigmas64(T.family("mixed"))
    assert sm[0] > 300 and sm[2] > 300 and sm[1] < 0.05 and sm[3] < 0.05


def test_the_reference_alone_meets_the_fit_tests_conditions():
    """The 40-step fit of tests/test_mlp_train_gpu.py with step64 on the float64 network (tests/mlp_vjp_ref.py): the loss falls, every
    sigma stays under the bar after every step."""
    z, target, start = T.fit_case()
    p = start.copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    losses = []
    for step in range(T.FIT_STEPS + 1):
        f = R.vjp64(p, z, np.zeros_like(target))[3]
        losses.append(float(((f - target) ** 2).mean()))
        if step == T.FIT_STEPS:
            break
        gw = R.vjp64(p, z, 2.0 * (f - target) / target.size)[1].astype(np.float32)
        s = T.step64(p, gw, m, v, step, cap=T.FIT_CAP)
        p, m, v = s["p"], s["m"], s["v"]
        assert not s["skipped"] and (s["sigma"] <= T.FIT_CAP * (1.0 + T.REL_BAR)).all()
    print(f"reference fit: loss {losses[0]:.4e} -> {losses[-1]:.4e}, ratio {losses[-1] / losses[0]:.4f}")
    assert losses[-1] < losses[0]


# ---------------------------------------------------------------- the optimiser's bookkeeping
class _StubTrain(_StubNet):
    """_StubNet with an optimiser step that writes through the parameter's MEMORY (w -= lr g, step += 1), as the kernel does: the tensor's
    version counter does not move."""

    def __init__(self, B, N):
        super().__init__(B, N)
        self.calls = []

    def mlp_adam_sn_device(self, w, g, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, sn=0.0, sigma=None, info=None, install=False,
                           stream=None):
        self.calls.append(dict(lr=lr, betas=betas, eps=eps, sn=sn, install=install, stream=stream))
        w.numpy()[...] -= lr * g.numpy()
        m.numpy()[...] = g.numpy()
        step.numpy()[...] += 1
        sigma.numpy()[...] = [1.0 + 2.0 ** -40, 2.0, 3.0, 4.0]                   # (not a float32 value: the round trip must keep it)
        info.numpy()[...] = [0, 5, 0, 0]
        if install:
            self._mlp_installed = None


def _stub_case(install):
    import torch
    B, N = 3, 20
    eng = _StubTrain(B, N)
    g = torch.Generator().manual_seed(8)
    other, ego = (torch.randn(B, N + 1, 10, generator=g, dtype=torch.float64) for _ in range(2))
    p = torch.nn.Parameter(torch.zeros(17859, dtype=torch.float32))
    from ndp_nmpc_qd_amd.torch_layer import DownwashAdamSN
    return eng, other, ego, p, DownwashAdamSN(p, eng, lr=0.5, sn=4.0, install=install)


@pytest.mark.parametrize("install", [True, False])
def test_step_bumps_the_version_and_settles_who_installs(install):
    import torch
    from ndp_nmpc_qd_amd.torch_layer import downwash
    eng, other, ego, p, opt = _stub_case(install)
    downwash(eng, other, ego, weights=p)
    assert eng.installed == 1
    p.grad = torch.ones_like(p)
    v0 = p._version
    opt.step()
    assert p._version > v0 and torch.equal(p.detach(), torch.full_like(p, -0.5))
    c = eng.calls[-1]
    assert (c["lr"], c["sn"], c["install"], c["betas"], c["eps"]) == (0.5, 4.0, install, (0.9, 0.999), 1e-8)
    downwash(eng, other, ego, weights=p)
    assert eng.installed == (1 if install else 2)             # the step installed them itself / the forward sees new weights
    downwash(eng, other, ego, weights=p)
    assert eng.installed == (1 if install else 2)
    opt.step()
    downwash(eng, other, ego, weights=p)
    assert eng.installed == (1 if install else 3)
    assert int(opt.state[p]["step"]) == 2


def test_state_dict_round_trips_with_its_dtypes():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import DownwashAdamSN
    eng, _, _, p, opt = _stub_case(True)
    p.grad = torch.arange(17859, dtype=torch.float32)
    opt.step()
    sd = opt.state_dict()
    st = opt.state[p]
    assert {k: t.dtype for k, t in st.items()} == DownwashAdamSN._DTYPES
    assert st["step"].shape == (1,) and st["sigma"].shape == (4,) and st["info"].shape == (4,)
    p2 = torch.nn.Parameter(p.detach().clone())
    opt2 = DownwashAdamSN(p2, eng)
    opt2.load_state_dict(sd)
    st2 = opt2.state[p2]
    assert set(st2) == set(st)
    for k in st:
        assert st2[k].dtype == st[k].dtype and torch.equal(st2[k], st[k]) and st2[k].data_ptr() != st[k].data_ptr(), k
    assert float(st2["sigma"][0]) == 1.0 + 2.0 ** -40
    g = opt2.param_groups[0]
    assert (g["lr"], g["sn"], g["install"]) == (0.5, 4.0, True)
    p2.grad = torch.ones_like(p2)
    opt2.step()
    assert int(st2["step"]) == 2 and int(st["step"]) == 1
    with pytest.raises(ValueError, match="ONE contiguous float32 parameter"):
        DownwashAdamSN(torch.nn.Parameter(torch.zeros(10)), eng)
    with pytest.raises(ValueError, match="betas"):
        DownwashAdamSN(p, eng, betas=(1.0, 0.999))
