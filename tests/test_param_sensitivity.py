"""Parameter sensitivities (du0/dxr, du0/dur, du0/df) without a GPU: the numpy reference (tests/fixed_set_ref.py) against central differences
of the whole linearise-and-KKT-solve, the device's code (RtiWave::psens_out) on the host wave emulator against that reference, the
translation identity that ties them to du0/dx0, and the torch layer's backward.  The device side: tests/test_param_sensitivity_gpu.py."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests import ref_numpy as R
from tests.fixed_set_ref import fixed_of, psens_ref, scale
from tests.step_deriv_emu import MIXED, _psens, step_emu  # noqa: F401


def test_psens_ref_matches_central_differences_of_linearise_and_solve(oracle):
    """Every parameter of a few entries of each kind: (u0(theta + h) - u0(theta - h)) / 2h of oracle.linearize + kkt_solve with the same
    pins, against psens_ref, with and without pins and with a force."""
    N = 20
    b = synth.make_batch(2, N=N, seed=synth.SEED0 + 3, **MIXED)
    rng = np.random.default_rng(7)
    c1 = oracle.default_cfg(N=N, use_fd=True)      # (use_fd off is the same QP as on with f = 0)
    for i, use_fd in ((0, False), (1, True)):
        cfg = oracle.default_cfg(N=N, use_fd=use_fd)
        x0, xr, ur = b["x0"][i], b["xr"][i], b["ur"][i]
        f = rng.normal(0.0, 0.5, (N + 1, 3)) if use_fd else None
        f0 = np.zeros((N + 1, 3)) if f is None else f
        X, U = xr + 0.01 * rng.normal(size=xr.shape), ur + 0.01 * rng.normal(size=ur.shape)
        for act in (None, np.eye(N, 4, dtype=np.int8)[:, ::-1].copy()):
            dxr, dur, df = psens_ref(oracle, cfg, x0, xr, ur, f, X, U, act)

            def u0_of(xr_, ur_, f_):
                qp = oracle.linearize(c1, x0, xr_, ur_, f_, X, U)
                return R.kkt_solve(qp, fixed_of(qp, act))[1][0]

            h = 1e-4
            for (k, j) in ((1, 0), (5, 4), (7, 7), (N, 9), (0, 2)):
                d = np.zeros_like(xr)
                d[k, j] = h
                fd = (u0_of(xr + d, ur, f0) - u0_of(xr - d, ur, f0)) / (2 * h)
                assert np.max(np.abs(fd - dxr[:, k, j])) <= 1e-7 * scale(dxr), (k, j)
            for (k, j) in ((0, 1), (3, 3), (N - 1, 0)):
                d = np.zeros_like(ur)
                d[k, j] = h
                fd = (u0_of(xr, ur + d, f0) - u0_of(xr, ur - d, f0)) / (2 * h)
                assert np.max(np.abs(fd - dur[:, k, j])) <= 1e-7 * scale(dur), (k, j)
            for (k, j) in ((0, 0), (4, 2), (N - 1, 1), (N, 2)):
                d = np.zeros_like(f0)
                d[k, j] = h
                fd = (u0_of(xr, ur, f0 + d) - u0_of(xr, ur, f0 - d)) / (2 * h)
                assert np.max(np.abs(fd - df[:, k, j])) <= 1e-7 * scale(df), (k, j)
            # stage 0's reference (x0 is fixed) and f_N (no dynamics) do not move u0: rounding only
            assert np.max(np.abs(dxr[:, 0])) <= 1e-13 * scale(dxr) and np.max(np.abs(df[:, N])) <= 1e-13 * scale(df)
            if act is not None:
                assert not dxr[act[0] != 0].any() and not dur[act[0] != 0].any() and not df[act[0] != 0].any()


# ---------------------------------------------------------------- the device program on the host wave emulator
@pytest.mark.parametrize("N,B,use_fd", [(20, 8, False), (13, 4, False), (20, 3, True)])
def test_emulated_param_sensitivities_match_the_fixed_set_reference(oracle, step_emu, N, B, use_fd):
    """RtiWave::psens_out on the host emulator (N = 20: the compile-time horizon; 13: the run-time form), mixed workload with inputs on
    their bounds: du0/dxr, du0/dur, du0/df against psens_ref of the QP at the pre-step iterate with the step's final set, to 1e-10 of
    max(1, |J|max); stage 0's reference rows and f_N exactly 0; pinned stage-0 rows exactly 0; and the translation identity
    du0/dx0[:, 0:3] + sum_k du0/dxr[:, k, 0:3] = 0 (a common shift of x0 and every reference position leaves the QP as it is)."""
    from tests.emu import emu
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd)
    ocfg = oracle.default_cfg(N=N, use_fd=use_fd)
    rng = np.random.default_rng(11)
    pinned = 0
    for i in range(B):
        X, U = b["xr"][i].copy(), b["ur"][i].copy()
        f = rng.normal(0.0, 0.3, (N + 1, 3)).astype(np.float32) if use_fd else None
        act = np.zeros(4 * N, dtype=np.int8)
        u0, _, _, st, _, act, du0, dxr, dur, df = _psens(step_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        assert st == 0
        A = act.reshape(N, 4)
        pinned += int(A.any())
        rx, ru, rf = psens_ref(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], None if f is None else f.astype(np.float64),
                               b["xr"][i], b["ur"][i], A)
        for got, ref in ((dxr, rx), (dur, ru), (df, rf)):
            assert np.max(np.abs(got - ref)) <= 1e-10 * scale(ref)
        assert not dxr[:, 0].any() and not df[:, N].any()
        assert not dxr[A[0] != 0].any() and not dur[A[0] != 0].any() and not df[A[0] != 0].any()
        assert np.max(np.abs(du0[:, 0:3] + dxr[:, :, 0:3].sum(axis=1))) <= 1e-10 * max(1.0, np.max(np.abs(du0)))
    assert pinned >= 1


def test_emulated_nan_state_gives_nan_param_sensitivities(step_emu):
    from tests.emu import emu
    b = synth.make_batch(1, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg()
    x0 = b["x0"][0].copy()
    x0[3] = np.nan
    X, U = b["xr"][0].copy(), b["ur"][0].copy()
    _, _, _, st, _, _, du0, dxr, dur, df = _psens(step_emu, cfg, x0, b["xr"][0], b["ur"][0], None, X, U, np.zeros(80, dtype=np.int8))
    assert st != 0 and np.isnan(du0).all() and np.isnan(dxr).all() and np.isnan(dur).all() and np.isnan(df).all()


# ---------------------------------------------------------------- the torch layer's backward
class _StubEngine:
    """update_device writes u0 = K0 x0 + sum(Jxr xr) + sum(Jur ur) + sum(Jf f) + c; the sensitivity getters return the J's (CPU
    tensors: the layer's math without a device)."""

    def __init__(self, K0, Jxr, Jur, Jf, c, params=True):
        self.K0, self.Jxr, self.Jur, self.Jf, self.c = K0, Jxr, Jur, Jf, c
        self.sensitivity_level, self.param_sensitivity_enabled, self.calls = 1, params, 0

    def update_device(self, x0, xr, ur, u0, f=None, other=None, ego_xy=None, stream=None):
        import torch
        self.calls += 1
        u = torch.bmm(self.K0, x0.unsqueeze(2)).squeeze(2) + self.c
        u = u + torch.einsum("bikj,bkj->bi", self.Jxr, xr) + torch.einsum("bikj,bkj->bi", self.Jur, ur)
        if f is not None:
            u = u + torch.einsum("bikj,bkj->bi", self.Jf, f.to(torch.float64))
        u0.copy_(u)

    def device_sensitivity(self):
        return self.K0, None, None

    def device_param_sensitivity(self):
        return self.Jxr, self.Jur, self.Jf


def test_torch_layer_parameter_gradients_are_the_output_gradient_contracted_with_the_sensitivities():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step
    g = torch.Generator().manual_seed(5)
    B, N = 8, 20
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    eng = _StubEngine(r(B, 4, 10), r(B, 4, N + 1, 10), r(B, 4, N, 4), r(B, 4, N + 1, 3), r(B, 4))
    x0 = r(B, 10).requires_grad_(True)
    xr, ur = r(B, N + 1, 10).requires_grad_(True), r(B, N, 4).requires_grad_(True)
    f = torch.randn(B, N + 1, 3, generator=g, dtype=torch.float32).requires_grad_(True)
    u0 = control_step(eng, x0, xr, ur, f=f)
    gu = r(B, 4)
    gx, gxr, gur, gf = torch.autograd.grad(u0, (x0, xr, ur, f), gu)
    assert gf.dtype == torch.float32 and gxr.dtype == torch.float64 and eng.calls == 1
    assert np.allclose(gx.numpy(), np.einsum("bij,bi->bj", eng.K0.numpy(), gu.numpy()), rtol=1e-14, atol=1e-14)
    for got, J in ((gxr, eng.Jxr), (gur, eng.Jur)):
        assert np.allclose(got.numpy(), np.einsum("bi,bikj->bkj", gu.numpy(), J.numpy()), rtol=1e-14, atol=1e-14)
    assert np.allclose(gf.numpy(), np.einsum("bi,bikj->bkj", gu.numpy(), eng.Jf.numpy()).astype(np.float32), rtol=1e-6, atol=1e-6)
    # only what requires grad gets a gradient; x0 alone is still fine
    u1 = control_step(eng, x0, xr.detach(), ur.detach())
    (g1,) = torch.autograd.grad(u1, x0, gu)
    assert np.allclose(g1.numpy(), gx.numpy(), rtol=1e-14, atol=1e-14)


def test_torch_layer_refusals_hold_without_parameter_sensitivities():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step
    B, N = 2, 20
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    eng = _StubEngine(z(B, 4, 10), z(B, 4, N + 1, 10), z(B, 4, N, 4), z(B, 4, N + 1, 3), z(B, 4), params=False)
    x0 = z(B, 10).requires_grad_(True)
    for name in ("xr", "ur", "f"):
        kw = dict(xr=z(B, N + 1, 10), ur=z(B, N, 4), f=torch.zeros(B, N + 1, 3))
        kw[name] = kw[name].requires_grad_(True)
        with pytest.raises(ValueError, match=f"{name} requires grad"):
            control_step(eng, x0, kw["xr"], kw["ur"], f=kw["f"])
    del eng.param_sensitivity_enabled                       # an engine without the attribute: the same
    with pytest.raises(ValueError, match="xr requires grad"):
        control_step(eng, x0, z(B, N + 1, 10).requires_grad_(True), z(B, N, 4))
    eng2 = _StubEngine(z(B, 4, 10), z(B, 4, N + 1, 10), z(B, 4, N, 4), z(B, 4, N + 1, 3), z(B, 4), params=True)
    for name in ("other", "ego_xy"):                       # the fused network's inputs are never differentiated
        kw = dict(other=None, ego_xy=None)
        kw[name] = z(B, N + 1, 10).requires_grad_(True)
        with pytest.raises(ValueError, match=f"{name} requires grad"):
            control_step(eng2, x0, z(B, N + 1, 10), z(B, N, 4), **kw)


def test_param_sensitivity_kernels_use_no_scratch():
    """Every rti_psens_kernel instantiation (the seven the served shapes need) keeps its state in registers: no scratch."""
    from ndp_nmpc_qd_amd import _lib, build, isa_inspect
    build.build()
    k = {n: v for n, v in isa_inspect.CodeObject(_lib.LIB_PATH).kernels().items() if "rti_psens_kernel" in n}
    assert len(k) == 7 and all(v["scratch"] == 0 for v in k.values()), k
