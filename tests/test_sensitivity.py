"""Initial-state sensitivities without a GPU: the numpy reference (tests/fixed_set_ref.py) against central differences of the dense KKT
solve, the device's sensitivity code (RtiWave::sens_out) on the host wave emulator against that reference, the torch layer's backward
and the acados facade's error paths.  The device side: tests/test_sensitivity_gpu.py."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests import ref_numpy as R
from tests.fixed_set_ref import scale, sens_ref
from tests.step_deriv_emu import MIXED, _emu_step, step_emu  # noqa: F401


def _qps(oracle, N, B, seed, f=False):
    b = synth.make_batch(B, N=N, seed=seed, **MIXED)
    cfg = oracle.default_cfg(N=N, use_fd=f)
    return b, cfg, [oracle.linearize(cfg, b["x0"][i], b["xr"][i], b["ur"][i], None, b["xr"][i], b["ur"][i]) for i in range(B)]


def test_sens_ref_matches_central_differences_of_the_kkt_solve(oracle):
    """The fixed-set derivative is the homogeneous problem's solution: against (kkt_solve(dx0 + h e_j) - kkt_solve(dx0 - h e_j)) / 2h
    with the same pins (held at their values), every column, with and without pins."""
    _, _, qps = _qps(oracle, 20, 2, synth.SEED0 + 3)
    for qp in qps:
        N = qp["A"].shape[0]
        for act in (None, np.eye(N, 4, dtype=np.int8)[:, ::-1] * np.int8(1)):
            fixed = [] if act is None else [((N + 1) * 10 + 4 * k + i, 0.3 * (k % 3 - 1)) for k, i in zip(*np.nonzero(act))]
            du0, dU, dX = sens_ref(qp, act)
            h = 1e-3
            for j in range(10):
                qa, qb = dict(qp), dict(qp)
                qa["dx0"] = qp["dx0"] + h * np.eye(10)[j]
                qb["dx0"] = qp["dx0"] - h * np.eye(10)[j]
                xa, ua = R.kkt_solve(qa, fixed)[:2]
                xb, ub = R.kkt_solve(qb, fixed)[:2]
                s = scale(dU)
                assert np.max(np.abs((ua - ub) / (2 * h) - dU[:, :, j])) <= 1e-7 * s
                assert np.max(np.abs((xa - xb) / (2 * h) - dX[:, :, j])) <= 1e-7 * max(1.0, np.max(np.abs(dX)))
            assert np.array_equal(du0, dU[0]) and np.array_equal(dX[0], np.eye(10))
            if act is not None:
                assert not dU[act != 0].any()


# ---------------------------------------------------------------- the sensitivity sweep on the host wave emulator
@pytest.mark.parametrize("N,B", [(20, 8), (13, 4)])
def test_emulated_sensitivity_sweep_matches_the_fixed_set_reference(oracle, step_emu, N, B):
    """The device's wave program with sensitivities (level 2) on the host emulator, mixed workload (inputs on their bounds): du0, dU
    and dX against sens_ref of the QP at the pre-step iterate with the step's final set, to 1e-10 of max(1, |K|max); pinned rows exactly
    0; dX_0 = I; level 1 writes the same du0 and nothing else."""
    from tests.emu import emu
    b, _, qps = _qps(oracle, N, B, synth.SEED0 + 40)
    cfg = emu.default_cfg(N=N)
    pinned = 0
    for i in range(B):
        X, U = b["xr"][i].copy(), b["ur"][i].copy()
        act = np.zeros(4 * N, dtype=np.int8)
        u0, _, _, st, it, act, du0, dU, dX = _emu_step(step_emu, cfg, 2, b["x0"][i], b["xr"][i], b["ur"][i], X, U, act)
        assert st == 0 and it & 0xffff == 0
        A = act.reshape(N, 4)
        pinned += int(A.any())
        r0, rU, rX = sens_ref(qps[i], A)
        s = scale(rU)
        assert np.max(np.abs(du0 - r0)) <= 1e-10 * s
        assert np.max(np.abs(dU - rU)) <= 1e-10 * s
        assert np.max(np.abs(dX - rX)) <= 1e-10 * max(1.0, np.max(np.abs(rX)))
        assert np.array_equal(dX[0], np.eye(10)) and not dU[A != 0].any() and np.array_equal(du0, dU[0])
        # level 1: the same du0, the level-2 outputs untouched
        X1, U1 = b["xr"][i].copy(), b["ur"][i].copy()
        a1 = np.zeros(4 * N, dtype=np.int8)
        u01, _, _, _, _, _, d1, dU1, dX1 = _emu_step(step_emu, cfg, 1, b["x0"][i], b["xr"][i], b["ur"][i], X1, U1, a1)
        assert np.array_equal(d1, du0) and np.array_equal(u01, u0) and (dU1 == -7.0).all() and (dX1 == -7.0).all()
    assert pinned >= 1


def test_emulated_nan_state_gives_nan_sensitivities(step_emu):
    from tests.emu import emu
    b = synth.make_batch(1, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg()
    x0 = b["x0"][0].copy()
    x0[3] = np.nan
    X, U = b["xr"][0].copy(), b["ur"][0].copy()
    _, _, _, st, _, _, du0, dU, dX = _emu_step(step_emu, cfg, 2, x0, b["xr"][0], b["ur"][0], X, U, np.zeros(80, dtype=np.int8))
    assert st != 0 and np.isnan(du0).all() and np.isnan(dU).all() and np.isnan(dX).all()


# ---------------------------------------------------------------- the torch layer's backward
class _StubEngine:
    """update_device writes u0 = K0 x0 + c; device_sensitivity returns K0 (CPU tensors: the layer's math without a device)."""

    def __init__(self, K0, c):
        self.K0, self.c, self.sensitivity_level, self.calls = K0, c, 1, 0

    def update_device(self, x0, xr, ur, u0, f=None, other=None, ego_xy=None, stream=None):
        import torch
        self.calls += 1
        u0.copy_(torch.bmm(self.K0, x0.unsqueeze(2)).squeeze(2) + self.c)

    def device_sensitivity(self):
        return self.K0, None, None


def test_torch_layer_backward_is_k0_transpose_times_the_output_gradient():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step
    g = torch.Generator().manual_seed(5)
    B = 16
    K0 = torch.randn(B, 4, 10, generator=g, dtype=torch.float64)
    eng = _StubEngine(K0, torch.randn(B, 4, generator=g, dtype=torch.float64))
    x0 = torch.randn(B, 10, generator=g, dtype=torch.float64, requires_grad=True)
    xr, ur = torch.zeros(B, 21, 10, dtype=torch.float64), torch.zeros(B, 20, 4, dtype=torch.float64)
    u0 = control_step(eng, x0, xr, ur)
    gu = torch.randn(B, 4, generator=g, dtype=torch.float64)
    (gx,) = torch.autograd.grad(u0, x0, gu)
    ref = np.einsum("bij,bi->bj", K0.numpy(), gu.numpy())
    assert np.allclose(gx.numpy(), ref, rtol=1e-14, atol=1e-14) and eng.calls == 1
    # a reference that requires grad is refused, not silently given a zero gradient
    with pytest.raises(ValueError, match="xr requires grad"):
        control_step(eng, x0, xr.clone().requires_grad_(True), ur)
    eng.sensitivity_level = 0
    with pytest.raises(ValueError, match="sensitivities are off"):
        control_step(eng, x0, xr, ur)


# ---------------------------------------------------------------- the acados facade
class _FacadeEngine:
    N = 20

    def get_iterate(self):
        return np.zeros((1, 21, 10)), np.zeros((1, 20, 4))


def test_facade_sensitivity_calls_say_how_to_enable_them():
    from ndp_nmpc_qd_amd.solver_facade import SolverFacade
    s = SolverFacade(_FacadeEngine(), disturbance=False)
    with pytest.raises(Exception, match="param_sens=True"):
        s.eval_param_sens(0)
    with pytest.raises(Exception, match="param_sens=True"):
        s.get(0, "sens_x")
    with pytest.raises(Exception, match="not supported"):
        s.get(0, "sens_pi")


def test_facade_sensitivity_shapes_and_argument_checks():
    from ndp_nmpc_qd_amd.solver_facade import SolverFacade

    class Eng(_FacadeEngine):
        level = 0

        def enable_sensitivity(self, level):
            self.level = level

        def sensitivity(self):
            dU = np.arange(20 * 40, dtype=float).reshape(1, 20, 4, 10)
            dX = np.arange(21 * 100, dtype=float).reshape(1, 21, 10, 10)
            return dU[:, 0], dU, dX

    e = Eng()
    s = SolverFacade(e, disturbance=False, param_sens=True)
    assert e.level == 2
    with pytest.raises(Exception, match="eval_param_sens"):
        s.get(0, "sens_u")
    for bad in (dict(index=10), dict(index=0, field="p"), dict(index=0, stage=1)):
        with pytest.raises(Exception):
            s.eval_param_sens(**bad)
    s.eval_param_sens(3)
    su, sx = s.get(5, "sens_u"), s.get(20, "sens_x")
    assert su.shape == (4,) and sx.shape == (10,)
    assert np.array_equal(su, np.arange(20 * 40).reshape(20, 4, 10)[5, :, 3])
    assert np.array_equal(sx, np.arange(21 * 100).reshape(21, 10, 10)[20, :, 3])
    with pytest.raises(Exception):
        s.get(20, "sens_u")


def test_sensitivity_kernels_use_no_scratch():
    """Every rti_sens_kernel instantiation (the nine the supported shapes need) keeps its state in registers: no scratch."""
    from ndp_nmpc_qd_amd import _lib, build, isa_inspect
    build.build()
    k = {n: v for n, v in isa_inspect.CodeObject(_lib.LIB_PATH).kernels().items() if "rti_sens_kernel" in n}
    assert len(k) == 9 and all(v["scratch"] == 0 for v in k.values()), k
