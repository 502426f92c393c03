"""The adjoint of the control step (RtiWave::vjp_out) without a GPU: the device's code on the host wave emulator against the dense fixed-set
KKT reference (tests/fixed_set_ref.py) for random upstream gradients on (u0, X, U), against the parameter sensitivities (the emulator's psens_emu_step) for an
upstream on u0 alone -- interior-point finishes included --, the recompute against the step, and the kernels' ISA.  The device side:
tests/test_step_vjp_gpu.py."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests.fixed_set_ref import scale, vjp_ref
from tests.step_deriv_emu import MIXED, _psens, _tape, _vjp, step_emu  # noqa: F401


@pytest.mark.parametrize("N,B,use_fd,as_iter_max", [(2, 4, False, None), (13, 4, True, None), (20, 6, False, None), (27, 3, True, None),
                                                    (20, 3, False, 0)])
def test_emulated_vjp_matches_the_dense_fixed_set_reference(oracle, step_emu, N, B, use_fd, as_iter_max):
    """Random (gu0, gX, gU) on mixed instances (inputs on their bounds among them; as_iter_max = 0: the early exit of rounds 1-5 or the
    interior point): every active-set / early-exit finish within 1e-10 of max(1, |g|max) of vjp_ref at the step's final set; stage 0's
    reference row and f_N exactly 0, pinned inputs' rows exactly 0."""
    from tests.emu import emu
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 60 + N, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd, as_iter_max=as_iter_max)
    ocfg = oracle.default_cfg(N=N, use_fd=use_fd)
    rng = np.random.default_rng(N)
    checked = pinned = 0
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = rng.normal(0.0, 0.3, (N + 1, 3)).astype(np.float32) if use_fd else None
        gu0, gX, gU = rng.normal(size=4), rng.normal(size=(N + 1, 10)), rng.normal(size=(N, 4))
        u0, Xn, Un, st, it, actn, gx0, gxr, gur, gf = _vjp(step_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act, gu0, gX, gU)
        assert st == 0
        if it & 0xffff:                                  # interior point: its last Newton system (test_gu0_only_...)
            continue
        A = actn.reshape(N, 4)
        pinned += int(A.any())
        ref = vjp_ref(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], None if f is None else f.astype(np.float64), X, U, A, gu0, gX, gU)
        s = max(scale(r) for r in ref)
        for got, r in zip((gx0, gxr, gur, gf), ref):
            assert np.max(np.abs(got - r)) <= 1e-10 * s, (i, np.max(np.abs(got - r)) / s)
        assert not gxr[0].any() and not gf[N].any() and not gur[A != 0].any()
        checked += 1
    assert checked >= 2
    if N in (13, 20) and as_iter_max is None:
        assert pinned >= 1


@pytest.mark.parametrize("N,use_fd,ipm", [(20, False, False), (13, True, False), (20, False, True), (13, True, True)])
def test_gu0_only_is_the_parameter_sensitivities_contracted(step_emu, N, use_fd, ipm):
    """An upstream on u0 alone: gx0 = K0' gu0, gxr / gur / gf = gu0 contracted with psens_emu_step's du0/dxr, du0/dur, du0/df, within 1e-12 of
    max(1, |g|max) for free and pinned finishes; interior-point ones (ipm: qp_mode 1, the velocity box shrunk to +-3) within 1e-6: both
    solve the last Newton system, whose barrier terms on an active velocity bound reach 1e10 -- they agree to ~1e-13 on most instances and
    to ~1e-7 on the stiffest.  The recompute IS the step: u0, X, U, status, iteration word and
    kept set bit-equal to psens_emu_step's."""
    from tests.emu import emu
    B = 6
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 70 + N, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd, qp_mode=1 if ipm else 0)
    if ipm:
        for j in range(3):
            cfg.lbv[j], cfg.ubv[j] = -3.0, 3.0
    rng = np.random.default_rng(5)
    n_ipm = 0
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = rng.normal(0.0, 0.3, (N + 1, 3)).astype(np.float32) if use_fd else None
        gu0 = rng.normal(size=4)
        a = _vjp(step_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act, gu0=gu0)
        p = _psens(step_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        for x, y in zip(a[:6], p[:6]):
            assert np.array_equal(x, y)
        if a[3] != 0:
            assert all(np.isnan(g).all() for g in a[6:])
            continue
        in_ipm = (a[4] & 0xffff) > 0
        n_ipm += int(in_ipm)
        du0, dxr, dur, df = p[6:]
        ref = (du0.T @ gu0, np.einsum("i,ikj->kj", gu0, dxr), np.einsum("i,ikj->kj", gu0, dur), np.einsum("i,ikj->kj", gu0, df))
        s = max(scale(r) for r in ref)
        for got, r in zip(a[6:], ref):
            assert np.max(np.abs(got - r)) <= (1e-6 if in_ipm else 1e-12) * s, (i, np.max(np.abs(got - r)) / s)
    if ipm:
        assert n_ipm >= 3


def test_emulated_nan_state_gives_nan_gradients(step_emu):
    from tests.emu import emu
    N = 20
    b = synth.make_batch(1, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg()
    x0 = b["x0"][0].copy()
    x0[3] = np.nan
    out = _vjp(step_emu, cfg, x0, b["xr"][0], b["ur"][0], None, b["xr"][0], b["ur"][0], np.zeros(4 * N, dtype=np.int8), gu0=np.ones(4))
    assert out[3] != 0 and all(np.isnan(g).all() for g in out[6:])


def test_vjp_kernels_use_no_scratch():
    """Both rti_vjp_kernel instantiations (N = 20 and the run-time horizon) keep their state in registers, and lie in one code object."""
    from ndp_nmpc_qd_amd import _lib, build, isa_inspect
    build.build()
    k = {n: v for n, v in isa_inspect.CodeObject(_lib.LIB_PATH).kernels().items() if "rti_vjp_kernel" in n}
    assert len(k) == 2 and all(v["scratch"] == 0 for v in k.values()), k
