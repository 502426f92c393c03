"""The control step's gradient in its cost weights and the mass (RtiWave::vjp_out<true>, rti_wvjp_kernel) without a GPU: the device's code
on the host wave emulator (tests/step_deriv_emu.cpp) against the dense fixed-set KKT reference (tests/fixed_set_ref.py), the scale identity, the
interior-point finishes beside the existing adjoint's, a failed step, the kernels' ISA and the header / ABI.  The device side:
tests/test_model_grad_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests.fixed_set_ref import NU, NX, model_grad_ref, scale, vjp_ref
from tests.step_deriv_emu import MIXED, _tape, _vjp, step_emu  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("N,B,use_fd,as_iter_max", [(2, 4, False, None), (13, 4, True, None), (20, 6, False, None), (27, 3, True, None),
                                                    (20, 3, False, 0)])
def test_emulated_model_gradient_matches_the_dense_fixed_set_reference(oracle, step_emu, N, B, use_fd, as_iter_max):
    """The shapes of test_emulated_vjp_matches_the_dense_fixed_set_reference, random (gu0, gX, gU): on every active-set / early-exit finish
    all 15 numbers within 1e-10 of max(1, |g|max) of model_grad_ref at the step's final set; gmodel[6] and gmodel[15] exactly 0, gmodel[14]
    exactly 0 without a force; the reference's two step sizes in 1 / m agree to 1e-9; the scale identity sum Qd gQd + sum Rd gRd = 0 within
    1e-10 of max(1, max |Qd g|); the other outputs bit-equal to vjp_emu_step's."""
    from tests.emu import emu
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 60 + N, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd, as_iter_max=as_iter_max)
    ocfg = oracle.default_cfg(N=N, use_fd=use_fd)
    w = np.array(list(cfg.Qd) + list(cfg.Rd))
    assert np.array_equal(w, np.array(list(ocfg.Qd) + list(ocfg.Rd))) and cfg.mass == ocfg.mass
    rng = np.random.default_rng(N)
    checked = pinned = 0
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = rng.normal(0.0, 0.3, (N + 1, 3)).astype(np.float32) if use_fd else None
        gu0, gX, gU = rng.normal(size=4), rng.normal(size=(N + 1, 10)), rng.normal(size=(N, 4))
        a = _vjp(step_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act, gu0, gX, gU, model=True)
        p = _vjp(step_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act, gu0, gX, gU)
        assert _same(a[:10], p)
        st, it, actn, gm = a[3], a[4], a[5], a[10]
        assert st == 0
        assert gm[6] == 0.0 and gm[15] == 0.0
        if not use_fd:
            assert gm[14] == 0.0
        if it & 0xffff:                                  # interior point: test_interior_point_finishes_...
            continue
        A = actn.reshape(N, 4)
        pinned += int(A.any())
        ref, gm2 = model_grad_ref(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], None if f is None else f.astype(np.float64), X, U, A,
                                  gu0, gX, gU)
        s = scale(ref)
        assert abs(ref[14] - gm2) <= 1e-9 * s, (i, ref[14], gm2)
        err = np.max(np.abs(gm - ref))
        print(f"N={N} i={i} pinned={int(A.any())} err/scale={err / s:.3e} scale={s:.3e}")
        assert err <= 1e-10 * s, (i, err / s, gm, ref)
        wg = w * gm[:14]
        assert abs(wg.sum()) <= 1e-10 * max(1.0, float(np.max(np.abs(wg)))), (i, wg.sum())
        checked += 1
    assert checked >= 2
    if N in (13, 20) and as_iter_max is None:
        assert pinned >= 1


@pytest.mark.parametrize("N,use_fd", [(20, False), (13, True)])
def test_interior_point_finishes_are_as_close_to_the_pinned_reference_as_the_existing_adjoint(oracle, step_emu, N, use_fd):
    """qp_mode 1 with the velocity box shrunk to +-3 (test_gu0_only_is_the_parameter_sensitivities_contracted's instances): the interior
    point's last Newton system is barrier-smoothed, so no distance from the dense reference is fixed.  Measured instead: the reference pins
    the bounds that are active at the solution (within 1e-6), and gmodel's distance from it (of max(1, |g|max)) is at most 10 x the
    distance of the existing gxr output from the same reference on the same instances.
    Measured here (emulator): see DESIGN section 3, "Gradient in the cost weights and the mass"."""
    from tests.emu import emu
    B = 6
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 70 + N, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd, qp_mode=1)
    ocfg = oracle.default_cfg(N=N, use_fd=use_fd)
    for j in range(3):
        cfg.lbv[j], cfg.ubv[j] = -3.0, 3.0
        ocfg.lbv[j], ocfg.ubv[j] = -3.0, 3.0
    rng = np.random.default_rng(5)
    n_ipm = 0
    worst_m = worst_x = 0.0
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = rng.normal(0.0, 0.3, (N + 1, 3)).astype(np.float32) if use_fd else None
        gu0, gX, gU = rng.normal(size=4), rng.normal(size=(N + 1, 10)), rng.normal(size=(N, 4))
        a = _vjp(step_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act, gu0, gX, gU, model=True)
        if a[3] != 0 or not (a[4] & 0xffff):
            continue
        n_ipm += 1
        Xn, Un = a[1].reshape(N + 1, NX), a[2].reshape(N, NU)
        f64 = None if f is None else f.astype(np.float64)
        qp = oracle.linearize(ocfg, b["x0"][i], b["xr"][i], b["ur"][i], f64 if use_fd else None, X, U)
        lbu, ubu, lbv, ubv = (np.array(list(v)) for v in (cfg.lbu, cfg.ubu, cfg.lbv, cfg.ubv))
        pins = []
        for k in range(N):
            for j in range(NU):
                if abs(Un[k, j] - ubu[j]) < 1e-6 or abs(Un[k, j] - lbu[j]) < 1e-6:
                    pins.append(((N + 1) * NX + NU * k + j, float(qp["uu"][k, j] if abs(Un[k, j] - ubu[j]) < 1e-6 else qp["lu"][k, j])))
        for k in range(1, N + 1):
            for j in range(3):
                if abs(Xn[k, 3 + j] - ubv[j]) < 1e-6 or abs(Xn[k, 3 + j] - lbv[j]) < 1e-6:
                    pins.append((k * NX + 3 + j, float(qp["uv"][k, j] if abs(Xn[k, 3 + j] - ubv[j]) < 1e-6 else qp["lv"][k, j])))
        ref, _ = model_grad_ref(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], f64, X, U, None, gu0, gX, gU, pin_v=pins)
        gxr = vjp_ref(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], f64, X, U, None, gu0, gX, gU, pin_v=pins)[1]
        dm = np.max(np.abs(a[10] - ref)) / scale(ref)
        dx = np.max(np.abs(a[7] - gxr)) / scale(gxr)
        print(f"N={N} i={i} pins={len(pins)} gmodel distance {dm:.3e}  gxr distance {dx:.3e}")
        worst_m, worst_x = max(worst_m, dm), max(worst_x, dx)
    print(f"N={N}: worst gmodel distance {worst_m:.3e}, worst gxr distance {worst_x:.3e}")
    assert n_ipm >= 3
    assert worst_m <= 10.0 * worst_x, (worst_m, worst_x)


def test_emulated_failed_step_gives_nan_in_all_16(step_emu):
    from tests.emu import emu
    N = 20
    b = synth.make_batch(1, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg()
    x0 = b["x0"][0].copy()
    x0[3] = np.nan
    out = _vjp(step_emu, cfg, x0, b["xr"][0], b["ur"][0], None, b["xr"][0], b["ur"][0], np.zeros(4 * N, dtype=np.int8), gu0=np.ones(4), model=True)
    assert out[3] != 0 and all(np.isnan(g).all() for g in out[6:])
    assert out[10].shape == (16,)


def test_wvjp_kernels_use_no_scratch_and_leave_the_adjoint_kernels_alone():
    """Both rti_wvjp_kernel instantiations (N = 20 and the run-time horizon) exist in the library's one code object and keep their state in
    registers; rti_vjp_kernel still has exactly its two."""
    from ndp_nmpc_qd_amd import _lib, build, isa_inspect
    build.build()
    ks = isa_inspect.CodeObject(_lib.LIB_PATH).kernels()
    k = {n: v for n, v in ks.items() if "rti_wvjp_kernel" in n}
    assert len(k) == 2 and all(v["scratch"] == 0 for v in k.values()), k
    assert len([n for n in ks if "rti_vjp_kernel" in n]) == 2


def test_header_declares_the_new_entries_and_the_abi_agrees():
    from ndp_nmpc_qd_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ndp_nmpc.h")).read()
    assert re.search(r"\bint\s+ndp_set_model\s*\(", hdr) and re.search(r"\bint\s+ndp_step_vjp_model_device\s*\(", hdr)
    m = re.search(r"#define\s+NDP_ABI_VERSION\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == 9
    from ndp_nmpc_qd_amd import build
    build.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "ndp_set_model") and hasattr(lib, "ndp_step_vjp_model_device")
