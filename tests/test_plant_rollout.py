"""The plant over an input sequence (ndp_plant_rollout_device and its reverse / forward mode), what can be held without a GPU: the float64
reference the GPU tests compare against (tests/plant_deriv_ref.py) against the oracle's plant step and against finite differences, and
the shipped library's interface and code objects."""
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import build, isa_inspect as I
from ndp_nmpc_qd_amd.params import nmpc_params as CP
from tests import plant_deriv_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("plant_rollout_kernel", "plant_rollout_vjp_kernel", "plant_rollout_jvp_kernel")
SYMBOLS = ("ndp_plant_rollout_device", "ndp_plant_rollout_vjp_device", "ndp_plant_rollout_jvp_device")


@pytest.mark.parametrize("force", [True, False])
def test_reference_forward_is_the_oracle_plant_step_tick_by_tick(oracle, force):
    cfg = oracle.default_cfg()
    x0, u, f = P.inputs(6, 5, seed=3, force=force)
    xs = P.rollout(x0, u, f, CP.ts_nmpc, 4, cfg.mass, cfg.g)
    x = x0.copy()
    for k in range(5):
        x = oracle.plant_step(cfg, x.copy(), u[k].copy(), f[k].copy() if force else np.zeros((6, 3)), CP.ts_nmpc, 4)
        np.testing.assert_allclose(xs[k], x, rtol=0, atol=1e-13)            # the plant bar of tests/test_relay_and_plant_rows.py


def test_reference_jacobian_against_central_differences():
    """Complex step against central differences with step 1e-6 on a few columns of each input: O(h^2) + eps / h ~ 1e-9, bar 1e-7."""
    B, ticks, sub, h = 3, 3, 4, 1e-6
    x0, u, f = P.inputs(B, ticks, seed=5)
    J = P.jacobian(x0, u, f, substeps=sub)
    assert J.shape == (B, ticks * 10, P.n_in(ticks))
    worst = 0.0
    for col in (0, 4, 6, 9, 10, 13, 10 + 4 * 1 + 2, 10 + 4 * ticks, 10 + 4 * ticks + 3 * 2 + 1):
        def at(step):
            a, b, c = x0.copy(), u.copy(), f.copy()
            if col < 10:
                a[:, col] += step
            elif col < 10 + 4 * ticks:
                b[(col - 10) // 4, :, (col - 10) % 4] += step
            else:
                c[(col - 10 - 4 * ticks) // 3, :, (col - 10 - 4 * ticks) % 3] += step
            return P.rollout(a, b, c, substeps=sub)
        fd = (at(h) - at(-h)) / (2 * h)                                      # [ticks, B, 10]
        err = np.abs(fd.transpose(1, 0, 2).reshape(B, ticks * 10) - J[:, :, col]).max()
        worst = max(worst, err)
    print("complex step - central differences, worst:", worst)
    assert worst < 1e-7


def test_reference_jacobian_is_causal_and_blind_along_the_quaternion():
    """A tick's input moves no earlier state; and the output quaternion's own direction lies in the left null space of every tick's block
    (q / |q| has no component along q)."""
    B, ticks = 2, 3
    x0, u, f = P.inputs(B, ticks, seed=6)
    J = P.jacobian(x0, u, f)
    xs = P.rollout(x0, u, f)
    for k in range(ticks):
        later_u = J[:, k * 10:(k + 1) * 10, 10 + 4 * (k + 1):10 + 4 * ticks]
        later_f = J[:, k * 10:(k + 1) * 10, 10 + 4 * ticks + 3 * (k + 1):]
        assert not later_u.any() and not later_f.any()
        along = np.einsum("bq,bqi->bi", xs[k][:, 6:], J[:, k * 10 + 6:(k + 1) * 10, :])
        assert np.abs(along).max() < 1e-13


def test_vjp_and_jvp_of_the_reference_are_dual():
    B, ticks, T = 2, 2, 3
    x0, u, f = P.inputs(B, ticks, seed=7)
    J = P.jacobian(x0, u, f)
    rng = np.random.default_rng(8)
    g = rng.normal(size=(ticks, B, 10))
    tx0, tu, tf = rng.normal(size=(B, T, 10)), rng.normal(size=(ticks, B, T, 4)), rng.normal(size=(ticks, B, T, 3))
    gx0, gu, gf = P.vjp(J, g)
    d = P.jvp(J, tx0, tu, tf)
    for t in range(T):
        lhs = (d[:, :, t] * g).sum()
        rhs = (gx0 * tx0[:, t]).sum() + (gu * tu[:, :, t]).sum() + (gf * tf[:, :, t]).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


# ---- the shipped library
@pytest.fixture(scope="module")
def co():
    return I.CodeObject(build.build())


def test_lib_exposes_the_three_entry_points(co):
    from ndp_nmpc_qd_amd import _lib
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    with open(os.path.join(ROOT, "include", "ndp_nmpc.h")) as fh:
        hdr = fh.read()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(ndp_handle \*h, int ticks, double dt, int substeps," % name, hdr), name
    assert re.search(r"#define NDP_PLANT_MAX_SUBSTEPS 16\b", hdr) and _lib.PLANT_MAX_SUBSTEPS == 16


def test_the_additions_leave_the_interface_version_alone():
    from ndp_nmpc_qd_amd import _lib
    with open(os.path.join(ROOT, "include", "ndp_nmpc.h")) as fh:
        m = re.search(r"#define NDP_ABI_VERSION (\d+)", fh.read())
    assert m and int(m.group(1)) == 9 and _lib.ABI_VERSION == 9
    assert _lib.load().ndp_abi_version() == 9


def test_plant_rollout_kernels_keep_their_state_in_registers(co):
    """One lane per vehicle and a long serial chain: no scratch memory (so no dynamically indexed private array survived), no LDS, and a
    register count that still leaves two waves per SIMD."""
    k = co.kernels()
    home = set()
    for part in KERNELS:
        found = [n for n in k if part in n]
        assert len(found) == 1, (part, found)
        v = k[found[0]]
        assert v["scratch"] == 0 and v["spill"] == 0 and v["lds"] == 0, (part, v)
        assert v["vgpr"] <= 256, (part, v)
        home.add(co.code_object_of(found[0]))
    assert len(home) == 1                                   # csrc/plant_deriv.hip's code object
    assert len([n for n in k if "plant_kernel" in n]) == 1  # the step's kernel stays where it was (rows.hip)
