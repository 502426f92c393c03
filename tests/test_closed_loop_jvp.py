"""The one-call forward mode of the closed loop (ndp_closed_loop_jvp_device), CPU side: the interface (header, binding, interface version),
the tangent link kernel's code-object properties, the torch layer's `closed_loop_jvp` on a stub engine, and that the device comparison at
another model NOTICES that model: closed_loop_chain_ref.forward at the default model lies at least NOTICE = 100 bars from the one at
tests/plant_side_cases.py's LOOP_CASE on the same record (tests/test_plant_side_envelope.py's convention).
Device side: tests/test_closed_loop_jvp_gpu.py.

The export takes 24 arguments: the handle, ticks, dt, substeps, eight primal pointers (x0, xr, ur, f, fp, xs, us, tape), n_tan, five
directions, five outputs and the stream -- the signature as the header states it."""
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import build, isa_inspect as I
from tests import closed_loop_chain_ref as R
from tests import closed_loop_jvp_cases as J
from tests import plant_side_cases as C
from tests.test_closed_loop_chain_gpu import BAR
from tests.test_closed_loop_vjp import _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL, KERNEL = "ndp_closed_loop_jvp_device", "closed_loop_tan_link_kernel"


def test_the_export_is_declared_and_bound():
    from ndp_nmpc_qd_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "ndp_nmpc.h")) as fh:
        hdr = fh.read()
    assert SYMBOL in _lib.EXPORTS and getattr(lib, SYMBOL).argtypes is not None
    m = re.search(r"\bint %s\(ndp_handle \*h, int ticks,([^;]*)\);" % SYMBOL, hdr)
    assert m and m.group(1).count(",") + 3 == len(lib.ndp_closed_loop_jvp_device.argtypes) == 24
    assert len(lib.ndp_closed_loop_device.argtypes) == 15 and len(lib.ndp_closed_loop_vjp_device.argtypes) == 23
    m = re.search(r"#define NDP_ABI_VERSION (\d+)", hdr)
    assert m and int(m.group(1)) == 9 and _lib.ABI_VERSION == 9 and lib.ndp_abi_version() == 9


def test_the_tangent_link_kernel_keeps_its_state_in_registers():
    """Exactly one kernel of that name: no scratch, no spill, no LDS, at most 256 registers, in the code object of its two siblings."""
    co = I.CodeObject(build.build())
    k = co.kernels()
    found = [n for n in k if KERNEL in n]
    assert len(found) == 1, found
    v = k[found[0]]
    assert v["scratch"] == 0 and v["spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, v
    assert v["vgpr"] + v["agpr"] <= 256, v
    for part in ("closed_loop_fwd_link_kernel", "closed_loop_rev_link_kernel"):
        sib = [n for n in k if part in n]
        assert len(sib) == 1 and co.code_object_of(sib[0]) == co.code_object_of(found[0]), part


# ---- the torch layer on a stub engine
class _StubJ(_Stub):
    def closed_loop_jvp_device(self, x0, xr, ur, xs, us, tape, dxs, dus, f=None, fp=None, tx0=None, txr=None, tur=None, tf=None, tfp=None,
                               dXs=None, dUs=None, status_check=None, n_tan=None, dt=None, substeps=None, stream=None):
        self.calls.append(("jvp", dict(x0=x0, xr=xr, ur=ur, xs=xs.clone(), us=us.clone(), tape=tape, f=f, fp=fp, t=(tx0, txr, tur, tf, tfp),
                                       n_tan=n_tan, dt=dt, substeps=substeps, stream=stream, dUs=dUs, status_check=status_check)))
        dxs[:] = 1.0 if tx0 is None else tx0[None] * 2.0
        dus[:] = 2.0 if tur is None else tur[:, :, :, 0, :]
        dXs[:] = 3.0 if txr is None else txr


def test_torch_closed_loop_jvp_on_a_stub_engine():
    """One forward call with a tape, then one forward-mode call on its xs, us and tape: detached contiguous float64 directions, f as
    given, dt and substeps passed on; the T axis kept when any direction has it and dropped when none has; a disagreement on T and no
    direction at all raise, with plant_rollout_jvp's texts."""
    torch = pytest.importorskip("torch")
    from ndp_nmpc_qd_amd import torch_layer as TL
    K, B, N, T = 3, 4, 5, 2
    g = torch.Generator().manual_seed(5)
    mk = lambda *s, dt=torch.float64: torch.randn(*s, generator=g, dtype=dt)  # noqa: E731
    eng = _StubJ(B, N)
    x0, xr, ur = mk(B, 10).requires_grad_(), mk(K, B, N + 1, 10), mk(K, B, N, 4)
    f, fp = mk(K, B, N + 1, 3, dt=torch.float32), mk(K, B, 3)
    tx0, txr, tur, tf, tfp = mk(B, T, 10), mk(K, B, T, N + 1, 10), mk(K, B, T, N, 4), mk(K, B, T, N + 1, 3, dt=torch.float32), mk(K, B, T, 3)
    out = TL.closed_loop_jvp(eng, x0, xr, ur, (tx0.requires_grad_(), txr, tur.transpose(0, 1).contiguous().transpose(0, 1), tf, tfp),
                             f=f, fp=fp, dt=0.02, substeps=2)
    assert [c[0] for c in eng.calls] == ["fwd", "jvp"]
    fw, jv = eng.calls[0][1], eng.calls[1][1]
    assert fw["dt"] == jv["dt"] == 0.02 and fw["substeps"] == jv["substeps"] == 2 and fw["tape"] is jv["tape"] and (jv["tape"] == 7).all()
    assert jv["f"].dtype == torch.float32 and not jv["x0"].requires_grad and jv["n_tan"] == T and jv["stream"] is None
    assert jv["dUs"] is None and jv["status_check"] is None
    assert torch.equal(jv["xs"], (x0.detach()[None] + 1.0).expand(K, B, 10)) and torch.equal(jv["us"], ur[:, :, 0, :])
    for got, want, shape in zip(jv["t"], (tx0, txr, tur, tf, tfp), ((B, T, 10), (K, B, T, N + 1, 10), (K, B, T, N, 4), (K, B, T, N + 1, 3), (K, B, T, 3))):
        assert got.dtype == torch.float64 and got.is_contiguous() and not got.requires_grad and tuple(got.shape) == shape
        assert torch.equal(got, want.detach().to(torch.float64))
    xs, us, Xs, dxs, dus, dXs = out
    assert tuple(xs.shape) == (K, B, 10) and tuple(us.shape) == (K, B, 4) and torch.equal(Xs, xr)
    assert tuple(dxs.shape) == (K, B, T, 10) and tuple(dus.shape) == (K, B, T, 4) and tuple(dXs.shape) == (K, B, T, N + 1, 10)
    assert torch.equal(dxs, (tx0.detach()[None] * 2.0).expand(K, B, T, 10)) and torch.equal(dus, tur[:, :, :, 0, :]) and torch.equal(dXs, txr)
    assert not dxs.requires_grad
    # no direction has the T axis: handed over with T = 1, returned without it; the others NULL
    eng.calls.clear()
    out = TL.closed_loop_jvp(eng, x0, xr, ur, (tx0[:, 0], None, tur[:, :, 0], None, None))
    jv = eng.calls[1][1]
    assert jv["n_tan"] == 1 and tuple(jv["t"][0].shape) == (B, 1, 10) and tuple(jv["t"][2].shape) == (K, B, 1, N, 4)
    assert jv["t"][1] is None and jv["t"][3] is None and jv["t"][4] is None and jv["f"] is None and jv["fp"] is None
    assert tuple(out[3].shape) == (K, B, 10) and tuple(out[4].shape) == (K, B, 4) and tuple(out[5].shape) == (K, B, N + 1, 10)
    assert torch.equal(out[3], (tx0[:, 0].detach()[None] * 2.0).expand(K, B, 10)) and torch.equal(out[4], tur[:, :, 0, 0, :])
    # one with the axis and one without: both are handed over with it (T = 1), and the outputs keep it
    out = TL.closed_loop_jvp(eng, x0, xr, ur, (tx0[:, :1], None, None, None, tfp[:, :, 0]))
    assert tuple(eng.calls[-1][1]["t"][4].shape) == (K, B, 1, 3) and tuple(out[3].shape) == (K, B, 1, 10)
    n_calls = len(eng.calls)
    with pytest.raises(ValueError, match="closed_loop_jvp: the tangents disagree on the number of directions"):
        TL.closed_loop_jvp(eng, x0, xr, ur, (tx0, txr[:, :, :1], None, None, None))
    with pytest.raises(ValueError, match=r"closed_loop_jvp: no tangent \(all None\)"):
        TL.closed_loop_jvp(eng, x0, xr, ur, (None,) * 5)
    with pytest.raises(ValueError, match="closed_loop_jvp: a tangent has 2 dimensions, expected 3 or 4"):
        TL.closed_loop_jvp(eng, x0, xr, ur, (None, None, None, None, tfp[:, :, 0, 0]))
    assert len(eng.calls) == n_calls                       # a refused call reaches the engine with nothing


# ---- the other model is noticed
def test_the_forward_sweep_at_the_loop_model_lies_100_bars_from_the_default_models(oracle):
    """N = 20, LOOP_CASE's record and referenced six: closed_loop_chain_ref.forward with the systems built at the DEFAULT model on the same
    record and directions differs from the one at LOOP_CASE by at least NOTICE bars in dxs, dus and dXs each, in the device comparison's
    own measure (rel_err with lead 3, bar BAR["ext"]) -- a link that folded a default 1 / m or default weights misses the device test
    by two orders of magnitude.  The reference's own forward / reverse duality gap at this model is printed (the device test's per-vehicle
    bar is built on it)."""
    N = 20
    a, rec, ok, which, ups = C.loop_record(oracle, N)
    cfg, dflt = C.loop_cfg(oracle, N), oracle.default_cfg(N=N, use_fd=True)
    assert len(which) == 6 and ok[which].all()
    t = J.directions(C.LOOP_K, C.B, N, 2)
    sys1, sys0 = (R.systems(oracle, rec, which, cfg=c) for c in (cfg, dflt))
    here, there = J.reference(sys1, rec, t), J.reference(sys0, rec, t)
    for n, v in J.errors(there, here).items():
        print(f"{n}: the default twin lies {v / BAR['ext']:.3g} bars away")
        assert v >= C.NOTICE * BAR["ext"], (n, v)
    gap = J.reference_gap(sys1, rec, t, ups)
    print("the reference's own duality gap per referenced vehicle: " + " ".join(f"{v}: {x:.2e}" for v, x in zip(which, gap)))
    assert np.isfinite(gap).all() and gap.max() <= C.LOOP_K * 1e-10     # (absolute; the two sweeps are one composition read both ways)
