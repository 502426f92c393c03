"""The handle's bookkeeping (run with -m gpu): whatever an engine acquires from the HIP runtime over its life -- device buffers, page-locked
blocks, events, streams -- is back when it is closed.  ndp_debug_live_resources counts the live owners (csrc/hip_own.hpp) of the whole
process; the test reads it before anything exists, lets an engine touch every lazily acquired resource once, closes it and expects the
starting value exactly, three times over.  Bookkeeping, not numerics: the inputs are the hover reference (synth.hover_reference) seen
from a few centimetres off, B = 5 (a ragged last workgroup of 4 instances) at N = 7 (a run-time horizon), and every step must end with
status 0."""
import gc

import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, synth
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401

pytestmark = pytest.mark.gpu

B, N, K, TICKS = 5, 7, 2, 2


def _live():
    gc.collect()            # (an engine an earlier test dropped without close() goes now, not between two readings)
    return int(_lib.load().ndp_debug_live_resources())


def _hover():
    xh, uh = synth.hover_reference(N)
    xr, ur = np.tile(xh, (B, 1, 1)), np.tile(uh, (B, 1, 1))
    xr[:, :, 0] += 1.5 * np.arange(B)[:, None]                  # the vehicles 1.5 m apart along x
    x0 = xr[:, 0, :].copy()
    x0[:, 0:3] += 0.03 * np.array([1.0, -1.0, 0.5]) * (1 + np.arange(B))[:, None] / B
    return dict(x0=x0, xr=xr, ur=ur)


def _ok(eng):
    eng.synchronize()
    st, _ = eng.status()
    assert not st.any(), st


def _touch_everything(ndp, eng, b):
    """One use of every lazily acquired resource of the handle; every step status 0."""
    import torch
    dev = _dev()
    z = lambda *s, dtype=torch.float64: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
    t = {k: _t(v) for k, v in b.items()}
    u0 = z(B, 4)
    # the host-array step: the slots' page-locked mirrors, their events, the pack pool
    eng.reset(b["xr"], b["ur"])
    _, _, _, st, _ = eng.update(b["x0"], b["xr"], b["ur"], full=True)
    assert not st.any()
    # the sensitivity buffers, both kinds, on and off again
    eng.enable_sensitivity(2)
    _, _, _, st, _ = eng.update(b["x0"], b["xr"], b["ur"], full=True)
    assert not st.any()
    eng.enable_param_sensitivity()
    assert eng.param_sensitivity_enabled
    eng.enable_param_sensitivity(False)
    eng.enable_sensitivity(0)
    # a recorded step and its adjoint: the recompute workspace
    tape = eng.record_tape()
    torch.cuda.synchronize()
    eng.update_device(t["x0"], t["xr"], t["ur"], u0)
    _ok(eng)
    gx0, stc = z(B, 10), z(B, dtype=torch.int32)
    eng.step_vjp_device(t["x0"], t["xr"], t["ur"], tape, gu0=torch.ones_like(u0), gx0=gx0, status_check=stc)
    eng.synchronize()
    assert not stc.cpu().numpy().any()
    # the closed loop with a tape, and its reverse mode: the link workspace
    xrs, urs = t["xr"].expand(TICKS, -1, -1, -1).contiguous(), t["ur"].expand(TICKS, -1, -1, -1).contiguous()
    xs, us, fps, stk = z(TICKS, B, 10), z(TICKS, B, 4), z(TICKS, B, 3), z(TICKS, B, dtype=torch.int32)
    cl_tape = eng.closed_loop_tape(TICKS)
    eng.closed_loop_device(t["x0"], xrs, urs, xs, us, status=stk, tape=cl_tape)
    eng.synchronize()
    assert not stk.cpu().numpy().any()
    eng.closed_loop_vjp_device(t["x0"], xrs, urs, xs, us, cl_tape, gxs=torch.ones_like(xs), gx0=gx0, status_check=stk)
    eng.synchronize()
    assert not stk.cpu().numpy().any()
    # the formation: its index block (K = 2), the loop, the reverse mode with the weight gradient (the formation workspace), then no formation
    index = np.stack([(np.arange(B) + 1) % B, (np.arange(B) + 2) % B], axis=1).astype(np.int32)
    eng.closed_loop_formation_config(index)
    eng.closed_loop_formation_device(t["x0"], xrs, urs, xs, us, fps, status=stk, tape=cl_tape)
    eng.synchronize()
    assert not stk.cpu().numpy().any()
    gw = z(_lib.MLP_NPARAM, dtype=torch.float32)
    eng.closed_loop_formation_vjp_device(t["x0"], xrs, urs, xs, us, fps, cl_tape, gxs=torch.ones_like(xs), gx0=gx0, gw=gw, status_check=stk)
    eng.synchronize()
    assert not stk.cpu().numpy().any()
    eng.closed_loop_formation_config(None)
    # the trajectory block, allocated twice (another segment count), the reference list and a window of it
    for n_seg in (4, 6):
        tr = synth.figure_eight_traj(B, n_seg=n_seg)
        eng.ref_set_trajectory(*(tr[k] for k in ("coeff_x", "coeff_y", "coeff_z", "coeff_yaw", "time_cum", "time_seg", "final_pt")))
    eng.ref_list_reset()
    xw, uw = eng.ref_list_window()
    assert np.isfinite(xw).all() and np.isfinite(uw).all()
    # the tick's thrust and index buffers, with and without an index
    eng.tick_config((np.arange(B) + 1) % B)
    eng.tick_config(None)
    # the downwash one tick ahead: the second stream, its fork and join events, the force slots and protocol words
    other = t["xr"].roll(1, 0).contiguous()
    ego_xy, side = t["x0"][:, 0:2].contiguous(), torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    eng.downwash_prefetch_device(other, t["xr"], ego_xy=ego_xy, after_stream=side)
    eng.prefetch_join()
    eng.synchronize()
    assert eng.prefetch_stats()["predictions"] == 1
    # the stamps' buffer, on then off
    eng.debug_stamps(True)
    eng.debug_stamps(False)
    # the timing events of one timed step
    eng.reset(b["xr"], b["ur"])
    eng.timing_enable(1)
    eng.update_device(t["x0"], t["xr"], t["ur"], u0)
    _ok(eng)
    assert eng.timing_read("rti")[1] == 1
    # the completion events of tracked steps
    eng.track_steps(True)
    eng.update_device(t["x0"], t["xr"], t["ur"], u0)
    _ok(eng)
    assert eng.last_step_event().value
    torch.cuda.synchronize()


def test_three_lives_leave_nothing_behind(ndp):
    start = _live()
    b = _hover()
    for life in range(3):
        eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
        created = _live()
        assert created > start, (life, start, created)
        _touch_everything(ndp, eng, b)
        assert _live() > created, life            # (the lazily acquired ones are counted too)
        eng.close()
        assert _live() == start, (life, start, _live())


def test_two_engines_closed_in_creation_order(ndp):
    """Two engines alive at once: the first one's end takes nothing of the second's -- it still steps, status 0, its u0 bit-equal to a
    fresh engine's on the same inputs -- and the counter is back at the start behind both."""
    start = _live()
    b = _hover()

    def step(eng):
        eng.reset(b["xr"], b["ur"])
        u0, _, _, st, _ = eng.update(b["x0"], b["xr"], b["ur"], full=True)
        assert not st.any()
        return u0

    first = ndp.BatchedNMPC(B, N=N, disturbance=True)
    one = _live()
    second = ndp.BatchedNMPC(B, N=N, disturbance=True)
    assert _live() > one > start
    step(first)
    first.close()
    assert _live() > start
    u_second = step(second)
    second.close()
    assert _live() == start
    fresh = ndp.BatchedNMPC(B, N=N, disturbance=True)
    u_fresh = step(fresh)
    fresh.close()
    assert _live() == start
    assert u_second.view(np.int64).tolist() == u_fresh.view(np.int64).tolist()
