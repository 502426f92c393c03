"""What the host side of the single / K-neighbour pairs and of the rollout families REFUSES (run with -m gpu): the return code, the complete
text left in ndp_last_error and the order in which refusals are tried, for every entry point of mlp_vjp.hip, mlp_jvp.hip, downwash.hip's
multi and plant-force forms, rows.hip's plant step and rollouts, plant_deriv.hip and closed_loop.hip.  The raw library functions are called
(e._lib, e._h, None for NULL); every argument set is one the library refuses, where two refusals apply both are sent so that their order
is pinned.  The expected texts are literals read off the source, not taken from the library.  Nothing is launched, so every output buffer
keeps its -7.0.  (A -1 leaves ndp_last_error as it was: the text in front of the call is expected behind it.)

Handles, batch 2, N = 3: `bare` has the NDP model and no weights (load_mlp=False); `nmpc` has the weights and the NMPC model
(disturbance=False), no trajectory; `sens` has initial-state sensitivities on.  All buffers are large enough for the call they are passed
to at K = 9, n_tan = 9, two ticks: a refusal that stopped refusing would compute garbage in bounds, not fault."""
import ctypes as C

import numpy as np
import pytest

from tests.deriv_gpu import _dev, ndp  # noqa: F401

pytestmark = pytest.mark.gpu

B, N, K = 2, 3, 2
SENTINEL = -7.0
GATE, COMPENSATE = 1, 2

SENS = (b": not available while initial-state sensitivities are enabled (ndp_sens_enable(h, 0) first): only the in-place and work-list step "
        b"forms compute them")
NO_MLP = b"downwash requested but ndp_set_mlp_weights was never called"


def _k_text(who, k):
    return who + b": K must be 1..8 (NDP_MAX_NEIGH neighbours per vehicle), got " + str(k).encode()


@pytest.fixture(scope="module")
def world(ndp):
    import torch
    bare = ndp.BatchedNMPC(B, N=N, disturbance=True, load_mlp=False)
    nmpc = ndp.BatchedNMPC(B, N=N, disturbance=False, load_mlp=True)
    sens = ndp.BatchedNMPC(B, N=N, disturbance=False)
    sens.enable_sensitivity(1)
    w = dict(bare=bare, nmpc=nmpc, sens=sens,
             zin=torch.zeros(1 << 16, dtype=torch.float64, device=_dev()),                   # every device input (as int32: index 0)
             out=torch.full((8, 1 << 14), SENTINEL, dtype=torch.float64, device=_dev()),      # row j: a call's j-th device output
             hin=np.zeros(1 << 12), hout=np.full(1 << 12, SENTINEL))                          # the host-array forms' input / output
    yield w
    for e in (bare, nmpc, sens):
        e.close()


def _refused(world, cases):
    """cases: (engine name, function name, arguments behind the handle, rc, complete text or None for 'as it was')."""
    import torch
    for i, (eng, fn, args, rc, text) in enumerate(cases):
        e = world[eng]
        L, h = e._lib, e._h
        before = L.ndp_last_error(h)
        got = getattr(L, fn)(h, *args)
        assert got == rc, (i, eng, fn, got, L.ndp_last_error(h))
        assert L.ndp_last_error(h) == (before if text is None else text), (i, eng, fn)
    for e in (world["bare"], world["nmpc"], world["sens"]):
        e.synchronize()
    torch.cuda.synchronize()
    assert bool((world["out"] == SENTINEL).all()) and (world["hout"] == SENTINEL).all()
    assert bool((world["zin"] == 0.0).all())


def test_downwash_vjp_single_and_multi(world):
    z = world["zin"].data_ptr()        # (no output buffer is ever passed: "no output" is the last refusal)
    s, m = "ndp_downwash_vjp_device", "ndp_downwash_multi_vjp_device"
    sw, mw = s.encode(), m.encode()
    # single: (other, stride, index, ego, ego_xy, gf, gz, gw, stream); multi: K behind the index
    _refused(world, [
        ("bare", s, (None, 7, z, z, z, None, None, None, None), -1, None),                  # NULL in front of everything else
        ("bare", s, (z, 7, z, None, z, None, None, None, None), -1, None),
        ("bare", s, (z, 7, z, z, z, None, None, None, None), -6, sw + b": ndp_set_mlp_weights was never called"),      # weights in front of the stride
        ("nmpc", s, (z, 7, z, z, z, None, None, None, None), -2, sw + b": other_stride must be 6 or 10"),              # stride in front of d_gf
        ("nmpc", s, (z, 10, z, z, z, None, None, None, None), -2, sw + b": d_gf is required (the upstream gradient of the force)"),   # d_gf in front of the outputs
        ("nmpc", s, (z, 6, None, z, None, z, None, None, None), -2, sw + b": no output asked for (d_gz and d_gw both NULL)"),
        ("bare", m, (None, 7, None, 0, z, z, None, None, None, None), -1, None),
        ("bare", m, (z, 7, None, 0, None, z, None, None, None, None), -1, None),
        ("bare", m, (z, 7, None, 0, z, z, None, None, None, None), -6, mw + b": ndp_set_mlp_weights was never called"),  # weights in front of K
        ("nmpc", m, (z, 7, None, 0, z, z, None, None, None, None), -2, mw + b": K must be 1..8 (NDP_MAX_NEIGH neighbours per vehicle)"),   # K in front of the index
        ("nmpc", m, (z, 7, None, 9, z, z, None, None, None, None), -2, mw + b": K must be 1..8 (NDP_MAX_NEIGH neighbours per vehicle)"),
        ("nmpc", m, (z, 7, None, K, z, z, None, None, None, None), -2, mw + b": d_other_index is required (int32 [B][K])"),             # index in front of the stride
        ("nmpc", m, (z, 7, z, K, z, z, None, None, None, None), -2, mw + b": other_stride must be 6 or 10"),
        ("nmpc", m, (z, 10, z, K, z, z, None, None, None, None), -2, mw + b": d_gf is required (the upstream gradient of the summed force)"),
        ("nmpc", m, (z, 6, z, K, z, None, z, None, None, None), -2, mw + b": no output asked for (d_gz and d_gw both NULL)"),
    ])


def test_downwash_jvp_single_and_multi(world):
    z, o = world["zin"].data_ptr(), [world["out"][j].data_ptr() for j in range(8)]
    s, m = "ndp_downwash_jvp_device", "ndp_downwash_multi_jvp_device"
    sw, mw = s.encode(), m.encode()
    # single: (other, stride, index, ego, ego_xy, n_tan, tz, tw, df, f_check, stream); multi: K behind the index
    _refused(world, [
        ("bare", s, (None, 7, z, z, z, 0, None, None, None, o[1], None), -1, None),
        ("bare", s, (z, 7, z, None, z, 0, None, None, None, o[1], None), -1, None),
        ("bare", s, (z, 7, z, z, z, 0, None, None, None, o[1], None), -6, sw + b": ndp_set_mlp_weights was never called"),
        ("nmpc", s, (z, 7, z, z, z, 0, None, None, None, o[1], None), -2, sw + b": other_stride must be 6 or 10"),     # stride in front of n_tan
        ("nmpc", s, (z, 10, z, z, z, 0, None, None, None, o[1], None), -2, sw + b": n_tan must be 1..8 (directions per call)"),   # n_tan in front of the tangents
        ("nmpc", s, (z, 10, z, z, z, 9, None, None, None, o[1], None), -2, sw + b": n_tan must be 1..8 (directions per call)"),
        ("nmpc", s, (z, 6, z, z, z, 1, None, None, None, o[1], None), -2, sw + b": no tangent given (d_tz and d_tw both NULL)"),   # tangents in front of d_df
        ("nmpc", s, (z, 6, None, z, None, 8, z, z, None, o[1], None), -2, sw + b": d_df is required (the tangent of the force)"),
        ("bare", m, (None, 7, None, 0, z, z, 0, None, None, None, o[1], None), -1, None),
        ("bare", m, (z, 7, None, 0, None, z, 0, None, None, None, o[1], None), -1, None),
        ("bare", m, (z, 7, None, 0, z, z, 0, None, None, None, o[1], None), -6, mw + b": ndp_set_mlp_weights was never called"),
        ("nmpc", m, (z, 7, None, 0, z, z, 0, None, None, None, o[1], None), -2, mw + b": K must be 1..8 (NDP_MAX_NEIGH neighbours per vehicle)"),
        ("nmpc", m, (z, 7, None, 9, z, z, 0, None, None, None, o[1], None), -2, mw + b": K must be 1..8 (NDP_MAX_NEIGH neighbours per vehicle)"),
        ("nmpc", m, (z, 7, None, K, z, z, 0, None, None, None, o[1], None), -2, mw + b": d_other_index is required (int32 [B][K])"),
        ("nmpc", m, (z, 7, z, K, z, z, 0, None, None, None, o[1], None), -2, mw + b": other_stride must be 6 or 10"),
        ("nmpc", m, (z, 10, z, K, z, z, 0, None, None, None, o[1], None), -2, mw + b": n_tan must be 1..8 (directions per call)"),
        ("nmpc", m, (z, 10, z, K, z, z, 9, None, None, None, o[1], None), -2, mw + b": n_tan must be 1..8 (directions per call)"),
        ("nmpc", m, (z, 6, z, K, z, z, 1, None, None, None, o[1], None), -2, mw + b": no tangent given (d_tz and d_tw both NULL)"),
        ("nmpc", m, (z, 6, z, K, z, None, 8, z, z, None, o[1], None), -2, mw + b": d_df is required (the tangent of the summed force)"),
    ])


def test_downwash_and_plant_force_forward_forms(world):
    z, o = world["zin"].data_ptr(), [world["out"][j].data_ptr() for j in range(8)]
    hi, ho = world["hin"].ctypes.data, world["hout"].ctypes.data
    _refused(world, [
        # ndp_plant_force_device (x, index, gate, scale, f, xy, stream): NULL, then the weights (only with an index)
        ("bare", "ndp_plant_force_device", (None, z, 1, 1.0, o[0], o[1], None), -1, None),
        ("bare", "ndp_plant_force_device", (z, z, 1, 1.0, None, o[1], None), -1, None),
        ("bare", "ndp_plant_force_device", (z, z, 1, 1.0, o[0], o[1], None), -6, NO_MLP),
        # ndp_plant_force (x, index, gate, scale, f)
        ("bare", "ndp_plant_force", (None, hi, 1, 1.0, ho), -1, None),
        ("bare", "ndp_plant_force", (hi, hi, 1, 1.0, None), -1, None),
        ("bare", "ndp_plant_force", (hi, hi, 1, 1.0, ho), -6, NO_MLP),
        # ndp_plant_force_multi_device (x, index, K, gate, scale, f, xy, stream): K in front of NULL, NULL in front of the weights
        ("bare", "ndp_plant_force_multi_device", (None, z, 0, 1, 1.0, None, o[1], None), -2, _k_text(b"ndp_plant_force_multi_device", 0)),
        ("bare", "ndp_plant_force_multi_device", (None, z, 9, 1, 1.0, None, o[1], None), -2, _k_text(b"ndp_plant_force_multi_device", 9)),
        ("bare", "ndp_plant_force_multi_device", (None, z, K, 1, 1.0, o[0], o[1], None), -1, None),
        ("bare", "ndp_plant_force_multi_device", (z, z, K, 1, 1.0, None, o[1], None), -1, None),
        ("bare", "ndp_plant_force_multi_device", (z, z, K, 1, 1.0, o[0], o[1], None), -6, NO_MLP),
        # ndp_plant_force_multi (x, index, K, gate, scale, f)
        ("bare", "ndp_plant_force_multi", (None, hi, 0, 1, 1.0, None), -2, _k_text(b"ndp_plant_force_multi", 0)),
        ("bare", "ndp_plant_force_multi", (None, hi, 9, 1, 1.0, None), -2, _k_text(b"ndp_plant_force_multi", 9)),
        ("bare", "ndp_plant_force_multi", (None, hi, K, 1, 1.0, ho), -1, None),
        ("bare", "ndp_plant_force_multi", (hi, hi, K, 1, 1.0, None), -1, None),
        ("bare", "ndp_plant_force_multi", (hi, hi, K, 1, 1.0, ho), -6, NO_MLP),
        # ndp_downwash_multi_device (other, stride, index, K, ego, ego_xy, f_out, stream): K, NULL, the stride (-13), the weights
        ("bare", "ndp_downwash_multi_device", (None, 7, None, 0, None, z, None, None), -2, _k_text(b"ndp_downwash_multi_device", 0)),
        ("bare", "ndp_downwash_multi_device", (None, 7, None, 9, None, z, None, None), -2, _k_text(b"ndp_downwash_multi_device", 9)),
        ("bare", "ndp_downwash_multi_device", (None, 7, z, K, z, z, o[0], None), -1, None),
        ("bare", "ndp_downwash_multi_device", (z, 7, None, K, z, z, o[0], None), -1, None),
        ("bare", "ndp_downwash_multi_device", (z, 7, z, K, None, z, o[0], None), -1, None),
        ("bare", "ndp_downwash_multi_device", (z, 7, z, K, z, z, None, None), -1, None),
        ("bare", "ndp_downwash_multi_device", (z, 7, z, K, z, z, o[0], None), -13, b"ndp_downwash_multi_device: other_stride must be 10 or 6"),
        ("bare", "ndp_downwash_multi_device", (z, 6, z, K, z, z, o[0], None), -6, NO_MLP),
        # ndp_downwash_multi (other, index, K, ego, ego_xy, f_out)
        ("bare", "ndp_downwash_multi", (None, None, 0, None, hi, None), -2, _k_text(b"ndp_downwash_multi", 0)),
        ("bare", "ndp_downwash_multi", (None, None, 9, None, hi, None), -2, _k_text(b"ndp_downwash_multi", 9)),
        ("bare", "ndp_downwash_multi", (None, hi, K, hi, hi, ho), -1, None),
        ("bare", "ndp_downwash_multi", (hi, None, K, hi, hi, ho), -1, None),
        ("bare", "ndp_downwash_multi", (hi, hi, K, None, hi, ho), -1, None),
        ("bare", "ndp_downwash_multi", (hi, hi, K, hi, hi, None), -1, None),
        ("bare", "ndp_downwash_multi", (hi, hi, K, hi, hi, ho), -6, NO_MLP),
        # ndp_downwash (other, ego, ego_xy, f_out)
        ("bare", "ndp_downwash", (None, hi, hi, ho), -1, None),
        ("bare", "ndp_downwash", (hi, None, hi, ho), -1, None),
        ("bare", "ndp_downwash", (hi, hi, hi, None), -1, None),
        ("bare", "ndp_downwash", (hi, hi, hi, ho), -6, NO_MLP),
    ])


def test_plant_step_and_rollouts(world):
    z, o = world["zin"].data_ptr(), [world["out"][j].data_ptr() for j in range(8)]
    hi, ho = world["hin"].ctypes.data, world["hout"].ctypes.data
    r, f, m = "ndp_rollout_device", "ndp_rollout_formation_device", "ndp_rollout_formation_multi_device"
    rw, fw, mw = r.encode(), f.encode(), m.encode()
    no_fd = b": NDP_FORM_COMPENSATE needs use_fd = 1 (NDP model)"
    no_w = b": ndp_set_mlp_weights was never called (the force on the plant is the network's)"
    no_traj = b": ndp_ref_set_trajectory was never called"
    both = GATE | COMPENSATE
    _refused(world, [
        # ndp_plant_step_device (x, u, f, dt, substeps, stream), ndp_plant_step (x, u, f, dt, substeps): -1 for NULL and for substeps < 1
        ("nmpc", "ndp_plant_step_device", (None, z, None, 0.01, 1, None), -1, None),
        ("nmpc", "ndp_plant_step_device", (o[0], None, None, 0.01, 1, None), -1, None),
        ("nmpc", "ndp_plant_step_device", (o[0], z, None, 0.01, 0, None), -1, None),
        ("nmpc", "ndp_plant_step", (None, hi, None, 0.01, 1), -1, None),
        ("nmpc", "ndp_plant_step", (ho, None, None, 0.01, 1), -1, None),
        ("nmpc", "ndp_plant_step", (ho, hi, None, 0.01, 0), -1, None),
        # ndp_rollout_device (ticks, t0, dt_tick, substeps, x, log, stream): sensitivities, then -1 (NULL, ticks, substeps), the model, the trajectory
        ("sens", r, (0, 0.0, 0.01, 0, None, o[1], None), -2, rw + SENS),
        ("bare", r, (0, 0.0, 0.01, 1, o[0], o[1], None), -1, None),
        ("bare", r, (1, 0.0, 0.01, 0, o[0], o[1], None), -1, None),
        ("bare", r, (1, 0.0, 0.01, 1, None, o[1], None), -1, None),
        ("bare", r, (1, 0.0, 0.01, 1, o[0], o[1], None), -8, rw + b": the rollout drives the NMPC model (use_fd = 0)"),      # the model in front of the trajectory
        ("nmpc", r, (1, 0.0, 0.01, 1, o[0], o[1], None), -11, b"ndp_ref_window" + no_traj),
        # ndp_rollout_formation_device (ticks, t0, dt_tick, substeps, index, flags, scale, x, log, log_u, log_f, worst, stream)
        ("sens", f, (0, 0.0, 0.01, 0, z, 4, 1.0, None, o[1], o[2], o[3], o[4], None), -2, fw + SENS),
        ("nmpc", f, (0, 0.0, 0.01, 1, z, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -1, None),                  # -1 in front of the -8s
        ("nmpc", f, (1, 0.0, 0.01, 0, z, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -1, None),
        ("nmpc", f, (1, 0.0, 0.01, 1, z, both, 1.0, None, o[1], o[2], o[3], o[4], None), -1, None),
        ("nmpc", f, (1, 0.0, 0.01, 1, z, both | 4, 1.0, o[0], o[1], o[2], o[3], o[4], None), -1, None),
        ("nmpc", f, (1, 0.0, 0.01, 1, z, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -8, fw + no_fd),            # the model in front of the trajectory
        ("bare", f, (1, 0.0, 0.01, 1, z, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -8, fw + no_w),             # the weights in front of the trajectory
        ("bare", f, (1, 0.0, 0.01, 1, None, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -8, fw + no_traj),       # no index: no weights needed
        ("nmpc", f, (1, 0.0, 0.01, 1, z, GATE, 1.0, o[0], o[1], o[2], o[3], o[4], None), -8, fw + no_traj),
        # ndp_rollout_formation_multi_device: K behind the index; sensitivities, -1, K, then the single form's -8s
        ("sens", m, (0, 0.0, 0.01, 0, z, 0, 4, 1.0, None, o[1], o[2], o[3], o[4], None), -2, mw + SENS),
        ("nmpc", m, (0, 0.0, 0.01, 1, z, 0, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -1, None),               # -1 in front of K
        ("nmpc", m, (1, 0.0, 0.01, 0, z, 0, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -1, None),
        ("nmpc", m, (1, 0.0, 0.01, 1, z, 0, both, 1.0, None, o[1], o[2], o[3], o[4], None), -1, None),
        ("nmpc", m, (1, 0.0, 0.01, 1, z, 0, both | 4, 1.0, o[0], o[1], o[2], o[3], o[4], None), -1, None),
        ("nmpc", m, (1, 0.0, 0.01, 1, None, 0, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -2, _k_text(mw, 0)),  # K in front of the model
        ("nmpc", m, (1, 0.0, 0.01, 1, z, 9, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -2, _k_text(mw, 9)),
        ("nmpc", m, (1, 0.0, 0.01, 1, z, K, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -8, mw + no_fd),
        ("bare", m, (1, 0.0, 0.01, 1, z, K, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -8, mw + no_w),
        ("bare", m, (1, 0.0, 0.01, 1, None, K, both, 1.0, o[0], o[1], o[2], o[3], o[4], None), -8, mw + no_traj),
        ("nmpc", m, (1, 0.0, 0.01, 1, z, K, GATE, 1.0, o[0], o[1], o[2], o[3], o[4], None), -8, mw + no_traj),
    ])


def _ticks_text(who, n):
    return who + b": ticks must be >= 1, got " + str(n).encode()


def _sub_text(who, n):
    return who + b": substeps must be 1..16 (NDP_PLANT_MAX_SUBSTEPS), got " + str(n).encode()


def test_plant_rollout_and_its_derivatives(world):
    z, o = world["zin"].data_ptr(), [world["out"][j].data_ptr() for j in range(8)]
    r, v, j = "ndp_plant_rollout_device", "ndp_plant_rollout_vjp_device", "ndp_plant_rollout_jvp_device"
    rw, vw, jw = r.encode(), v.encode(), j.encode()
    _refused(world, [
        # (ticks, dt, substeps, x0, u, f, xs, stream)
        ("nmpc", r, (0, 0.01, 0, None, z, z, o[0], None), -1, None),                       # NULL in front of ticks
        ("nmpc", r, (0, 0.01, 0, z, None, z, o[0], None), -1, None),
        ("nmpc", r, (0, 0.01, 0, z, z, z, None, None), -1, None),
        ("nmpc", r, (0, 0.01, 0, z, z, z, o[0], None), -2, _ticks_text(rw, 0)),            # ticks in front of substeps
        ("nmpc", r, (2, 0.01, 0, z, z, z, o[0], None), -2, _sub_text(rw, 0)),
        ("nmpc", r, (2, 0.01, 17, z, z, z, o[0], None), -2, _sub_text(rw, 17)),
        # (ticks, dt, substeps, x0, u, f, xs, gxs, gx0, gu, gf, stream)
        ("nmpc", v, (0, 0.01, 0, None, z, z, z, z, None, None, None, None), -1, None),
        ("nmpc", v, (0, 0.01, 0, z, None, z, z, z, None, None, None, None), -1, None),
        ("nmpc", v, (0, 0.01, 0, z, z, z, None, z, None, None, None, None), -1, None),
        ("nmpc", v, (0, 0.01, 0, z, z, z, z, None, None, None, None, None), -1, None),     # the upstream gradient is a required pointer here
        ("nmpc", v, (0, 0.01, 0, z, z, z, z, z, None, None, None, None), -2, _ticks_text(vw, 0)),
        ("nmpc", v, (2, 0.01, 0, z, z, z, z, z, None, None, None, None), -2, _sub_text(vw, 0)),      # substeps in front of the outputs
        ("nmpc", v, (2, 0.01, 17, z, z, z, z, z, None, None, None, None), -2, _sub_text(vw, 17)),
        ("nmpc", v, (2, 0.01, 16, z, z, z, z, z, None, None, None, None), -2, vw + b": no output asked for (d_gx0, d_gu and d_gf all NULL)"),
        # (ticks, dt, substeps, x0, u, f, n_tan, tx0, tu, tf, dxs, xs_check, stream)
        ("nmpc", j, (0, 0.01, 0, None, z, z, 0, None, None, None, None, o[1], None), -1, None),
        ("nmpc", j, (0, 0.01, 0, z, None, z, 0, None, None, None, None, o[1], None), -1, None),
        ("nmpc", j, (0, 0.01, 0, z, z, z, 0, None, None, None, None, o[1], None), -2, _ticks_text(jw, 0)),
        ("nmpc", j, (2, 0.01, 0, z, z, z, 0, None, None, None, None, o[1], None), -2, _sub_text(jw, 0)),      # substeps in front of n_tan
        ("nmpc", j, (2, 0.01, 17, z, z, z, 0, None, None, None, None, o[1], None), -2, _sub_text(jw, 17)),
        ("nmpc", j, (2, 0.01, 1, z, z, z, 0, None, None, None, None, o[1], None), -2, jw + b": n_tan must be 1..8 (directions per call)"),   # n_tan in front of the tangents
        ("nmpc", j, (2, 0.01, 1, z, z, z, 9, None, None, None, None, o[1], None), -2, jw + b": n_tan must be 1..8 (directions per call)"),
        ("nmpc", j, (2, 0.01, 1, z, z, z, 8, None, None, None, None, o[1], None), -2, jw + b": no tangent given (d_tx0, d_tu and d_tf all NULL)"),   # in front of d_dxs
        ("nmpc", j, (2, 0.01, 1, z, z, z, 1, z, z, z, None, o[1], None), -2, jw + b": d_dxs is required (the tangent of the log)"),
    ])


def test_closed_loop_and_its_derivatives(world):
    z, o = world["zin"].data_ptr(), [world["out"][j].data_ptr() for j in range(8)]
    c, v, j = "ndp_closed_loop_device", "ndp_closed_loop_vjp_device", "ndp_closed_loop_jvp_device"
    cw, vw, jw = c.encode(), v.encode(), j.encode()
    force = b": a disturbance force (d_f) needs use_fd = 1 (NDP model)"
    tape = b": d_tape is required (the forward's, recorded by ndp_closed_loop_device)"

    # (ticks, dt, substeps, x0, xr, ur, f, fp, xs, us, Xs, status, tape, stream)
    def fwd(ticks=2, sub=1, x0=z, xr=z, ur=z, f=None, xs=o[0], us=o[1]):
        return (ticks, 0.01, sub, x0, xr, ur, f, z, xs, us, o[2], o[3], o[4], None)

    # (ticks, dt, substeps, x0, xr, ur, f, fp, xs, us, tape, gxs, gus, gXs, gx0, gxr, gur, gf, gfp, gmodel, status_check, stream)
    def vjp(ticks=2, sub=1, x0=z, xr=z, ur=z, f=None, xs=z, us=z, tp=z, up=z, outs=True):
        g = [o[0], o[1], o[2], o[3], o[4], o[5]] if outs else [None] * 6
        return (ticks, 0.01, sub, x0, xr, ur, f, z, xs, us, tp, up, None, None, *g, o[6], None)

    # (ticks, dt, substeps, x0, xr, ur, f, fp, xs, us, tape, n_tan, tx0, txr, tur, tf, tfp, dxs, dus, dXs, dUs, status_check, stream)
    def jvp(ticks=2, sub=1, x0=z, xr=z, ur=z, f=None, xs=z, us=z, tp=z, T=1, tx0=z, tf=None, dxs=o[0], dus=o[1]):
        return (ticks, 0.01, sub, x0, xr, ur, f, z, xs, us, tp, T, tx0, None, None, tf, None, dxs, dus, o[2], o[3], o[6], None)

    cases = []
    for fn, who, mk in ((c, cw, fwd), (v, vw, vjp), (j, jw, jvp)):
        cases += [
            ("sens", fn, mk(x0=None, ticks=0), -1, None),                                   # NULL in front of the sensitivities
            ("nmpc", fn, mk(xr=None, ticks=0), -1, None),
            ("nmpc", fn, mk(ur=None, ticks=0), -1, None),
            ("nmpc", fn, mk(xs=None, ticks=0), -1, None),
            ("nmpc", fn, mk(us=None, ticks=0), -1, None),
            ("sens", fn, mk(ticks=0, sub=0, f=z), -2, who + SENS),                          # the sensitivities in front of ticks
            ("nmpc", fn, mk(ticks=0, sub=0, f=z), -2, _ticks_text(who, 0)),                 # ticks in front of substeps
            ("nmpc", fn, mk(sub=0, f=z), -2, _sub_text(who, 0)),                            # substeps in front of the force
            ("nmpc", fn, mk(sub=17, f=z), -2, _sub_text(who, 17)),
            ("bare", fn, mk(sub=17, f=z), -2, _sub_text(who, 17)),
        ]
    cases += [
        ("nmpc", v, vjp(f=z, tp=None, up=None, outs=False), -2, vw + force),               # the force in front of the tape
        ("nmpc", v, vjp(tp=None, up=None, outs=False), -2, vw + tape),                      # the tape in front of the upstream gradient
        ("bare", v, vjp(f=z, tp=None, up=None, outs=False), -2, vw + tape),
        ("nmpc", v, vjp(up=None, outs=False), -2, vw + b": no upstream gradient (d_gxs, d_gus and d_gXs all NULL)"),   # in front of the outputs
        ("nmpc", v, vjp(outs=False), -2, vw + b": no output asked for (d_gx0, d_gxr, d_gur, d_gf, d_gfp and d_gmodel all NULL)"),
        ("nmpc", j, jvp(f=z, tp=None, T=0), -2, jw + force),
        ("nmpc", j, jvp(tp=None, T=0), -2, jw + tape),                                      # the tape in front of n_tan
        ("nmpc", j, jvp(T=0, tx0=None), -2, jw + b": n_tan must be 1..8 (directions per call)"),   # n_tan in front of the tangents
        ("nmpc", j, jvp(T=9, tx0=None), -2, jw + b": n_tan must be 1..8 (directions per call)"),
        ("nmpc", j, jvp(tx0=None, tf=None, dxs=None), -2, jw + b": no tangent given (d_tx0, d_txr, d_tur, d_tf and d_tfp all NULL)"),
        ("nmpc", j, jvp(tf=z, dxs=None), -2, jw + b": a force tangent (d_tf) needs use_fd = 1 (NDP model)"),   # in front of the outputs
        ("nmpc", j, jvp(dxs=None), -2, jw + b": d_dxs and d_dus are required (the tangents of the two logs)"),
        ("bare", j, jvp(tf=z, dus=None), -2, jw + b": d_dxs and d_dus are required (the tangents of the two logs)"),
    ]
    _refused(world, cases)


def test_the_handles_still_work(world):
    """Behind all of the above: a refusal leaves the handle usable (ndp_synchronize on each, and the tape size of the closed loop)."""
    for name in ("bare", "nmpc", "sens"):
        e = world[name]
        n = C.c_size_t(0)
        assert e._lib.ndp_closed_loop_tape_bytes(e._h, 2, C.byref(n)) == 0 and n.value > 0
        e.synchronize()
