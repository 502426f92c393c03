"""BatchedNMPC: B independent quadrotor OCPs solved per call on one MI355X through the C-ABI.

This is the batched form of the reference's controller objects
(nmpc_ctl/nmpc_body_rate_ctl.py:20-112, ndp_nmpc_ctl/ndp_nmpc_body_rate_ctl.py:20-112):
`reset(xr, ur)` seeds the persistent SQP iterate, `update(...)` runs one SQP-RTI iteration per
instance (plus the downwash MLP when neighbour windows are given) and returns u0[B,4].
Host arrays go through ndp_step; torch CUDA tensors go through ndp_step_device (no host copies).
"""
import ctypes as C

import numpy as np

from . import _lib
from .params import downwash_params as DP
from .params import nmpc_params as CP


class NdpError(RuntimeError):
    pass


def _raise_status(rc):
    # same text as nmpc_body_rate_ctl.py:109-110
    raise Exception("acados acados_ocp_solver returned status {}. Exiting.".format(rc))


def _t_axis_shapes(who, B, rows, n_tan=None):
    """The T axis of a forward-mode call, from shapes alone.  rows: one (shape, tail, lead) per tangent / output -- the tensor's shape
    (None: not given), its shape behind the T axis (a tuple), and the number of batch dimensions in front of the axis (1: [B,T,...];
    0: [T,...], the weights' direction).  Returns (T, demanded): T is n_tan when given, else read from the shapes (a shape without the
    axis means T = 1; nothing given: 1); demanded[i] is the shape tensor i must have (what _dptr then holds it to) -- with the axis where
    it came with it, else without (T = 1 as it lies) -- and None for a tensor not given."""
    if n_tan is None:
        Ts = {int(s[lead]) if len(s) == lead + 1 + len(tail) else 1 for s, tail, lead in rows if s is not None}
        if len(Ts) > 1:
            raise ValueError(f"{who}: tangents and outputs disagree on the number of directions ({sorted(Ts)})")
        n_tan = Ts.pop() if Ts else 1
    T, heads, demanded = int(n_tan), ((), (B,)), []
    for s, tail, lead in rows:
        if s is not None:
            if len(s) == lead + 1 + len(tail):
                s = heads[lead] + (T,) + tail
            elif T != 1:
                raise ValueError(f"{who}: a tensor without the T axis with n_tan = {T}")
            else:
                s = heads[lead] + tail
        demanded.append(s)
    return T, demanded


class BatchedNMPC:
    def __init__(self, batch, N=CP.N_node, disturbance=False, n_rti=1, qp_mode=_lib.QP_AUTO, device=0,
                 dt=CP.th_pred, load_mlp=None, **cfg_overrides):
        self._lib = _lib.load()
        # ndp_create refuses ipm_refine > 0 (the library default: 2) for shapes whose kernels carry no refinement path (N >= 28, the
        # precision studies): such engines are created with ipm_refine = 0 unless the caller says otherwise (and is then told no)
        if "ipm_refine" not in cfg_overrides and (7 * int(N) - 3 > 192 or cfg_overrides.get("qp_precision", 0)):
            cfg_overrides = dict(cfg_overrides, ipm_refine=0)
        # (r_horiz: the reference's gate radius unless the caller overrides it like any other ndp_cfg field)
        self.cfg = _lib.default_cfg(batch=int(batch), N=int(N), n_rti=int(n_rti), use_fd=int(bool(disturbance)),
                                    qp_mode=int(qp_mode), device=int(device), dt=float(dt),
                                    **{"r_horiz": DP.r_horiz, **cfg_overrides})
        self.B, self.N = int(batch), int(N)
        self.disturbance = bool(disturbance)
        self._h = C.c_void_p()
        rc = self._lib.ndp_create(C.byref(self.cfg), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise NdpError(f"ndp_create failed ({rc}): {self._lib.ndp_last_error(None).decode()}")
        self._form_K = self._form_index = None      # closed_loop_formation_config: what is configured (K, a host copy of the index)
        if load_mlp is None:
            load_mlp = self.disturbance
        if load_mlp:
            self.set_mlp_weights(_lib.load_weights())

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "_h", None):
            self._lib.ndp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise NdpError(f"{what} failed ({rc}): {self._lib.ndp_last_error(self._h).decode()}")
        return rc

    def set_mlp_weights(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self._check(self._lib.ndp_set_mlp_weights(self._h, _lib.ptr(blob), blob.size), "ndp_set_mlp_weights")
        self._mlp_installed = None          # (torch_layer: whatever tensor was installed through set_mlp_weights_device no longer is)

    # ------------------------------------------------------------------ reference-shaped API (host arrays)
    def reset(self, xr, ur):
        """nmpc_body_rate_ctl.py:86-91 for every instance."""
        xr = _lib.f64(xr, (self.B, self.N + 1, 10))
        ur = _lib.f64(ur, (self.B, self.N, 4))
        self._check(self._lib.ndp_reset(self._h, _lib.ptr(xr), _lib.ptr(ur)), "ndp_reset")

    def update(self, x0, xr, ur, f=None, other=None, ego_xy=None, raise_on_status=True, full=False):
        """update(x0, xr, ur[, f]) for every instance; returns u0[B,4] float64.

        f: [B,N+1,3] disturbance force (NDP).  other/ego_xy: neighbour reference windows and ego
        odometry xy; the force is then predicted on the device (DownwashNN.update + r_horiz gate).
        full=True: returns (u0, X, U, status, ipm_iters) from the same call (ndp_step_ex: one synchronisation) -- what
        the reference's callers read after solve_for_x0 (solver.get / solver.status).
        """
        x0 = _lib.f64(x0, (self.B, 10))
        xr = _lib.f64(xr, (self.B, self.N + 1, 10))
        ur = _lib.f64(ur, (self.B, self.N, 4))
        u0 = np.empty((self.B, 4), dtype=np.float64)
        X = U = st = it = None
        if full:
            X, U, st, it = self._full_out()
        if f is not None and other is None and np.asarray(f).dtype == np.float64:
            # a float64 force goes to the device as it is (ndp_step_ex_f64): the reference hands acados a float64 p
            # (ndp_nmpc_body_rate_ctl.py:97-99); DownwashNN's float32 output takes the fp32 entries below -- the same numbers
            f64 = _lib.f64(f, (self.B, self.N + 1, 3))
            rc = self._check(self._lib.ndp_step_ex_f64(self._h, _lib.ptr(x0), _lib.ptr(xr), _lib.ptr(ur), _lib.ptr(f64), _lib.ptr(u0),
                                                       _lib.ptr(X), _lib.ptr(U), _lib.ptr(st), _lib.ptr(it)), "ndp_step_ex_f64")
        else:
            f32 = None if f is None else np.ascontiguousarray(f, dtype=np.float32).reshape(self.B, self.N + 1, 3)
            other = _lib.f64(other, (self.B, self.N + 1, 10))
            ego_xy = _lib.f64(ego_xy, (self.B, 2))
            if full:
                rc = self._check(self._lib.ndp_step_ex(self._h, _lib.ptr(x0), _lib.ptr(xr), _lib.ptr(ur), _lib.ptr(f32),
                                                       _lib.ptr(other), _lib.ptr(ego_xy), _lib.ptr(u0), _lib.ptr(X), _lib.ptr(U),
                                                       _lib.ptr(st), _lib.ptr(it)), "ndp_step_ex")
            else:
                rc = self._check(self._lib.ndp_step(self._h, _lib.ptr(x0), _lib.ptr(xr), _lib.ptr(ur), _lib.ptr(f32),
                                                    _lib.ptr(other), _lib.ptr(ego_xy), _lib.ptr(u0)), "ndp_step")
        if rc != 0 and raise_on_status:
            _raise_status(rc)
        return (u0, X, U, st, it) if full else u0

    def _full_out(self, tick=False):
        """The outputs only full=True returns: (X, U, status, ipm_iters) of the step forms, (u0, status, ipm_iters) of the tick forms."""
        st, it = np.empty(self.B, dtype=np.int32), np.empty(self.B, dtype=np.int32)
        if tick:
            return np.empty((self.B, 4)), st, it
        return np.empty((self.B, self.N + 1, 10)), np.empty((self.B, self.N, 4)), st, it

    def update_begin(self, x0, xr, ur, f=None, other=None, ego_xy=None, want_iterate=False):
        """First half of update(): packs the host arrays into a page-locked mirror, enqueues ONE launch that reads the mirror over
        PCIe and writes its results into a page-locked block itself (zero-copy: no H2D / D2H copy operation) and returns without
        waiting (ndp_step_begin).  Up to two steps may be in flight: begin tick i+1 before update_end() of tick i and the packing
        of tick i+1 overlaps tick i's kernel.  The arrays may be reused as soon as this returns.  Drain every begun step with
        update_end() before reset() / set_iterate() / close()."""
        x0 = _lib.f64(x0, (self.B, 10))
        xr = _lib.f64(xr, (self.B, self.N + 1, 10))
        ur = _lib.f64(ur, (self.B, self.N, 4))
        f32 = None if f is None else np.ascontiguousarray(f, dtype=np.float32).reshape(self.B, self.N + 1, 3)
        other = _lib.f64(other, (self.B, self.N + 1, 10))
        ego_xy = _lib.f64(ego_xy, (self.B, 2))
        self._check(self._lib.ndp_step_begin(self._h, _lib.ptr(x0), _lib.ptr(xr), _lib.ptr(ur), _lib.ptr(f32), _lib.ptr(other),
                                             _lib.ptr(ego_xy), 1 if want_iterate else 0), "ndp_step_begin")

    def update_end(self, raise_on_status=True, full=False, out=None):
        """Second half: waits for the oldest begun step; returns u0[B,4] (full=True: (u0, X, U, status, ipm_iters); X, U only if
        that step was begun with want_iterate).  `out`: a [B,4] float64 array to write u0 into."""
        u0 = np.empty((self.B, 4), dtype=np.float64) if out is None else out
        X = U = st = it = None
        if full:
            X, U, st, it = self._full_out()
        rc = self._check(self._lib.ndp_step_end(self._h, _lib.ptr(u0), _lib.ptr(X), _lib.ptr(U), _lib.ptr(st), _lib.ptr(it)),
                         "ndp_step_end")
        if rc != 0 and raise_on_status:
            _raise_status(rc)
        return (u0, X, U, st, it) if full else u0

    def update_debug(self, x0, xr, ur, f=None, other=None, ego_xy=None):
        """B = 1 only: one step that also returns the kernel's LDS image after linearisation (tests)."""
        x0, xr, ur = _lib.f64(x0, (1, 10)), _lib.f64(xr, (1, self.N + 1, 10)), _lib.f64(ur, (1, self.N, 4))
        f32 = None if f is None else np.ascontiguousarray(f, dtype=np.float32).reshape(1, self.N + 1, 3)
        other, ego_xy = _lib.f64(other, (1, self.N + 1, 10)), _lib.f64(ego_xy, (1, 2))
        u0 = np.empty((1, 4))
        dump = np.zeros(self._lib.ndp_debug_lds_doubles(self.N))
        self._check(self._lib.ndp_step_debug(self._h, _lib.ptr(x0), _lib.ptr(xr), _lib.ptr(ur), _lib.ptr(f32),
                                             _lib.ptr(other), _lib.ptr(ego_xy), _lib.ptr(u0), _lib.ptr(dump)),
                    "ndp_step_debug")
        return u0, dump

    def downwash(self, other, ego_ref, ego_xy=None):
        """DownwashNN.update for every instance (+ optional gate); returns f[B,N+1,3] float32."""
        other = _lib.f64(other, (self.B, self.N + 1, 10))
        ego_ref = _lib.f64(ego_ref, (self.B, self.N + 1, 10))
        ego_xy = _lib.f64(ego_xy, (self.B, 2))
        f = np.empty((self.B, self.N + 1, 3), dtype=np.float32)
        self._check(self._lib.ndp_downwash(self._h, _lib.ptr(other), _lib.ptr(ego_ref), _lib.ptr(ego_xy), _lib.ptr(f)),
                    "ndp_downwash")
        return f

    # ------------------------------------------------------------------ f3: hover-throttle estimator + actuator command
    def throttle_reset(self):
        self._check(self._lib.ndp_throttle_reset(self._h), "ndp_throttle_reset")

    def throttle_update(self, vz, throttle):
        """HoverThrottleEstimator.update for every instance: returns k_throttle[B]."""
        vz, throttle = _lib.f64(vz, (self.B,)), _lib.f64(throttle, (self.B,))
        k = np.empty(self.B)
        self._check(self._lib.ndp_throttle_update(self._h, _lib.ptr(vz), _lib.ptr(throttle), _lib.ptr(k)), "ndp_throttle_update")
        return k

    def throttle_state(self):
        st = np.empty((self.B, 8))
        self._check(self._lib.ndp_throttle_get_state(self._h, _lib.ptr(st)), "ndp_throttle_get_state")
        return st

    def actuator_cmd(self, u0, k_throttle):
        """nmpc_u_2_att_tgt for every instance: [wx, wy, wz, c] -> [wx, wy, wz, thrust]."""
        u0, k = _lib.f64(u0, (self.B, 4)), _lib.f64(k_throttle, (self.B,))
        cmd = np.empty((self.B, 4))
        self._check(self._lib.ndp_actuator_cmd(self._h, _lib.ptr(u0), _lib.ptr(k), _lib.ptr(cmd)), "ndp_actuator_cmd")
        return cmd

    # ------------------------------------------------------------------ f2: follower reference relay
    def relay_reset(self):
        self._check(self._lib.ndp_relay_reset(self._h), "ndp_relay_reset")

    def relay_formation(self, form):
        """One formation_ref message per instance (nmpc_follower_node.py:44-56): returns the filtered offsets [B,3]."""
        form = _lib.f64(form, (self.B, 3))
        off = np.empty((self.B, 3))
        self._check(self._lib.ndp_relay_formation(self._h, _lib.ptr(form), _lib.ptr(off)), "ndp_relay_formation")
        return off

    def relay_reference(self, xr_lead):
        """Leader windows -> follower references (nmpc_follower_node.py:58-74); ur is the leader's, unchanged."""
        xr_lead = _lib.f64(xr_lead, (self.B, self.N + 1, 10))
        out = np.empty_like(xr_lead)
        self._check(self._lib.ndp_relay_reference(self._h, _lib.ptr(xr_lead), _lib.ptr(out)), "ndp_relay_reference")
        return out

    # ------------------------------------------------------------------ f1: reference window generation
    def ref_set_trajectory(self, coeff_x, coeff_y, coeff_z, coeff_yaw, time_cum, time_seg, final_pt):
        """TrajCoefficients of every instance (NMPCRefPublisher.reset, pt_pub/pt_publisher.py:57-60); all instances
        carry the same number of segments: coeff_x/y/z[B,n_seg*8], coeff_yaw[B,n_seg*4], time_cum[B,n_seg+1], ..."""
        time_seg = _lib.f64(time_seg)
        n_seg = time_seg.shape[1]
        cx, cy, cz = (_lib.f64(np.reshape(c, (self.B, n_seg * 8)), (self.B, n_seg * 8)) for c in (coeff_x, coeff_y, coeff_z))
        cyaw = _lib.f64(np.reshape(coeff_yaw, (self.B, n_seg * 4)), (self.B, n_seg * 4))
        time_cum, final_pt = _lib.f64(time_cum, (self.B, n_seg + 1)), _lib.f64(final_pt, (self.B, 3))
        self._check(self._lib.ndp_ref_set_trajectory(self._h, n_seg, _lib.ptr(cx), _lib.ptr(cy), _lib.ptr(cz), _lib.ptr(cyaw),
                                                     _lib.ptr(time_cum), _lib.ptr(_lib.f64(time_seg, (self.B, n_seg))),
                                                     _lib.ptr(final_pt)), "ndp_ref_set_trajectory")

    def ref_window(self, t):
        """get_nmpc_pts for every instance at trajectory times t[B]: returns xr[B,N+1,10], ur[B,N,4]."""
        t = _lib.f64(t, (self.B,))
        xr, ur = np.empty((self.B, self.N + 1, 10)), np.empty((self.B, self.N, 4))
        self._check(self._lib.ndp_ref_window(self._h, _lib.ptr(t), _lib.ptr(xr), _lib.ptr(ur)), "ndp_ref_window")
        return xr, ur

    # the reference's own sliding list of reference points (NMPCRefPublisher, pt_pub/pt_publisher.py:36-103), on the device
    def ref_list_reset(self):
        """_gen_long_list_w_traj for every vehicle (needs ref_set_trajectory)."""
        self._check(self._lib.ndp_ref_list_reset(self._h), "ndp_ref_list_reset")

    def ref_list_fix_pt(self, x_odom, quirk_b1=True):
        """gen_fix_pt_ref's list: every entry = x_odom[B,10], u = [0, 0, 0, mass*g] (the reference's value)."""
        x_odom = _lib.f64(x_odom, (self.B, 10))
        self._check(self._lib.ndp_ref_list_fix_pt(self._h, _lib.ptr(x_odom), int(bool(quirk_b1))), "ndp_ref_list_fix_pt")

    def ref_list_window(self, t=None):
        """t[B] given: get_nmpc_pts (drop the oldest entry, append the point at t + T_horizon, return the window);
        t None: get_nmpc_ref_from_long_list only."""
        t = _lib.f64(t, (self.B,))
        xr, ur = np.empty((self.B, self.N + 1, 10)), np.empty((self.B, self.N, 4))
        self._check(self._lib.ndp_ref_list_window(self._h, _lib.ptr(t), _lib.ptr(xr), _lib.ptr(ur)), "ndp_ref_list_window")
        return xr, ur

    def ref_list_advance_device(self, t, stream=None):
        import torch
        self._check(self._lib.ndp_ref_list_advance_device(self._h, self._dptr(t, torch.float64, (self.B,)), self._stream(stream)),
                    "ndp_ref_list_advance_device")

    def ref_list_window_device(self, xr_out, ur_out, stream=None):
        import torch
        self._check(self._lib.ndp_ref_list_window_device(
            self._h, self._dptr(xr_out, torch.float64, (self.B, self.N + 1, 10)),
            self._dptr(ur_out, torch.float64, (self.B, self.N, 4)), self._stream(stream)), "ndp_ref_list_window_device")

    def ref_window_device(self, t, xr_out, ur_out, stream=None):
        import torch
        self._check(self._lib.ndp_ref_window_device(
            self._h, self._dptr(t, torch.float64, (self.B,)), self._dptr(xr_out, torch.float64, (self.B, self.N + 1, 10)),
            self._dptr(ur_out, torch.float64, (self.B, self.N, 4)), self._stream(stream)), "ndp_ref_window_device")

    # ------------------------------------------------------------------ the node's control tick (odometry in, command out)
    def tick_config(self, other_index=None, gate=True):
        """Who is whose neighbour (int32[B], < 0 / None: none) and whether the r_horiz gate on the ego odometry applies
        (ndp_nmpc_leader_node.py:40,60-76)."""
        oi = None if other_index is None else np.ascontiguousarray(other_index, dtype=np.int32).reshape(self.B)
        self._check(self._lib.ndp_tick_config(self._h, _lib.ptr(oi), 1 if gate else 0), "ndp_tick_config")

    def tick_reset(self):
        """nmpc_ctl.reset(*ref_pub.get_nmpc_ref_from_long_list()) (nmpc_node.py:92,151-152) on the device."""
        self._check(self._lib.ndp_tick_reset(self._h), "ndp_tick_reset")

    def _tick_in(self, x_odom, t, vz, throttle, estimate, want_u0):
        flags = (_lib.TICK_ESTIMATE if estimate else 0) | (_lib.TICK_WANT_U0 if want_u0 else 0)
        if t is not None and np.ndim(t) == 0:            # one clock for every vehicle: a scalar (NDP_TICK_T_UNIFORM)
            t, flags = np.array([float(t)]), flags | _lib.TICK_T_UNIFORM
        else:
            t = _lib.f64(t, (self.B,))
        return (_lib.f64(x_odom, (self.B, 10)), t, _lib.f64(vz, (self.B,)), _lib.f64(throttle, (self.B,)), flags)

    def _tick_t_device(self, t, flags):
        """(pointer, flags) for the t of the device ticks: a CUDA tensor [B] or None as it is; a scalar is one time for every vehicle,
        read by the call from the host (NDP_TICK_T_UNIFORM; the pointer keeps its one-element array alive)."""
        import torch
        if t is not None and not isinstance(t, torch.Tensor):
            return _lib.ptr(np.array([float(t)])), flags | _lib.TICK_T_UNIFORM
        return self._dptr(t, torch.float64, (self.B,)), flags

    def tick_begin(self, x_odom, t=None, vz=None, throttle=None, estimate=False, want_u0=False):
        """First half of tick(): ndp_tick_begin -- only x_odom[B,10] (+ t, vz, throttle [B]) cross PCIe; returns without waiting.
        Up to two ticks in flight."""
        x, t, vz, th, flags = self._tick_in(x_odom, t, vz, throttle, estimate, want_u0)
        self._check(self._lib.ndp_tick_begin(self._h, _lib.ptr(x), _lib.ptr(t), _lib.ptr(vz), _lib.ptr(th), flags), "ndp_tick_begin")

    def tick_end(self, raise_on_status=True, full=False, out=None):
        """Second half: cmd[B,4] = [wx, wy, wz, thrust] of the oldest tick (full=True: (cmd, u0, status, ipm_iters); u0 only if the
        tick was begun with want_u0)."""
        cmd = np.empty((self.B, 4)) if out is None else out
        u0 = st = it = None
        if full:
            u0, st, it = self._full_out(tick=True)
        rc = self._check(self._lib.ndp_tick_end(self._h, _lib.ptr(cmd), _lib.ptr(u0), _lib.ptr(st), _lib.ptr(it)), "ndp_tick_end")
        if rc != 0 and raise_on_status:
            _raise_status(rc)
        return (cmd, u0, st, it) if full else cmd

    def tick(self, x_odom, t=None, vz=None, throttle=None, estimate=False, raise_on_status=True, full=False):
        """One control period of ControllerNode (nmpc_node.py:211-231,251-253) for every vehicle: reference list advance ->
        estimator -> control step (downwash from the neighbour's window) -> actuator command.  Returns cmd[B,4]
        (full=True: (cmd, u0, status, ipm_iters))."""
        x, t, vz, th, flags = self._tick_in(x_odom, t, vz, throttle, estimate, full)
        cmd = np.empty((self.B, 4))
        u0 = st = it = None
        if full:
            u0, st, it = self._full_out(tick=True)
        rc = self._check(self._lib.ndp_tick(self._h, _lib.ptr(x), _lib.ptr(t), _lib.ptr(vz), _lib.ptr(th), flags, _lib.ptr(cmd),
                                            _lib.ptr(u0), _lib.ptr(st), _lib.ptr(it)), "ndp_tick")
        if rc != 0 and raise_on_status:
            _raise_status(rc)
        return (cmd, u0, st, it) if full else cmd

    def tick_device(self, x_odom, cmd_out, t=None, vz=None, throttle=None, estimate=False, u0_out=None, stream=None):
        """The tick's launches on CUDA tensors and a caller's stream (ndp_tick_device); no synchronisation."""
        import torch
        B = self.B
        tp, flags = self._tick_t_device(t, _lib.TICK_ESTIMATE if estimate else 0)
        self._check(self._lib.ndp_tick_device(
            self._h, self._dptr(x_odom, torch.float64, (B, 10)), tp,
            self._dptr(vz, torch.float64, (B,)), self._dptr(throttle, torch.float64, (B,)), flags,
            self._dptr(cmd_out, torch.float64, (B, 4)), self._dptr(u0_out, torch.float64, (B, 4)), self._stream(stream)),
            "ndp_tick_device")

    # ---- the tick with neighbours on other ranks: advance -> window columns -> (exchange) -> step
    def tick_config_remote(self, windows, other_index, gate=True):
        """Neighbour windows come from `windows` (CUDA tensor [rows, N+1, 6 or 10]: an exchange's gathered / peer-mapped buffer, kept
        alive by the caller); other_index[B] = the row of every vehicle's neighbour (< 0: none).  ndp_tick_config_remote."""
        import torch
        assert isinstance(windows, torch.Tensor) and windows.is_cuda and windows.is_contiguous() and windows.dtype == torch.float64
        assert windows.dim() == 3 and windows.shape[1] == self.N + 1 and windows.shape[2] in (6, 10)
        oi = np.ascontiguousarray(other_index, dtype=np.int32).reshape(self.B)
        self._tick_windows = windows
        self._check(self._lib.ndp_tick_config_remote(self._h, C.c_void_p(windows.data_ptr()), int(windows.shape[2]), C.c_int64(int(windows.shape[0])),
                                                     _lib.ptr(oi), 1 if gate else 0), "ndp_tick_config_remote")

    def tick_advance_device(self, x_odom, t=None, vz=None, throttle=None, estimate=False, stream=None):
        """Stage 1: list advance (t: scalar, CUDA tensor [B] or None) + estimator.  ndp_tick_advance_device."""
        import torch
        tp, flags = self._tick_t_device(t, _lib.TICK_ESTIMATE if estimate else 0)
        self._check(self._lib.ndp_tick_advance_device(self._h, self._dptr(x_odom, torch.float64, (self.B, 10)), tp,
                                                      self._dptr(vz, torch.float64, (self.B,)), self._dptr(throttle, torch.float64, (self.B,)),
                                                      flags, self._stream(stream)), "ndp_tick_advance_device")

    def tick_window_pv_device(self, pv_out, stream=None):
        """Stage 2: this tick's window, position / velocity columns -> pv_out [B, N+1, 6] (the exchange's send buffer)."""
        import torch
        self._check(self._lib.ndp_tick_window_pv_device(self._h, self._dptr(pv_out, torch.float64, (self.B, self.N + 1, 6)), self._stream(stream)),
                    "ndp_tick_window_pv_device")

    def tick_step_device(self, x_odom, cmd_out, u0_out=None, stream=None):
        """Stage 3 (behind the exchange): the control step against the exchanged windows + the actuator command."""
        import torch
        self._check(self._lib.ndp_tick_step_device(self._h, self._dptr(x_odom, torch.float64, (self.B, 10)),
                                                   self._dptr(cmd_out, torch.float64, (self.B, 4)), self._dptr(u0_out, torch.float64, (self.B, 4)),
                                                   self._stream(stream)), "ndp_tick_step_device")

    # ------------------------------------------------------------------ f4: plant step (closed-loop rollouts)
    def plant_step(self, x, u, f=None, dt=CP.ts_nmpc, substeps=4):
        x = _lib.f64(x, (self.B, 10)).copy()
        u = _lib.f64(u, (self.B, 4))
        f = _lib.f64(f, (self.B, 3))
        self._check(self._lib.ndp_plant_step(self._h, _lib.ptr(x), _lib.ptr(u), _lib.ptr(f), float(dt), int(substeps)),
                    "ndp_plant_step")
        return x

    def rollout_device(self, ticks, x, log=None, t0=0.0, dt=CP.ts_nmpc, substeps=4, stream=None):
        """Closed loop on the device: reference window -> control step -> plant step, `ticks` times, enqueued on `stream`.
        x[B,10] (CUDA tensor) is the plant state, updated in place; log[ticks,B,10] (optional) receives every state."""
        import torch
        self._check(self._lib.ndp_rollout_device(
            self._h, int(ticks), float(t0), float(dt), int(substeps), self._dptr(x, torch.float64, (self.B, 10)),
            self._dptr(log, torch.float64, (int(ticks), self.B, 10)), self._stream(stream)), "ndp_rollout_device")

    # ---- f4, the plant over a given input sequence, with reverse and forward mode
    def plant_rollout_device(self, x0, u, xs, f=None, dt=CP.ts_nmpc, substeps=4, stream=None):
        """The plant over an input sequence in one launch, enqueued on `stream` with no synchronisation (ndp_plant_rollout_device;
        include/ndp_nmpc.h): x0[B,10], u[ticks,B,4], f[ticks,B,3] or None (each force held over its tick), all float64 CUDA tensors;
        xs[ticks,B,10] receives the state after every tick, row k bit-equal to k + 1 ndp_plant_step_device calls.  x0 may be a slot of
        xs.  ticks is read from u.  The engine's state is not written."""
        import torch
        B, K = self.B, self._plant_ticks(u, "plant_rollout_device")
        d = self._dptr
        self._check(self._lib.ndp_plant_rollout_device(
            self._h, K, float(dt), int(substeps), d(x0, torch.float64, (B, 10)), d(u, torch.float64, (K, B, 4)),
            d(f, torch.float64, (K, B, 3)), d(xs, torch.float64, (K, B, 10)), self._stream(stream)), "ndp_plant_rollout_device")

    def plant_rollout_vjp_device(self, x0, u, xs, gxs, f=None, gx0=None, gu=None, gf=None, dt=CP.ts_nmpc, substeps=4, stream=None):
        """Enqueues the backward pass of plant_rollout_device on `stream` (ndp_plant_rollout_vjp_device; include/ndp_nmpc.h): x0, u, f as
        the forward took them, xs[ticks,B,10] its log, gxs[ticks,B,10] the gradient of every logged state.  Outputs (None = not computed,
        not all None), overwritten, float64: gx0[B,10], gu[ticks,B,4], gf[ticks,B,3] (also with f None: the derivative at f = 0).  The
        derivative of the arithmetic performed: force held over the tick, quaternion renormalised once per tick.  No workspace; two calls
        are bit-identical."""
        import torch
        B, K = self.B, self._plant_ticks(u, "plant_rollout_vjp_device")
        d = self._dptr
        self._check(self._lib.ndp_plant_rollout_vjp_device(
            self._h, K, float(dt), int(substeps), d(x0, torch.float64, (B, 10)), d(u, torch.float64, (K, B, 4)),
            d(f, torch.float64, (K, B, 3)), d(xs, torch.float64, (K, B, 10)), d(gxs, torch.float64, (K, B, 10)),
            d(gx0, torch.float64, (B, 10)), d(gu, torch.float64, (K, B, 4)), d(gf, torch.float64, (K, B, 3)), self._stream(stream)),
            "ndp_plant_rollout_vjp_device")

    def plant_rollout_jvp_device(self, x0, u, dxs, f=None, tx0=None, tu=None, tf=None, n_tan=None, xs_check=None, dt=CP.ts_nmpc, substeps=4,
                                 stream=None):
        """Enqueues the forward mode of plant_rollout_device on `stream` (ndp_plant_rollout_jvp_device; include/ndp_nmpc.h).  Directions
        (None = 0, not all None), float64: tx0[B,T,10], tu[ticks,B,T,4], tf[ticks,B,T,3].  Outputs: dxs[ticks,B,T,10], required;
        xs_check[ticks,B,10], optional -- the primal, bit-equal to plant_rollout_device's log.  T (1..8) is n_tan when given, else read
        from dxs.  T directions in one call equal T calls bit for bit.  No workspace; the engine's state is not written."""
        import torch
        B, K = self.B, self._plant_ticks(u, "plant_rollout_jvp_device")
        if n_tan is None:
            if not (isinstance(dxs, torch.Tensor) and dxs.dim() == 4):
                raise ValueError("plant_rollout_jvp_device: dxs must be a [ticks,B,T,10] tensor")
            n_tan = dxs.shape[2]
        T = int(n_tan)
        d = self._dptr
        self._check(self._lib.ndp_plant_rollout_jvp_device(
            self._h, K, float(dt), int(substeps), d(x0, torch.float64, (B, 10)), d(u, torch.float64, (K, B, 4)),
            d(f, torch.float64, (K, B, 3)), T, d(tx0, torch.float64, (B, T, 10)), d(tu, torch.float64, (K, B, T, 4)),
            d(tf, torch.float64, (K, B, T, 3)), d(dxs, torch.float64, (K, B, T, 10)), d(xs_check, torch.float64, (K, B, 10)),
            self._stream(stream)), "ndp_plant_rollout_jvp_device")

    # ---- the closed loop over given windows and forces, recorded, and its reverse mode: one call per direction
    def closed_loop_tape(self, ticks):
        """A tape for closed_loop_device over `ticks` ticks: a uint8 CUDA tensor [ticks, slot bytes] (ndp_closed_loop_tape_bytes).  Slot k
        holds what step k started from; closed_loop_tape_slot gives its three arrays."""
        import torch
        n = C.c_size_t(0)
        self._check(self._lib.ndp_closed_loop_tape_bytes(self._h, int(ticks), C.byref(n)), "ndp_closed_loop_tape_bytes")
        if n.value != int(ticks) * self._closed_loop_slot_bytes():
            raise NdpError(f"closed_loop_tape: the library's tape is {n.value} bytes, this binding expects {int(ticks) * self._closed_loop_slot_bytes()}")
        return torch.empty((int(ticks), self._closed_loop_slot_bytes()), dtype=torch.uint8, device=torch.device("cuda", self.cfg.device))

    def _closed_loop_slot_bytes(self):
        B, N = self.B, self.N
        return (B * ((N + 1) * 10 * 8 + N * 4 * 8 + N * 4) + 255) // 256 * 256        # (closed_loop.hip: cl_slot_bytes)

    def closed_loop_tape_slot(self, tape, k):
        """(X_lin [B,N+1,10] float64, U_lin [B,N,4] float64, act_lin [B,N,4] int8): views of slot k of a tape, as record_tape returns
        them and step_vjp_device takes them."""
        import torch
        B, N = self.B, self.N
        nx, nu, na = B * (N + 1) * 10 * 8, B * N * 4 * 8, B * N * 4
        row = tape[k]
        return (row[:nx].view(torch.float64).view(B, N + 1, 10), row[nx:nx + nu].view(torch.float64).view(B, N, 4),
                row[nx + nu:nx + nu + na].view(torch.int8).view(B, N, 4))

    def _closed_loop_args(self, who, x0, xr, ur, f, fp):
        import torch
        if not (isinstance(xr, torch.Tensor) and xr.dim() == 4 and xr.shape[0] >= 1):
            raise ValueError(f"{who}: xr must be a [ticks,B,N+1,10] tensor with ticks >= 1")
        K, B, N, d = int(xr.shape[0]), self.B, self.N, self._dptr
        return K, [d(x0, torch.float64, (B, 10)), d(xr, torch.float64, (K, B, N + 1, 10)), d(ur, torch.float64, (K, B, N, 4)),
                   d(f, torch.float32, (K, B, N + 1, 3)), d(fp, torch.float64, (K, B, 3))]

    def _torch_default_wait(self, stream):
        """stream None or torch's default stream: the call goes on the engine's own stream (the C-ABI's NULL), behind a wait for torch's."""
        import torch
        if stream is None or getattr(stream, "cuda_stream", stream) == 0:
            torch.cuda.current_stream(torch.device("cuda", self.cfg.device)).synchronize()

    def closed_loop_device(self, x0, xr, ur, xs, us, f=None, fp=None, Xs=None, status=None, tape=None, dt=CP.ts_nmpc, substeps=4,
                           stream=None):
        """Enqueues the closed loop over given windows on `stream`, no synchronisation (ndp_closed_loop_device; include/ndp_nmpc.h): from
        the engine's current iterate and kept sets, per tick the control step at the plant state with xr[k], ur[k] and the float32 force
        f[k] the controller sees, then the plant tick with u0_k and the force fp[k] on the plant.  x0[B,10], xr[ticks,B,N+1,10],
        ur[ticks,B,N,4], f[ticks,B,N+1,3] float32 or None, fp[ticks,B,3] or None; outputs xs[ticks,B,10] (x_{k+1}), us[ticks,B,4] (u0_k),
        optional Xs[ticks,B,N+1,10], status[ticks,B] int32 and tape (closed_loop_tape(ticks): what closed_loop_vjp_device needs).  ticks is
        read from xr.  Values, status words and the engine's state afterwards are bit-equal to the loop of update_device and
        ndp_plant_step_device.  stream None or torch's default: the engine's own stream behind a wait for torch's."""
        import torch
        K, args = self._closed_loop_args("closed_loop_device", x0, xr, ur, f, fp)
        B, N, d = self.B, self.N, self._dptr
        self._torch_default_wait(stream)
        self._check(self._lib.ndp_closed_loop_device(
            self._h, K, float(dt), int(substeps), *args, d(xs, torch.float64, (K, B, 10)), d(us, torch.float64, (K, B, 4)),
            d(Xs, torch.float64, (K, B, N + 1, 10)), d(status, torch.int32, (K, B)),
            d(tape, torch.uint8, (K, self._closed_loop_slot_bytes())),
            self._stream(stream)), "ndp_closed_loop_device")

    def closed_loop_vjp_device(self, x0, xr, ur, xs, us, tape, f=None, fp=None, gxs=None, gus=None, gXs=None, gx0=None, gxr=None, gur=None,
                               gf=None, gfp=None, gmodel=None, status_check=None, dt=CP.ts_nmpc, substeps=4, stream=None):
        """Enqueues the reverse mode of closed_loop_device on `stream` (ndp_closed_loop_vjp_device; include/ndp_nmpc.h) for
        L = sum_k <gxs[k], x_{k+1}> + <gus[k], u0_k> + <gXs[k], X_k>: the inputs as the forward took them, its xs, us and tape; upstreams
        gxs[ticks,B,10], gus[ticks,B,4], gXs[ticks,B,N+1,10] (None = 0, not all None); float64 outputs the caller allocates (None = not
        written, not all None): gx0[B,10], gxr, gur as xr, ur, gf[ticks,B,N+1,3], gfp[ticks,B,3], gmodel[B,16] (per vehicle, summed over
        the ticks: dL/dQd [0:10], dL/dRd [10:14], the controller's mass share [14], the plant's [15]); status_check[ticks,B] int32.  Every
        tick's linearisation point and final set are held fixed.  Nothing of the engine's state or the tape is written; two calls are
        bit-identical.  stream None or torch's default: the engine's own stream behind a wait for torch's; read the outputs after
        engine.synchronize()."""
        import torch
        K, args = self._closed_loop_args("closed_loop_vjp_device", x0, xr, ur, f, fp)
        B, N, d = self.B, self.N, self._dptr
        self._torch_default_wait(stream)
        self._check(self._lib.ndp_closed_loop_vjp_device(
            self._h, K, float(dt), int(substeps), *args, d(xs, torch.float64, (K, B, 10)), d(us, torch.float64, (K, B, 4)),
            d(tape, torch.uint8, (K, self._closed_loop_slot_bytes())),
            d(gxs, torch.float64, (K, B, 10)), d(gus, torch.float64, (K, B, 4)), d(gXs, torch.float64, (K, B, N + 1, 10)),
            d(gx0, torch.float64, (B, 10)), d(gxr, torch.float64, (K, B, N + 1, 10)), d(gur, torch.float64, (K, B, N, 4)),
            d(gf, torch.float64, (K, B, N + 1, 3)), d(gfp, torch.float64, (K, B, 3)), d(gmodel, torch.float64, (B, 16)),
            d(status_check, torch.int32, (K, B)), self._stream(stream)), "ndp_closed_loop_vjp_device")

    def closed_loop_jvp_device(self, x0, xr, ur, xs, us, tape, dxs, dus, f=None, fp=None, tx0=None, txr=None, tur=None, tf=None, tfp=None,
                               dXs=None, dUs=None, status_check=None, n_tan=None, dt=CP.ts_nmpc, substeps=4, stream=None, tmodel=None):
        """Enqueues the forward mode of closed_loop_device on `stream` (ndp_closed_loop_jvp_device; include/ndp_nmpc.h): the inputs as the
        forward took them, its xs, us and tape.  Directions (None = 0, not all None), float64: tx0[B,T,10], txr[ticks,B,T,N+1,10],
        tur[ticks,B,T,N,4], tf[ticks,B,T,N+1,3], tfp[ticks,B,T,3].  Outputs the caller allocates, float64, overwritten: dxs[ticks,B,T,10]
        and dus[ticks,B,T,4], required -- the first-order change of x_{k+1} and of u0_k; dXs[ticks,B,T,N+1,10], dUs[ticks,B,T,N,4] and
        status_check[ticks,B] int32, optional.  T (1..8) is n_tan when given, else read from dxs.  Every tick's linearisation point and
        final set are held fixed.  Nothing of the engine's state or the tape is written; T directions in one call equal T calls bit for
        bit.  stream None or torch's default: the engine's own stream behind a wait for torch's; read the outputs after
        engine.synchronize().
        tmodel [B,T,16] float64 (given: the call is ndp_closed_loop_jvp_model_device, and the data directions may all be None): the
        model's direction, constant over the ticks: Qd' [0:10], Rd' [10:14], the controller's mass' [14], the plant's mass' [15]."""
        import torch
        K, args = self._closed_loop_args("closed_loop_jvp_device", x0, xr, ur, f, fp)
        if n_tan is None:
            if not (isinstance(dxs, torch.Tensor) and dxs.dim() == 4):
                raise ValueError("closed_loop_jvp_device: dxs must be a [ticks,B,T,10] tensor")
            n_tan = dxs.shape[2]
        B, N, T, d = self.B, self.N, int(n_tan), self._dptr
        self._torch_default_wait(stream)
        name = "ndp_closed_loop_jvp_device" if tmodel is None else "ndp_closed_loop_jvp_model_device"
        model = () if tmodel is None else (d(tmodel, torch.float64, (B, T, 16)),)      # (behind tfp)
        self._check(getattr(self._lib, name)(
            self._h, K, float(dt), int(substeps), *args, d(xs, torch.float64, (K, B, 10)), d(us, torch.float64, (K, B, 4)),
            d(tape, torch.uint8, (K, self._closed_loop_slot_bytes())), T,
            d(tx0, torch.float64, (B, T, 10)), d(txr, torch.float64, (K, B, T, N + 1, 10)), d(tur, torch.float64, (K, B, T, N, 4)),
            d(tf, torch.float64, (K, B, T, N + 1, 3)), d(tfp, torch.float64, (K, B, T, 3)), *model,
            d(dxs, torch.float64, (K, B, T, 10)), d(dus, torch.float64, (K, B, T, 4)), d(dXs, torch.float64, (K, B, T, N + 1, 10)),
            d(dUs, torch.float64, (K, B, T, N, 4)), d(status_check, torch.int32, (K, B)), self._stream(stream)), name)

    # ---- the closed loop of a formation: the plant force made inside the loop from the configured index, and its reverse mode
    def closed_loop_formation_config(self, other_index):
        """Configures the formation of closed_loop_formation_device (ndp_closed_loop_formation_config; include/ndp_nmpc.h): other_index a
        HOST int32 [B,K] array, 1 <= K <= 8 (< 0 or >= B: an empty slot); None clears it.  Synchronous: the handle keeps a device copy of
        the index and its reverse lists (who hears vehicle v), built on the host."""
        self._form_K = self._form_index = None
        if other_index is None:
            self._check(self._lib.ndp_closed_loop_formation_config(self._h, None, 0), "ndp_closed_loop_formation_config")
            return
        oi, K = self._index_multi(other_index)
        self._check(self._lib.ndp_closed_loop_formation_config(self._h, _lib.ptr(oi), K), "ndp_closed_loop_formation_config")
        self._form_K, self._form_index = K, oi.copy()       # (what is configured: torch_layer configures only what is not)

    def plant_force_scatter_device(self, gz, gx, stream=None):
        """Enqueues the scatter of plant_force_multi_vjp_device's gz[B,K,6] (K the configured one) onto the states, gx[B,10] float64,
        overwritten (ndp_plant_force_scatter_device): per vehicle the sum over the slots that hear it, in ascending slot number, minus the
        sum over its own slots; empty and self slots left out; columns 6..9 exactly 0.  A gather: no atomics, two calls bit-identical."""
        import torch
        # (nothing configured: any K lets the call through to the library, which refuses it with its reason)
        K = self._form_K or (gz.shape[1] if isinstance(gz, torch.Tensor) and gz.dim() == 3 else 1)
        self._check(self._lib.ndp_plant_force_scatter_device(
            self._h, self._dptr(gz, torch.float64, (self.B, K, 6)), self._dptr(gx, torch.float64, (self.B, 10)), self._stream(stream)),
            "ndp_plant_force_scatter_device")

    def closed_loop_formation_device(self, x0, xr, ur, xs, us, fps, f=None, Xs=None, status=None, tape=None, gate=True, plant_scale=1.0,
                                     dt=CP.ts_nmpc, substeps=4, stream=None):
        """closed_loop_device with the force on the plant made inside the loop (ndp_closed_loop_formation_device; include/ndp_nmpc.h): per
        tick fps[k] = plant_force_multi_device(x_k, the configured index, gate, plant_scale), the control step with xr[k], ur[k] and the
        given f[k], the plant tick with fps[k].  fps[ticks,B,3] float64 is an output, required; the others as closed_loop_device.
        Everything written is bit-equal to the loop of plant_force_multi_device, update_device and ndp_plant_step_device."""
        import torch
        K, args = self._closed_loop_args("closed_loop_formation_device", x0, xr, ur, f, None)
        B, N, d = self.B, self.N, self._dptr
        self._torch_default_wait(stream)
        self._check(self._lib.ndp_closed_loop_formation_device(
            self._h, K, float(dt), int(substeps), 1 if gate else 0, float(plant_scale), *args[:4], d(xs, torch.float64, (K, B, 10)),
            d(us, torch.float64, (K, B, 4)), d(fps, torch.float64, (K, B, 3)), d(Xs, torch.float64, (K, B, N + 1, 10)),
            d(status, torch.int32, (K, B)), d(tape, torch.uint8, (K, self._closed_loop_slot_bytes())), self._stream(stream)),
            "ndp_closed_loop_formation_device")

    def closed_loop_formation_vjp_device(self, x0, xr, ur, xs, us, fps, tape, f=None, gxs=None, gus=None, gXs=None, gfps=None, gx0=None,
                                         gxr=None, gur=None, gf=None, gw=None, gmodel=None, status_check=None, gate=True, plant_scale=1.0,
                                         dt=CP.ts_nmpc, substeps=4, stream=None):
        """Enqueues the reverse mode of closed_loop_formation_device on `stream` (ndp_closed_loop_formation_vjp_device) for
        L = sum_k <gxs[k], x_{k+1}> + <gus[k], u0_k> + <gXs[k], X_k> + <gfps[k], fps[k]>: the inputs as the forward took them, its xs, us,
        fps and tape; upstreams None = 0, not all None; outputs as closed_loop_vjp_device's, with gw[17859] float32 (overwritten: the
        gradient in the network's weights, summed over the ticks in float64 and rounded once) in place of gfp.  Linearisation points, final
        sets and gates are held fixed; gradients cross the vehicles through a gather on the device, no atomics, two calls bit-identical."""
        import torch
        K, args = self._closed_loop_args("closed_loop_formation_vjp_device", x0, xr, ur, f, None)
        B, N, d = self.B, self.N, self._dptr
        self._torch_default_wait(stream)
        self._check(self._lib.ndp_closed_loop_formation_vjp_device(
            self._h, K, float(dt), int(substeps), 1 if gate else 0, float(plant_scale), *args[:4], d(xs, torch.float64, (K, B, 10)),
            d(us, torch.float64, (K, B, 4)), d(fps, torch.float64, (K, B, 3)), d(tape, torch.uint8, (K, self._closed_loop_slot_bytes())),
            d(gxs, torch.float64, (K, B, 10)), d(gus, torch.float64, (K, B, 4)), d(gXs, torch.float64, (K, B, N + 1, 10)),
            d(gfps, torch.float64, (K, B, 3)), d(gx0, torch.float64, (B, 10)), d(gxr, torch.float64, (K, B, N + 1, 10)),
            d(gur, torch.float64, (K, B, N, 4)), d(gf, torch.float64, (K, B, N + 1, 3)), d(gw, torch.float32, (_lib.MLP_NPARAM,)),
            d(gmodel, torch.float64, (B, 16)), d(status_check, torch.int32, (K, B)), self._stream(stream)),
            "ndp_closed_loop_formation_vjp_device")

    @staticmethod
    def _plant_ticks(u, who):
        import torch
        if not (isinstance(u, torch.Tensor) and u.dim() == 3 and u.shape[0] >= 1):
            raise ValueError(f"{who}: u must be a [ticks,B,4] tensor with ticks >= 1")
        return int(u.shape[0])

    # ---- f4, the formation form: the downwash acting on the plant
    def plant_force(self, x, other_index, gate=True, scale=1.0):
        """The downwash force on every vehicle from the plant states x[B,10] (ndp_plant_force; include/ndp_nmpc.h): vehicle v feels the
        network at (x[other_index[v]] - x[v])[0:6] behind the r_horiz gate (gate=False: open everywhere); other_index int32[B], < 0 =
        none, None = nobody has a neighbour.  Returns f[B,3] float64 = scale * net, exactly 0 where closed."""
        x = _lib.f64(x, (self.B, 10))
        oi = None if other_index is None else np.ascontiguousarray(other_index, dtype=np.int32).reshape(self.B)
        f = np.empty((self.B, 3))
        self._check(self._lib.ndp_plant_force(self._h, _lib.ptr(x), _lib.ptr(oi), 1 if gate else 0, float(scale), _lib.ptr(f)), "ndp_plant_force")
        return f

    def plant_force_device(self, x, other_index, f_out, xy_out=None, gate=True, scale=1.0, stream=None):
        """plant_force on CUDA tensors, enqueued on `stream` with no synchronisation (ndp_plant_force_device): x[B,10] float64,
        other_index int32[B] or None, f_out[B,3] float64; xy_out[B,2] float64 (optional) receives x[:, 0:2], the ego_xy of update_device."""
        import torch
        self._check(self._lib.ndp_plant_force_device(
            self._h, self._dptr(x, torch.float64, (self.B, 10)), self._dptr(other_index, torch.int32, (self.B,)), 1 if gate else 0, float(scale),
            self._dptr(f_out, torch.float64, (self.B, 3)), self._dptr(xy_out, torch.float64, (self.B, 2)), self._stream(stream)),
            "ndp_plant_force_device")

    def rollout_formation_device(self, ticks, x, other_index, log=None, log_u=None, log_f=None, worst_status=None, t0=0.0, dt=CP.ts_nmpc,
                                 substeps=4, gate=True, compensate=None, plant_scale=1.0, stream=None):
        """rollout_device with the downwash acting on the plant (ndp_rollout_formation_device; include/ndp_nmpc.h): per tick reference
        window -> plant force (plant_force_device at scale plant_scale) -> control step -> plant step with that force, held over the tick.
        compensate (default: the engine's `disturbance`): the controller predicts the force from its neighbour's reference window (the
        fused step with other = the batch's reference windows, other_index, ego_xy = the plant's xy); False: it flies blind through the
        same downwash.  x[B,10] is updated in place; other_index int32[B] CUDA tensor (< 0: none) or None; optional CUDA tensors
        log[ticks,B,10] the states, log_u[ticks,B,4] u0, log_f[ticks,B,3] the plant force (float64), worst_status[B] int32 the largest
        status of every vehicle's steps."""
        import torch
        K, B = int(ticks), self.B
        comp = self.disturbance if compensate is None else bool(compensate)
        flags = (_lib.FORM_GATE if gate else 0) | (_lib.FORM_COMPENSATE if comp else 0)
        self._check(self._lib.ndp_rollout_formation_device(
            self._h, K, float(t0), float(dt), int(substeps), self._dptr(other_index, torch.int32, (B,)), flags, float(plant_scale),
            self._dptr(x, torch.float64, (B, 10)), self._dptr(log, torch.float64, (K, B, 10)), self._dptr(log_u, torch.float64, (K, B, 4)),
            self._dptr(log_f, torch.float64, (K, B, 3)), self._dptr(worst_status, torch.int32, (B,)), self._stream(stream)),
            "ndp_rollout_formation_device")

    # ---- f4 with K neighbours per vehicle: the forces of the slots superposed (a modelling assumption: the network was trained on pairs)
    def _index_multi(self, other_index):
        """other_index int32[B, K] as a contiguous array -> (array, K)."""
        oi = np.ascontiguousarray(other_index, dtype=np.int32)
        if oi.ndim != 2 or oi.shape[0] != self.B:
            raise ValueError(f"other_index: expected int32 [{self.B}, K], got {tuple(oi.shape)}")
        return oi, int(oi.shape[1])

    def _dindex_multi(self, other_index):
        """other_index int32[B, K] CUDA tensor -> (pointer, K)."""
        import torch
        if not (isinstance(other_index, torch.Tensor) and other_index.dim() == 2):
            raise ValueError(f"other_index: expected a CUDA int32 [{self.B}, K] tensor")
        K = int(other_index.shape[1])
        return self._dptr(other_index, torch.int32, (self.B, K)), K

    def downwash_multi(self, other, other_index, ego_ref, ego_xy=None):
        """downwash with K neighbours per instance (ndp_downwash_multi; include/ndp_nmpc.h): other[B,N+1,10] the batch's windows,
        other_index int32[B,K] the rows of `other` instance i hears (< 0: an empty slot).  Returns f[B,N+1,3] float32: the fp32 sum, in slot
        order, of what downwash gives per slot, each slot behind its own gate (ego_xy[B,2]; None: open)."""
        other = _lib.f64(other, (self.B, self.N + 1, 10))
        ego_ref = _lib.f64(ego_ref, (self.B, self.N + 1, 10))
        ego_xy = _lib.f64(ego_xy, (self.B, 2))
        oi, K = self._index_multi(other_index)
        f = np.empty((self.B, self.N + 1, 3), dtype=np.float32)
        self._check(self._lib.ndp_downwash_multi(self._h, _lib.ptr(other), _lib.ptr(oi), K, _lib.ptr(ego_ref), _lib.ptr(ego_xy), _lib.ptr(f)),
                    "ndp_downwash_multi")
        return f

    def downwash_multi_device(self, other, other_index, ego_ref, f_out, ego_xy=None, stream=None):
        """downwash_multi on CUDA tensors, enqueued on `stream` with no synchronisation (ndp_downwash_multi_device): other [rows,N+1,6 or
        10] float64 as update_device takes it with other_index, other_index int32[B,K], ego_ref[B,N+1,10], f_out[B,N+1,3] float32 (the
        `f` of update_device), ego_xy[B,2] or None."""
        import torch
        B, N = self.B, self.N
        optr, stride = self._other_ptr(other, other_index)
        iptr, K = self._dindex_multi(other_index)
        self._check(self._lib.ndp_downwash_multi_device(
            self._h, optr, stride, iptr, K, self._dptr(ego_ref, torch.float64, (B, N + 1, 10)), self._dptr(ego_xy, torch.float64, (B, 2)),
            self._dptr(f_out, torch.float32, (B, N + 1, 3)), self._stream(stream)), "ndp_downwash_multi_device")

    def plant_force_multi(self, x, other_index, gate=True, scale=1.0):
        """plant_force with K neighbours per vehicle (ndp_plant_force_multi): other_index int32[B,K] (< 0 or >= B: an empty slot).  Returns
        f[B,3] float64: the fp64 sum, in slot order, of what plant_force gives per slot."""
        x = _lib.f64(x, (self.B, 10))
        oi, K = self._index_multi(other_index)
        f = np.empty((self.B, 3))
        self._check(self._lib.ndp_plant_force_multi(self._h, _lib.ptr(x), _lib.ptr(oi), K, 1 if gate else 0, float(scale), _lib.ptr(f)),
                    "ndp_plant_force_multi")
        return f

    def plant_force_multi_device(self, x, other_index, f_out, xy_out=None, gate=True, scale=1.0, stream=None):
        """plant_force_multi on CUDA tensors, enqueued on `stream` with no synchronisation (ndp_plant_force_multi_device): x[B,10] float64,
        other_index int32[B,K], f_out[B,3] float64; xy_out[B,2] float64 (optional) receives x[:, 0:2]."""
        import torch
        iptr, K = self._dindex_multi(other_index)
        self._check(self._lib.ndp_plant_force_multi_device(
            self._h, self._dptr(x, torch.float64, (self.B, 10)), iptr, K, 1 if gate else 0, float(scale),
            self._dptr(f_out, torch.float64, (self.B, 3)), self._dptr(xy_out, torch.float64, (self.B, 2)), self._stream(stream)),
            "ndp_plant_force_multi_device")

    # ---- the derivatives of the plant force (ndp_plant_force*_vjp_device, ndp_plant_force*_jvp_device; include/ndp_nmpc.h)
    def _slots_of(self, other_index, *shaped):
        """K of a multi call: other_index int32[B,K], or -- other_index None -- the slot axis of the first output given (else 1)."""
        if other_index is not None:
            return self._dindex_multi(other_index)
        for t, pos in shaped:
            if t is not None and t.dim() > pos:
                return None, int(t.shape[pos])
        return None, 1

    def plant_force_multi_vjp_device(self, x, other_index, gf, gz=None, gw=None, gate=True, scale=1.0, stream=None):
        """Enqueues the backward pass of plant_force_multi_device on `stream` (ndp_plant_force_multi_vjp_device): x[B,10] float64,
        other_index int32[B,K] or None, gf[B,3] float64 the gradient of the summed force.  Outputs (None = not computed, not both None):
        gz [B,K,6] float64, the gradient per network input row, 0 on closed and empty slots -- the scatter onto the states (+gz to
        x[o][0:6], -gz to x[v][0:6]) is the caller's (torch_layer.plant_force does it); gw [17859] float32, overwritten, two calls
        bit-identical.  A vehicle whose gf row (or a slot whose input) is not finite adds nothing to gw and has NaN in its gz.  Shares
        downwash_vjp_device's workspace: order the calls against each other.  The engine's state is not written.  stream None or torch's
        default stream: as downwash_vjp_device."""
        import torch
        B = self.B
        self._torch_default_wait(stream)
        iptr, K = self._slots_of(other_index, (gz, 1))
        d = self._dptr
        self._check(self._lib.ndp_plant_force_multi_vjp_device(
            self._h, d(x, torch.float64, (B, 10)), iptr, K, 1 if gate else 0, float(scale), d(gf, torch.float64, (B, 3)),
            d(gz, torch.float64, (B, K, 6)), d(gw, torch.float32, (_lib.MLP_NPARAM,)), self._stream(stream)),
            "ndp_plant_force_multi_vjp_device")

    def plant_force_vjp_device(self, x, other_index, gf, gz=None, gw=None, gate=True, scale=1.0, stream=None):
        """plant_force_multi_vjp_device with one neighbour per vehicle (ndp_plant_force_vjp_device): other_index int32[B] or None,
        gz [B,6].  The K = 1 case, bit for bit."""
        import torch
        B = self.B
        self._torch_default_wait(stream)
        d = self._dptr
        self._check(self._lib.ndp_plant_force_vjp_device(
            self._h, d(x, torch.float64, (B, 10)), d(other_index, torch.int32, (B,)), 1 if gate else 0, float(scale),
            d(gf, torch.float64, (B, 3)), d(gz, torch.float64, (B, 6)), d(gw, torch.float32, (_lib.MLP_NPARAM,)), self._stream(stream)),
            "ndp_plant_force_vjp_device")

    def _plant_force_tangents(self, who, tx, tw, df, n_tan):
        """(T, tx, tw, df pointers) of a forward-mode call of the plant force."""
        import torch
        d = self._dptr
        T, (stx, stw, sdf) = _t_axis_shapes(who, self.B, (
            (getattr(tx, "shape", None), (10,), 1), (getattr(tw, "shape", None), (_lib.MLP_NPARAM,), 0), (getattr(df, "shape", None), (3,), 1)), n_tan)
        return T, d(tx, torch.float64, stx), d(tw, torch.float32, stw), d(df, torch.float64, sdf)

    def plant_force_multi_jvp_device(self, x, other_index, tx=None, tw=None, n_tan=None, df=None, f_check=None, gate=True, scale=1.0,
                                     stream=None):
        """Enqueues the forward mode of plant_force_multi_device on `stream` (ndp_plant_force_multi_jvp_device).  Directions (None = 0, not
        both None): tx [B,T,10] float64, directions of the STATES -- the kernel gathers a slot's input direction tx[o] - tx[v], so no
        scatter is needed; tw [T,17859] float32.  Outputs: df [B,T,3] float64, required -- the float64 sum in slot order of scale x the
        slots' tangents, exactly 0 where no slot is open; f_check [B,3] float64, optional -- bit-equal to plant_force_multi_device's force.
        T (1..8) is n_tan when given, else read from the tensors; tensors without the T axis mean T = 1.  T directions in one call equal T
        calls bit for bit.  No workspace; the engine's state is not written.  stream None or torch's default stream: as
        downwash_jvp_device."""
        import torch
        B = self.B
        self._torch_default_wait(stream)
        iptr, K = self._slots_of(other_index)
        T, ptx, ptw, pdf = self._plant_force_tangents("plant_force_multi_jvp_device", tx, tw, df, n_tan)
        d = self._dptr
        self._check(self._lib.ndp_plant_force_multi_jvp_device(
            self._h, d(x, torch.float64, (B, 10)), iptr, K, 1 if gate else 0, float(scale), T, ptx, ptw, pdf,
            d(f_check, torch.float64, (B, 3)), self._stream(stream)), "ndp_plant_force_multi_jvp_device")

    def plant_force_jvp_device(self, x, other_index, tx=None, tw=None, n_tan=None, df=None, f_check=None, gate=True, scale=1.0, stream=None):
        """plant_force_multi_jvp_device with one neighbour per vehicle (ndp_plant_force_jvp_device): other_index int32[B] or None.  The
        K = 1 case, bit for bit."""
        import torch
        B = self.B
        self._torch_default_wait(stream)
        T, ptx, ptw, pdf = self._plant_force_tangents("plant_force_jvp_device", tx, tw, df, n_tan)
        d = self._dptr
        self._check(self._lib.ndp_plant_force_jvp_device(
            self._h, d(x, torch.float64, (B, 10)), d(other_index, torch.int32, (B,)), 1 if gate else 0, float(scale), T, ptx, ptw, pdf,
            d(f_check, torch.float64, (B, 3)), self._stream(stream)), "ndp_plant_force_jvp_device")

    def rollout_formation_multi_device(self, ticks, x, other_index, log=None, log_u=None, log_f=None, worst_status=None, t0=0.0,
                                       dt=CP.ts_nmpc, substeps=4, gate=True, compensate=None, plant_scale=1.0, stream=None):
        """rollout_formation_device with K neighbours per vehicle (ndp_rollout_formation_multi_device; include/ndp_nmpc.h): other_index
        int32[B,K] CUDA tensor (< 0: an empty slot) or None.  The plant feels the sum of the slots' forces (plant_force_multi_device); with
        compensate the controller is given the sum of the slots' predictions (downwash_multi_device on the batch's reference windows, then
        the step with that f).  Everything else as rollout_formation_device."""
        import torch
        T, B = int(ticks), self.B
        comp = self.disturbance if compensate is None else bool(compensate)
        flags = (_lib.FORM_GATE if gate else 0) | (_lib.FORM_COMPENSATE if comp else 0)
        iptr, K = (None, 1) if other_index is None else self._dindex_multi(other_index)
        self._check(self._lib.ndp_rollout_formation_multi_device(
            self._h, T, float(t0), float(dt), int(substeps), iptr, K, flags, float(plant_scale),
            self._dptr(x, torch.float64, (B, 10)), self._dptr(log, torch.float64, (T, B, 10)), self._dptr(log_u, torch.float64, (T, B, 4)),
            self._dptr(log_f, torch.float64, (T, B, 3)), self._dptr(worst_status, torch.int32, (B,)), self._stream(stream)),
            "ndp_rollout_formation_multi_device")

    def get_iterate(self):
        X = np.empty((self.B, self.N + 1, 10))
        U = np.empty((self.B, self.N, 4))
        self._check(self._lib.ndp_get_iterate(self._h, _lib.ptr(X), _lib.ptr(U)), "ndp_get_iterate")
        return X, U

    def set_iterate(self, X=None, U=None):
        X = _lib.f64(X, (self.B, self.N + 1, 10))
        U = _lib.f64(U, (self.B, self.N, 4))
        self._check(self._lib.ndp_set_iterate(self._h, _lib.ptr(X), _lib.ptr(U)), "ndp_set_iterate")

    def set_model(self, Qd=None, Rd=None, mass=None):
        """Changes the cost weights Qd [10], Rd [4] and / or the mass of the live engine (ndp_set_model; include/ndp_nmpc.h); None = keep.
        Waits for the engine's work in flight.  The iterate, kept sets, network weights and estimator state stay: the next step is
        warm-started as before, and bit-equal to a fresh engine's with these values and that state.  A refused value (negative Qd,
        non-positive Rd or mass, an Rd above what as_gamma holds) raises NdpError and changes nothing.  self.cfg follows."""
        q = None if Qd is None else _lib.f64(Qd, (10,))
        r = None if Rd is None else _lib.f64(Rd, (4,))
        m = 0.0 if mass is None else float(mass)
        if mass is not None and not m > 0.0:
            raise NdpError(f"set_model: the mass must be positive (got {m})")
        self._check(self._lib.ndp_set_model(self._h, _lib.ptr(q), _lib.ptr(r), m), "ndp_set_model")
        if q is not None:
            self.cfg.Qd[:] = [float(v) for v in q]
        if r is not None:
            self.cfg.Rd[:] = [float(v) for v in r]
        if mass is not None:
            self.cfg.mass = m

    def status(self):
        st = np.zeros(self.B, dtype=np.int32)
        it = np.zeros(self.B, dtype=np.int32)
        self._check(self._lib.ndp_get_status(self._h, _lib.ptr(st), _lib.ptr(it)), "ndp_get_status")
        return st, it

    def host_info(self):
        """{hw_threads, usable_cores, pack_threads} of the host-array path (ndp_debug_host_info)."""
        out = np.zeros(3, dtype=np.int32)
        self._check(self._lib.ndp_debug_host_info(self._h, _lib.ptr(out)), "ndp_debug_host_info")
        return {"hw_threads": int(out[0]), "usable_cores": int(out[1]), "pack_threads": int(out[2])}

    def active_set(self):
        """(sweeps[B], act[B,N,4]) of the last step's QPs (ndp_get_active_set): Riccati sweeps taken by QP_AUTO's active-set
        iterations, and the set kept for the next step (+1 / -1: input on its upper / lower bound)."""
        sw = np.zeros(self.B, dtype=np.int32)
        act = np.zeros((self.B, self.N, 4), dtype=np.int8)
        self._check(self._lib.ndp_get_active_set(self._h, _lib.ptr(sw), _lib.ptr(act)), "ndp_get_active_set")
        return sw & 0xfff, act

    def set_active_set(self, act):
        """The kept sets handed in (act[B,N,4] int8, entries -1 / 0 / +1): the warm start of the next step's QPs (ndp_set_active_set;
        after set_iterate, which empties them)."""
        a = np.ascontiguousarray(act, dtype=np.int8).reshape(self.B, self.N, 4)
        self._check(self._lib.ndp_set_active_set(self._h, _lib.ptr(a)), "ndp_set_active_set")

    def condensed_kept(self):
        """qp_precision 5 / 6 (config 5's condensed study): how many of the last step's QPs per instance kept their condensed solve's
        result (it passed the fp64 inside-the-box test); the others were solved by the fp64 Riccati path."""
        sw = np.zeros(self.B, dtype=np.int32)
        self._check(self._lib.ndp_get_active_set(self._h, _lib.ptr(sw), None), "ndp_get_active_set")
        return (sw >> 12) & 0xf

    # ------------------------------------------------------------------ initial-state sensitivities
    def enable_sensitivity(self, level=1):
        """Every later step also writes the derivative of its QP with respect to x0 (ndp_sens_enable; include/ndp_nmpc.h): level 1
        du0/dx0, level 2 also dU/dx0 and dX/dx0, 0 off.  N <= 27, qp_precision 0 and n_rti = 1 only; with sensitivities on, the
        tick, late-force and rollout entry points raise."""
        self._check(self._lib.ndp_sens_enable(self._h, int(level)), "ndp_sens_enable")

    @property
    def sensitivity_level(self):
        return int(self._lib.ndp_sens_level(self._h))

    def sensitivity(self):
        """(du0_dx0 [B,4,10], dU_dx0 [B,N,4,10], dX_dx0 [B,N+1,10,10]) of the last step, numpy float64; the last two are None at level 1.
        Column j = d / dx0[j]; rows of pinned inputs are 0; an instance with a nonzero status is NaN throughout."""
        lvl = self.sensitivity_level
        if lvl < 1:
            raise NdpError("sensitivities are not enabled (enable_sensitivity)")
        du0 = np.empty((self.B, 4, 10))
        dU = np.empty((self.B, self.N, 4, 10)) if lvl >= 2 else None
        dX = np.empty((self.B, self.N + 1, 10, 10)) if lvl >= 2 else None
        self._check(self._lib.ndp_get_sens(self._h, _lib.ptr(du0), _lib.ptr(dU), _lib.ptr(dX)), "ndp_get_sens")
        return du0, dU, dX

    def _device_views(self, *views):
        """CUDA tensor views (no copy) of the handle's buffers: views = (C getter, shape[, typestr; float64 without]); None for a buffer
        that is not there."""
        import torch
        from .dist import _DevMem
        dev = torch.device("cuda", self.cfg.device)
        ptrs = [(fn(self._h), rest) for fn, *rest in views]
        return tuple(torch.as_tensor(_DevMem(ptr, *rest), device=dev) if ptr else None for ptr, rest in ptrs)

    def device_sensitivity(self):
        """The device buffers as CUDA tensor views (no copy): (du0_dx0 [B,4,10], dU_dx0 [B,N,4,10] or None, dX_dx0 [B,N+1,10,10] or
        None), float64.  Valid once the step's stream has reached them; the next step overwrites them."""
        if self.sensitivity_level < 1:
            raise NdpError("sensitivities are not enabled (enable_sensitivity)")
        return self._device_views((self._lib.ndp_device_sens_u0, (self.B, 4, 10)), (self._lib.ndp_device_sens_u, (self.B, self.N, 4, 10)),
                                  (self._lib.ndp_device_sens_x, (self.B, self.N + 1, 10, 10)))

    def enable_param_sensitivity(self, on=True):
        """Every later step also writes the derivative of its QP with respect to xr, ur and the force f (ndp_sens_params_enable;
        include/ndp_nmpc.h): du0/dxr [B,4,N+1,10], du0/dur [B,4,N,4], du0/df [B,4,N+1,3].  Needs enable_sensitivity(1 or 2) first;
        enable_sensitivity(0) switches them off too.  At N != 20 the step must be the fused one (neighbour windows given)."""
        self._check(self._lib.ndp_sens_params_enable(self._h, int(bool(on))), "ndp_sens_params_enable")

    @property
    def param_sensitivity_enabled(self):
        return bool(self._lib.ndp_sens_params_enabled(self._h) == 1)

    def param_sensitivity(self):
        """(du0_dxr [B,4,N+1,10], du0_dur [B,4,N,4], du0_df [B,4,N+1,3]) of the last step, numpy float64.  Row i = d u0[i]; the rows of
        pinned inputs are 0, stage 0's reference rows and f_N are 0; an instance with a nonzero status is NaN throughout."""
        if not self.param_sensitivity_enabled:
            raise NdpError("parameter sensitivities are not enabled (enable_param_sensitivity)")
        dxr = np.empty((self.B, 4, self.N + 1, 10))
        dur = np.empty((self.B, 4, self.N, 4))
        df = np.empty((self.B, 4, self.N + 1, 3))
        self._check(self._lib.ndp_get_sens_params(self._h, _lib.ptr(dxr), _lib.ptr(dur), _lib.ptr(df)), "ndp_get_sens_params")
        return dxr, dur, df

    def device_param_sensitivity(self):
        """The device buffers as CUDA tensor views (no copy): (du0_dxr [B,4,N+1,10], du0_dur [B,4,N,4], du0_df [B,4,N+1,3]), float64.
        Valid once the step's stream has reached them; the next step overwrites them."""
        if not self.param_sensitivity_enabled:
            raise NdpError("parameter sensitivities are not enabled (enable_param_sensitivity)")
        return self._device_views((self._lib.ndp_device_sens_xr, (self.B, 4, self.N + 1, 10)), (self._lib.ndp_device_sens_ur, (self.B, 4, self.N, 4)),
                                  (self._lib.ndp_device_sens_f, (self.B, 4, self.N + 1, 3)))

    # ------------------------------------------------------------------ adjoint of the control step (reverse mode)
    def record_tape(self, stream=None):
        """(X_lin [B,N+1,10] float64, U_lin [B,N,4] float64, act_lin [B,N,4] int8): device clones of the iterate and kept active sets the
        NEXT step on `stream` (a torch CUDA stream; default: the current one) starts from -- what step_vjp_device needs, beside that
        step's own x0, xr, ur and force, to differentiate it later (ndp_step_vjp_device).  The clones are ordered on `stream`: record the
        tape on the stream the step will run on, before it.  torch's default stream cannot be named through the C-ABI (a NULL stream is
        the engine's own), so there the engine's work is waited for first and the clones after."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(torch.device("cuda", self.cfg.device))
        default = s.cuda_stream == 0
        if default:
            self.synchronize()
        with torch.cuda.stream(s):
            tape = tuple(v.clone() for v in self._device_views(
                (self._lib.ndp_device_iterate_x, (self.B, self.N + 1, 10)), (self._lib.ndp_device_iterate_u, (self.B, self.N, 4)),
                (self._lib.ndp_device_active_set, (self.B, self.N, 4), "|i1")))
        if default:
            s.synchronize()
        return tape

    def step_vjp_device(self, x0, xr, ur, tape, gu0=None, gX=None, gU=None, f=None, gx0=None, gxr=None, gur=None, gf=None,
                        u0_check=None, status_check=None, stream=None, gmodel=None):
        """Enqueues the adjoint of one recorded step on `stream` (ndp_step_vjp_device; include/ndp_nmpc.h): the step is recomputed from
        `tape` (record_tape) and its x0, xr, ur and fp32 force f (the caller's, or device_force() after a step with neighbour windows;
        None = no force), and the upstream gradients gu0 [B,4], gX [B,N+1,10], gU [B,N,4] (None = 0, not all None) are contracted with
        the derivative of its QP into gx0 [B,10], gxr [B,N+1,10], gur [B,N,4], gf [B,N+1,3] (float64 CUDA tensors the caller allocates;
        None = not written).  u0_check [B,4] float64 / status_check [B] int32: the recompute's u0 and status.  Sensitivities need not be
        on; nothing of the engine's state is written.  stream None or torch's default stream: the call goes on the engine's own stream
        (the C-ABI's NULL) behind a wait for torch's; read the outputs after engine.synchronize().
        gmodel [B,16] float64 (given: the call is ndp_step_vjp_model_device, the same outputs bit for bit plus gmodel): per instance
        dL/dQd [0:10], dL/dRd [10:14], dL/dmass [14], 0 [15]; NaN in all 16 where the step failed.  Sum over the batch yourself."""
        import torch
        B, N = self.B, self.N
        self._torch_default_wait(stream)
        d = self._dptr
        X, U, A = tape
        args = [d(x0, torch.float64, (B, 10)), d(xr, torch.float64, (B, N + 1, 10)), d(ur, torch.float64, (B, N, 4)),
                d(f, torch.float32, (B, N + 1, 3)), d(X, torch.float64, (B, N + 1, 10)), d(U, torch.float64, (B, N, 4)),
                d(A, torch.int8, (B, N, 4)), d(gu0, torch.float64, (B, 4)), d(gX, torch.float64, (B, N + 1, 10)),
                d(gU, torch.float64, (B, N, 4)), d(gx0, torch.float64, (B, 10)), d(gxr, torch.float64, (B, N + 1, 10)),
                d(gur, torch.float64, (B, N, 4)), d(gf, torch.float64, (B, N + 1, 3)), d(u0_check, torch.float64, (B, 4)),
                d(status_check, torch.int32, (B,)), self._stream(stream)]
        name = "ndp_step_vjp_device"
        if gmodel is not None:
            args.insert(14, d(gmodel, torch.float64, (B, 16)))         # (behind gf)
            name = "ndp_step_vjp_model_device"
        self._check(getattr(self._lib, name)(self._h, *args), name)

    def step_jvp_device(self, x0, xr, ur, tape, tx0=None, txr=None, tur=None, tf=None, f=None, du0=None, dX=None, dU=None,
                        u0_check=None, status_check=None, stream=None, tmodel=None):
        """Enqueues the forward-mode derivative of one recorded step on `stream` (ndp_step_jvp_device; include/ndp_nmpc.h): the step is
        recomputed from `tape`, x0, xr, ur and f as step_vjp_device does, and the first-order change of its output along T directions
        (tx0 [B,T,10], txr [B,T,N+1,10], tur [B,T,N,4], tf [B,T,N+1,3]; float64 CUDA tensors, None = 0, not all None) is written into
        du0 [B,T,4], dX [B,T,N+1,10], dU [B,T,N,4] (float64 CUDA tensors the caller allocates; None = not written, not all None).  T
        (1..8) is read from the tangents' second dimension; tangents and outputs without that axis mean T = 1.  u0_check, status_check
        and stream: as step_vjp_device's.  Nothing of the engine's state is written.
        tmodel [B,T,16] float64 (given: the call is ndp_step_jvp_model_device, and the data tangents may all be None): per instance and
        direction Qd' [0:10], Rd' [10:14], mass' [14], [15] not read; it adds to the data tangents' direction."""
        import torch
        B, N = self.B, self.N
        self._torch_default_wait(stream)
        tails = [(10,), (N + 1, 10), (N, 4), (N + 1, 3), (4,), (N + 1, 10), (N, 4)]
        tans = [tx0, txr, tur, tf, du0, dX, dU]
        name = "ndp_step_jvp_device"
        if tmodel is not None:
            tans.insert(4, tmodel)                                      # (behind tf)
            tails.insert(4, (16,))
            name = "ndp_step_jvp_model_device"
        # (without the T axis: [B, ...] is [B, 1, ...] as it lies)
        T, shapes = _t_axis_shapes("step_jvp_device", B, [(getattr(t, "shape", None), s, 1) for t, s in zip(tans, tails)])
        d = self._dptr
        X, U, A = tape
        args = [d(x0, torch.float64, (B, 10)), d(xr, torch.float64, (B, N + 1, 10)), d(ur, torch.float64, (B, N, 4)),
                d(f, torch.float32, (B, N + 1, 3)), d(X, torch.float64, (B, N + 1, 10)), d(U, torch.float64, (B, N, 4)),
                d(A, torch.int8, (B, N, 4)), T, *(d(t, torch.float64, s) for t, s in zip(tans, shapes)),
                d(u0_check, torch.float64, (B, 4)), d(status_check, torch.int32, (B,)), self._stream(stream)]
        self._check(getattr(self._lib, name)(self._h, *args), name)

    # ------------------------------------------------------------------ backward pass of the downwash network
    def _other_ptr(self, other, other_index):
        """(pointer, doubles per node) of neighbour windows [rows, N+1, 6 or 10] (rows = B without other_index): a CUDA tensor, or raw
        device memory (dist.DevWindows: e.g. another process's window buffer mapped with ndp_peer_open)."""
        import torch
        raw = hasattr(other, "dev_ptr")
        shape = tuple(other.shape) if raw or isinstance(other, torch.Tensor) else ()
        fits = len(shape) == 3 and shape[1] == self.N + 1 and shape[2] in (6, 10) and (other_index is not None or shape[0] == self.B)
        if raw:
            if not fits:
                raise ValueError("other: expected device windows of shape [rows, N+1, 6 or 10]")
            return C.c_void_p(int(other.dev_ptr)), int(shape[2])
        if not (fits and other.is_cuda and other.is_contiguous() and other.dtype == torch.float64):
            raise ValueError("other: expected a contiguous CUDA float64 [rows, N+1, 6 or 10] tensor")
        return C.c_void_p(other.data_ptr()), int(shape[2])

    def downwash_vjp_device(self, other, ego_ref, gf, ego_xy=None, other_index=None, gz=None, gw=None, stream=None):
        """Enqueues the backward pass of the downwash network and its gate on `stream` (ndp_downwash_vjp_device; include/ndp_nmpc.h):
        other / other_index / ego_ref (= the step's xr) / ego_xy as the step that produced the force took them, gf [B,N+1,3] float64 the
        gradient of that force (step_vjp_device's gf as it lies).  Outputs (CUDA tensors the caller allocates, None = not computed, not
        both None): gz [B,N+1,6] float64 = dL/d(other - ego_ref)[..., 0:6], exactly 0 on closed and neighbour-less instances; gw [17859]
        float32 in blob order, overwritten.  A row whose gf is not finite (an instance whose step failed) adds nothing to gw and has NaN
        in its own gz row.  This is the exact derivative of the fp32 network the step ran, with the gate held fixed.  Two calls with the
        same inputs give bit-identical results; the engine's state is not written.  stream None or torch's default stream: the call goes
        on the engine's own stream behind a wait for torch's (read the outputs after engine.synchronize())."""
        import torch
        B, N = self.B, self.N
        self._torch_default_wait(stream)
        optr, stride = self._other_ptr(other, other_index)
        d = self._dptr
        self._check(self._lib.ndp_downwash_vjp_device(
            self._h, optr, stride, d(other_index, torch.int32, (B,)), d(ego_ref, torch.float64, (B, N + 1, 10)),
            d(ego_xy, torch.float64, (B, 2)), d(gf, torch.float64, (B, N + 1, 3)), d(gz, torch.float64, (B, N + 1, 6)),
            d(gw, torch.float32, (_lib.MLP_NPARAM,)), self._stream(stream)), "ndp_downwash_vjp_device")

    def downwash_jvp_device(self, other, ego_ref, tz=None, tw=None, ego_xy=None, other_index=None, n_tan=None, df=None, f_check=None,
                            stream=None):
        """Enqueues the forward mode of the downwash network and its gate on `stream` (ndp_downwash_jvp_device; include/ndp_nmpc.h):
        other / other_index / ego_ref (= the step's xr) / ego_xy as the step that produced the force took them.  Directions (None = 0, not
        both None): tz [B,T,N+1,6] float64, the direction of (other - ego_ref)[..., 0:6]; tw [T,17859] float32, the direction of the
        weights in blob order.  Outputs (CUDA tensors the caller allocates): df [B,T,N+1,3] float64, required -- the first-order change
        of the force in step_jvp_device's tf layout, exactly 0 on closed and neighbour-less instances; f_check [B,N+1,3] float32, optional
        -- the recomputed force.  T (1..8) is n_tan when given, else read from the tensors; tensors without the T axis mean T = 1.  The
        gate is held fixed.  T directions in one call equal T calls of one bit for bit; the engine's state is not written.  stream None or
        torch's default stream: the call goes on the engine's own stream behind a wait for torch's (read the outputs after
        engine.synchronize())."""
        import torch
        B, N = self.B, self.N
        self._torch_default_wait(stream)
        T, (stz, stw, sdf) = _t_axis_shapes("downwash_jvp_device", B, (
            (getattr(tz, "shape", None), (N + 1, 6), 1), (getattr(tw, "shape", None), (_lib.MLP_NPARAM,), 0), (getattr(df, "shape", None), (N + 1, 3), 1)), n_tan)
        d = self._dptr
        optr, stride = self._other_ptr(other, other_index)
        self._check(self._lib.ndp_downwash_jvp_device(
            self._h, optr, stride, d(other_index, torch.int32, (B,)), d(ego_ref, torch.float64, (B, N + 1, 10)),
            d(ego_xy, torch.float64, (B, 2)), T, d(tz, torch.float64, stz), d(tw, torch.float32, stw), d(df, torch.float64, sdf),
            d(f_check, torch.float32, (B, N + 1, 3)), self._stream(stream)), "ndp_downwash_jvp_device")

    # ---- the same two with K neighbours per instance (the derivatives of downwash_multi_device)
    def downwash_multi_vjp_device(self, other, other_index, ego_ref, gf, ego_xy=None, gz=None, gw=None, stream=None):
        """Enqueues the backward pass of downwash_multi_device on `stream` (ndp_downwash_multi_vjp_device; include/ndp_nmpc.h): other
        [rows,N+1,6 or 10] / other_index int32[B,K] / ego_ref / ego_xy as the forward took them, gf [B,N+1,3] float64 the gradient of the
        SUMMED force (shared by the slots).  Outputs (None = not computed, not both None): gz [B,K,N+1,6] float64 per slot, bit-equal to
        what downwash_vjp_device gives for other_index[:, k] (0 on closed and empty slots); gw [17859] float32, overwritten, the sum over
        all rows and slots in one fixed order.  A row whose gf is not finite adds nothing to gw and has NaN in the gz rows of its open
        slots.  Shares downwash_vjp_device's workspace: order the two against each other.  The engine's state is not written.  stream None
        or torch's default stream: as downwash_vjp_device."""
        import torch
        B, N = self.B, self.N
        self._torch_default_wait(stream)
        optr, stride = self._other_ptr(other, other_index)
        iptr, K = self._dindex_multi(other_index)
        d = self._dptr
        self._check(self._lib.ndp_downwash_multi_vjp_device(
            self._h, optr, stride, iptr, K, d(ego_ref, torch.float64, (B, N + 1, 10)), d(ego_xy, torch.float64, (B, 2)),
            d(gf, torch.float64, (B, N + 1, 3)), d(gz, torch.float64, (B, K, N + 1, 6)), d(gw, torch.float32, (_lib.MLP_NPARAM,)),
            self._stream(stream)), "ndp_downwash_multi_vjp_device")

    def downwash_multi_jvp_device(self, other, other_index, ego_ref, tz=None, tw=None, ego_xy=None, n_tan=None, df=None, f_check=None,
                                  stream=None):
        """Enqueues the forward mode of downwash_multi_device on `stream` (ndp_downwash_multi_jvp_device; include/ndp_nmpc.h).  Directions
        (None = 0, not both None): tz [B,T,K,N+1,6] float64 per slot, tw [T,17859] float32.  Outputs: df [B,T,N+1,3] float64, required --
        the float64 sum in slot order of what downwash_jvp_device gives per slot, exactly 0 where no slot is open; f_check [B,N+1,3]
        float32, optional -- the summed force, bit-equal to downwash_multi_device's.  T (1..8) is n_tan when given, else read from the
        tensors; tensors without the T axis mean T = 1.  No workspace; the engine's state is not written.  stream None or torch's default
        stream: as downwash_jvp_device."""
        import torch
        B, N = self.B, self.N
        self._torch_default_wait(stream)
        optr, stride = self._other_ptr(other, other_index)
        iptr, K = self._dindex_multi(other_index)
        T, (stz, stw, sdf) = _t_axis_shapes("downwash_multi_jvp_device", B, (
            (getattr(tz, "shape", None), (K, N + 1, 6), 1), (getattr(tw, "shape", None), (_lib.MLP_NPARAM,), 0), (getattr(df, "shape", None), (N + 1, 3), 1)), n_tan)
        d = self._dptr
        self._check(self._lib.ndp_downwash_multi_jvp_device(
            self._h, optr, stride, iptr, K, d(ego_ref, torch.float64, (B, N + 1, 10)), d(ego_xy, torch.float64, (B, 2)), T,
            d(tz, torch.float64, stz), d(tw, torch.float32, stw), d(df, torch.float64, sdf), d(f_check, torch.float32, (B, N + 1, 3)),
            self._stream(stream)), "ndp_downwash_multi_jvp_device")

    def set_mlp_weights_device(self, blob, stream=None):
        """set_mlp_weights from a float32 CUDA tensor of 17859 values in blob order, enqueued on `stream` with no host synchronisation
        (ndp_set_mlp_weights_device): steps enqueued behind it on that stream use the new weights."""
        import torch
        self._torch_default_wait(stream)
        self._check(self._lib.ndp_set_mlp_weights_device(self._h, self._dptr(blob, torch.float32, (_lib.MLP_NPARAM,)), self._stream(stream)),
                    "ndp_set_mlp_weights_device")
        self._mlp_installed = None          # (torch_layer._install_weights notes what IT installed, behind this call)

    def debug_mlp_fragments(self):
        """(frag, frag_t): host copies of the network's two device images as uint32 / float32 arrays (ndp_debug_mlp_fragments)."""
        from . import mlp_frag
        fr = np.zeros(mlp_frag.FR_TOTAL, dtype=np.uint32)
        frt = np.zeros(mlp_frag.FRT_TOTAL, dtype=np.float32)
        self._check(self._lib.ndp_debug_mlp_fragments(self._h, _lib.ptr(fr), _lib.ptr(frt)), "ndp_debug_mlp_fragments")
        return fr, frt

    # ---- training the downwash network on the device (csrc/mlp_train.hip)
    def mlp_spectral_norms(self, blob):
        """float64 [4]: the largest singular value of each layer's weight matrix of a host blob (17859 float32 in blob order;
        ndp_mlp_spectral_norms).  Synchronises.  The engine's own weights are not read."""
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        if blob.size != _lib.MLP_NPARAM:
            raise ValueError(f"blob: expected {_lib.MLP_NPARAM} float32 values, got {blob.size}")
        out = np.zeros(4, dtype=np.float64)
        self._check(self._lib.ndp_mlp_spectral_norms(self._h, _lib.ptr(blob), _lib.ptr(out)), "ndp_mlp_spectral_norms")
        return out

    def mlp_spectral_norms_device(self, w, sigma, stream=None):
        """Enqueues the four spectral norms of the float32 CUDA blob `w` [17859] into the float64 CUDA tensor `sigma` [4] on `stream`
        (ndp_mlp_spectral_norms_device): a direct method in fp64, accurate to the order of 1e-14 whatever the gaps between singular values.
        stream None or torch's default stream: as downwash_vjp_device."""
        import torch
        self._torch_default_wait(stream)
        d = self._dptr
        self._check(self._lib.ndp_mlp_spectral_norms_device(self._h, d(w, torch.float32, (_lib.MLP_NPARAM,)), d(sigma, torch.float64, (4,)),
                                                            self._stream(stream)), "ndp_mlp_spectral_norms_device")

    def mlp_adam_sn_device(self, w, g, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, sn=0.0, sigma=None, info=None, install=False,
                           stream=None):
        """Enqueues one optimiser step on `stream` (ndp_mlp_adam_sn_device; include/ndp_nmpc.h): torch.optim.Adam's update (defaults: no
        weight decay, no amsgrad) of the float32 CUDA blob `w` [17859] with the gradient `g` (what downwash_vjp_device writes as gw) and
        the moments `m`, `v` (float32 [17859], in place), then, with sn > 0, every weight matrix whose spectral norm exceeds sn scaled back
        onto it (biases never).  `step` int64 CUDA [1] counts the steps taken and is advanced by the kernel, so calls can be enqueued back
        to back or captured.  A non-finite gradient changes nothing and sets info[0].  sigma float64 [4] (the norms after the call) and
        info int32 [4] (skipped flag, bitmask of scaled layers, 0, 0) are optional.  install: the engine's network becomes the updated `w`
        behind the step (set_mlp_weights_device on the same stream).  Never synchronises the device.  stream None or torch's default
        stream: as downwash_vjp_device."""
        import torch
        self._torch_default_wait(stream)
        d, n = self._dptr, (_lib.MLP_NPARAM,)
        self._check(self._lib.ndp_mlp_adam_sn_device(
            self._h, d(w, torch.float32, n), d(g, torch.float32, n), d(m, torch.float32, n), d(v, torch.float32, n),
            d(step, torch.int64, (1,)), float(lr), float(betas[0]), float(betas[1]), float(eps), float(sn), d(sigma, torch.float64, (4,)),
            d(info, torch.int32, (4,)), int(bool(install)), self._stream(stream)), "ndp_mlp_adam_sn_device")
        if install:
            self._mlp_installed = None      # (torch_layer.DownwashAdamSN notes what IT installed, behind this call)

    # ---- the network on sample rows (ndp_mlp_rows_device, ndp_mlp_fit_rows_device): no window, no gate, any number of rows
    @staticmethod
    def _rows_shape(z, index, f):
        """(R, M) of a row call: z [R,6]; M from index [M], else from f [M,3], else R."""
        R = int(z.shape[0]) if z is not None and z.dim() == 2 else 0
        M = int(index.shape[0]) if index is not None else int(f.shape[0]) if f is not None else R
        return R, M

    def mlp_rows_device(self, z, f, index=None, stream=None):
        """Enqueues the installed network on the float32 CUDA rows z [R,6] on `stream` (ndp_mlp_rows_device; include/ndp_nmpc.h):
        f [M,3] float32, row m from data row index[m] (int32 CUDA [M]; None: row m, M <= R).  An index < 0 or >= R is an empty slot: never
        read, its f row exactly 0.  Each row is bit-equal to downwash_device's for the same six float32 inputs.  The engine's state is
        not written.  stream None or torch's default stream: as downwash_vjp_device."""
        import torch
        self._torch_default_wait(stream)
        R, M = self._rows_shape(z, index, f)
        d = self._dptr
        self._check(self._lib.ndp_mlp_rows_device(self._h, d(z, torch.float32, (R, 6)), d(index, torch.int32, (M,)), R, M,
                                                  d(f, torch.float32, (M, 3)), self._stream(stream)), "ndp_mlp_rows_device")

    def mlp_fit_rows_device(self, z, y, scale, index=None, row_weight=None, groups=0, loss=None, gw=None, f=None, info=None, M=None,
                            stream=None):
        """Enqueues the fused loss and weight gradient of the installed network on sample rows on `stream` (ndp_mlp_fit_rows_device;
        include/ndp_nmpc.h): z [R,6], y [R,3], row_weight [R] (None: 1) float32 CUDA; index int32 CUDA [M] as in mlp_rows_device (None:
        the first M rows; M defaults to R).  Outputs (CUDA tensors the caller allocates, None = not computed, not all of loss, gw, f):
        loss float64 [1] = scale * sum rw |f - y|^2 (scale = 1 / (3 n): nn.MSELoss); gw [17859] float32 in blob order, overwritten;
        f [M,3] float32, the prediction; info int32 [2], rows used and rows skipped (non-finite z, y, rw or prediction).  groups: the
        number of workgroups, 0 = the library's choice, 1.._lib.FIT_MAX_GROUPS forces it (summation order only).  Two calls give
        identical bits.  Its workspace is its own; fit calls on one engine must be ordered against each other.  The engine's state is
        not written.  stream None or torch's default stream: as downwash_vjp_device."""
        import torch
        self._torch_default_wait(stream)
        R, Mi = self._rows_shape(z, index, f)
        M = Mi if M is None else int(M)
        d = self._dptr
        self._check(self._lib.ndp_mlp_fit_rows_device(
            self._h, d(z, torch.float32, (R, 6)), d(y, torch.float32, (R, 3)), d(row_weight, torch.float32, (R,)),
            d(index, torch.int32, (M,)), R, M, float(scale), int(groups), d(loss, torch.float64, (1,)),
            d(gw, torch.float32, (_lib.MLP_NPARAM,)), d(f, torch.float32, (M, 3)), d(info, torch.int32, (2,)), self._stream(stream)),
            "ndp_mlp_fit_rows_device")

    def device_iterate(self):
        """The engine's iterate as CUDA tensor views (no copy): (X [B,N+1,10], U [B,N,4]) float64 (ndp_device_iterate_x / _u); valid once
        the step's stream has reached them; the next step overwrites them."""
        return self._device_views((self._lib.ndp_device_iterate_x, (self.B, self.N + 1, 10)), (self._lib.ndp_device_iterate_u, (self.B, self.N, 4)))

    # ------------------------------------------------------------------ HBM-resident API (torch CUDA tensors)
    @staticmethod
    def _dptr(t, dtype, shape):
        if t is None:
            return None
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == dtype
                and tuple(t.shape) == tuple(shape)):
            raise ValueError(f"expected contiguous CUDA tensor {dtype} {tuple(shape)}")
        return C.c_void_p(t.data_ptr())

    def reset_device(self, xr, ur, stream=None):
        import torch
        self._check(self._lib.ndp_reset_device(self._h, self._dptr(xr, torch.float64, (self.B, self.N + 1, 10)),
                                               self._dptr(ur, torch.float64, (self.B, self.N, 4)),
                                               self._stream(stream)), "ndp_reset_device")

    def update_device(self, x0, xr, ur, u0_out, f=None, other=None, ego_xy=None, stream=None, other_index=None):
        """Enqueues one control step on `stream` (default: the library's stream); no synchronisation.

        other: [B,N+1,10] neighbour windows, or -- with other_index (int32[B]: row of `other` holding instance i's
        neighbour, < 0 = none) -- any [rows,N+1,10] or [rows,N+1,6] buffer, e.g. what an all-gather over the GPUs left."""
        self.bind_update_device(x0, xr, ur, u0_out, f=f, other=other, ego_xy=ego_xy, stream=stream, other_index=other_index)()

    def bind_update_device(self, x0, xr, ur, u0_out, f=None, other=None, ego_xy=None, stream=None, other_index=None):
        """update_device with the argument checks done ONCE: returns a callable that enqueues the step on the same buffers (one
        ctypes call, ~3 us of host time instead of ~13) -- for loops that launch from the host at the control step's own pace.
        The tensors must stay alive and in place for as long as the callable is used."""
        import torch
        B, N = self.B, self.N
        # (rows picked through other_index -- any number of rows -- or row i = instance i of a [B, N+1, 6 or 10] window)
        optr, stride = (None, 10) if other is None else self._other_ptr(other, other_index)
        args = (self._h, self._dptr(x0, torch.float64, (B, 10)), self._dptr(xr, torch.float64, (B, N + 1, 10)),
                self._dptr(ur, torch.float64, (B, N, 4)), self._dptr(f, torch.float32, (B, N + 1, 3)),
                optr, stride, self._dptr(other_index, torch.int32, (B,)), self._dptr(ego_xy, torch.float64, (B, 2)),
                self._dptr(u0_out, torch.float64, (B, 4)), self._stream(stream))
        fn, check = self._lib.ndp_step_device_ex, self._check

        def launch():
            check(fn(*args), "ndp_step_device")
        return launch

    # ------------------------------------------------------------------ downwash one tick ahead (second stream)
    def downwash_prefetch_device(self, other, ego_ref, ego_xy=None, other_index=None, after_stream=None, on_stream=None):
        """Enqueues gate + MLP for the NEXT control step on the engine's second stream (ndp_downwash_prefetch_device): it runs
        beside the control-step kernel of the current tick.  other / other_index as in update_device; ego_ref = that tick's xr."""
        import torch
        B, N = self.B, self.N
        optr, stride = self._other_ptr(other, other_index)
        self._check(self._lib.ndp_downwash_prefetch_device(
            self._h, optr, stride, self._dptr(other_index, torch.int32, (B,)), self._dptr(ego_ref, torch.float64, (B, N + 1, 10)),
            self._dptr(ego_xy, torch.float64, (B, 2)), self._stream(after_stream), self._stream(on_stream)),
            "ndp_downwash_prefetch_device")

    def update_device_prefetched(self, x0, xr, ur, u0_out, stream=None):
        """The control step that consumes the oldest prediction of downwash_prefetch_device (ndp_step_device_prefetched)."""
        import torch
        B, N = self.B, self.N
        self._check(self._lib.ndp_step_device_prefetched(
            self._h, self._dptr(x0, torch.float64, (B, 10)), self._dptr(xr, torch.float64, (B, N + 1, 10)),
            self._dptr(ur, torch.float64, (B, N, 4)), self._dptr(u0_out, torch.float64, (B, 4)), self._stream(stream)),
            "ndp_step_device_prefetched")

    def prefetch_join(self, stream=None):
        self._check(self._lib.ndp_prefetch_join(self._h, self._stream(stream)), "ndp_prefetch_join")

    def prefetch_stats(self):
        out = (C.c_ulonglong * 5)()
        self._check(self._lib.ndp_prefetch_stats(self._h, out), "ndp_prefetch_stats")
        return dict(predictions=int(out[0]), steps=int(out[1]), force_timeouts=int(out[2]), slot_timeouts=int(out[3]),
                    late_waves=int(out[4]))

    def force_slot(self, slot):
        """The force of prediction m (slot m & 1) as a CUDA tensor view [B, N+1, 3] float32 (valid after prefetch_join / stats)."""
        f, = self._device_views((lambda h: self._lib.ndp_device_force_slot(h, int(slot)), (self.B, self.N + 1, 3), "<f4"))
        if f is None:
            raise NdpError("no force slots: downwash_prefetch_device was never called")
        return f

    def device_force(self):
        """The force the fused downwash (or ndp_downwash_device) of the last step left in HBM: CUDA tensor view [B, N+1, 3] float32
        (ndp_device_force); valid once the step's stream has reached it."""
        return self._device_views((self._lib.ndp_device_force, (self.B, self.N + 1, 3), "<f4"))[0]

    def track_steps(self, on=True):
        """Every control step launched from now on marks an event at its completion without a packet of its own (ndp_track_steps)."""
        self._check(self._lib.ndp_track_steps(self._h, 1 if on else 0), "ndp_track_steps")

    def last_step_event(self):
        """The raw HIP event (ctypes.c_void_p) of the control step launched last (track_steps first)."""
        ev = C.c_void_p()
        self._check(self._lib.ndp_last_step_event(self._h, C.byref(ev)), "ndp_last_step_event")
        return ev

    @property
    def refine_active(self):
        """True when cfg.ipm_refine acts on this engine's control steps (three-slot kernels, N <= 27); the five-slot kernels and the
        late-force step ignore it (include/ndp_nmpc.h: ndp_cfg.ipm_refine)."""
        return self._lib.ndp_refine_active(self._h) == 1

    @property
    def work_queue(self):
        """True when this engine's steps send interior-point solves through the in-kernel work queue (cfg.work_queue)."""
        return self._lib.ndp_work_queue_enabled(self._h) == 1

    def downwash_device(self, other, ego_ref, f_out, ego_xy=None, stream=None):
        import torch
        B, N = self.B, self.N
        self._check(self._lib.ndp_downwash_device(
            self._h, self._dptr(other, torch.float64, (B, N + 1, 10)), self._dptr(ego_ref, torch.float64, (B, N + 1, 10)),
            self._dptr(ego_xy, torch.float64, (B, 2)), self._dptr(f_out, torch.float32, (B, N + 1, 3)),
            self._stream(stream)), "ndp_downwash_device")

    @staticmethod
    def _stream(stream):
        if stream is None:
            return None
        return C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))

    def synchronize(self):
        self._check(self._lib.ndp_synchronize(self._h), "ndp_synchronize")

    def debug_rti_launched(self):
        """(names, waves, fusable): the rows of the control-step kernel table (csrc/rti_table.hpp: enum RtiId) this handle launched since
        the last call (ndp_debug_rti_launched; reading clears them), its instances per workgroup, and whether the downwash network can
        run inside the control step's launch."""
        mask, out = C.c_uint64(0), np.zeros(3, dtype=np.int32)
        self._check(self._lib.ndp_debug_rti_launched(self._h, C.byref(mask), _lib.ptr(out)), "ndp_debug_rti_launched")
        names = _lib.rti_kernel_names()
        if len(names) != out[0]:
            raise NdpError(f"the library has {out[0]} control-step kernels, enum RtiId names {len(names)}")
        return {n for i, n in enumerate(names) if mask.value >> i & 1}, int(out[1]), bool(out[2])

    def debug_stamps(self, enable=True, read=False):
        """Whole-batch phase stamps (profiling hook): returns [B,24] of the last step when read=True."""
        out = np.zeros((self.B, 24)) if read else None
        self._check(self._lib.ndp_debug_stamps(self._h, int(bool(enable)), _lib.ptr(out)), "ndp_debug_stamps")
        return out

    def timing_enable(self, every=1):
        """Bracket every `every`-th launch of each kernel with HIP events (0 / False: off)."""
        self._check(self._lib.ndp_timing_enable(self._h, int(every)), "ndp_timing_enable")

    def timing_read(self, name):
        tot, n = C.c_double(0.0), C.c_int64(0)
        rc = self._lib.ndp_timing_read(self._h, name.encode(), C.byref(tot), C.byref(n))
        if rc < 0:
            return 0.0, 0
        return tot.value, n.value
