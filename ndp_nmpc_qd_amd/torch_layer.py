"""The batched control step as a differentiable torch layer: u0 = step(x0, xr, ur, f), backward grad_x0 = K0' grad_u0 and, with
parameter sensitivities on, grad_xr / grad_ur / grad_f.

K0 = du0/dx0 is the initial-state sensitivity the step writes beside u0 (BatchedNMPC.enable_sensitivity, ndp_sens_enable): the
derivative of the QP the step solved, with its active set held fixed (exact: the solution is piecewise affine in x0) or, when the
interior-point loop finished it, of its last Newton system.  With BatchedNMPC.enable_param_sensitivity (ndp_sens_params_enable) the
step also writes du0/dxr, du0/dur and du0/df of the same QP -- linearisation point, x0 and active set held fixed -- and xr, ur and f may
require grad: their gradients are einsum('bi,bi...->b...', grad_u0, du0_d.), in each input's dtype (f: float32).  Without them the
layer raises if xr, ur or f requires grad (a silent zero gradient would be wrong, not approximate).  The linearisation point is a
constant, and so are the fused downwash network's inputs (other, ego_xy): the layer raises if they require grad.  Instances with a
nonzero status have NaN in every sensitivity and therefore in their gradients.

Every forward call IS a control step of the engine: it advances the engine's iterate and kept active sets (its warm start), exactly
as BatchedNMPC.update_device does.  Two forward calls on the same x0 therefore need not return the same u0.

control_step_trajectory (ControlStepTrajectoryFunction) returns the whole new iterate as well -- (u0, X, U), the predicted trajectory --
and differentiates all three by the adjoint (reverse mode): the forward step records a small tape (the iterate and kept sets it started
from, BatchedNMPC.record_tape) and runs unchanged; the backward recomputes the step from the tape and solves one adjoint system of its QP
with the upstream gradients (BatchedNMPC.step_vjp_device).  Same derivative as above; no sensitivities need to be on.

downwash / control_step_ndp / NDPControlStep (at the end of this file) continue that adjoint through the downwash network: gradients of the
neighbour windows and of the network's weights (BatchedNMPC.downwash_vjp_device).  The entry points above keep refusing other / ego_xy.

control_step_jvp is the forward-mode counterpart (BatchedNMPC.step_jvp_device): the step, then the first-order change of (u0, X, U) along
given directions of x0, xr, ur and f.  It returns plain tensors; there is no autograd hookup.

downwash_jvp / control_step_ndp_jvp continue that forward mode through the downwash network (BatchedNMPC.downwash_jvp_device): the force's tangent
is the network's, along directions of the neighbour windows, of xr and of the weights.  Plain tensors as well.

downwash_multi / control_step_ndp_multi / NDPControlStepMulti and downwash_multi_jvp / control_step_ndp_multi_jvp (behind their
single-neighbour siblings) are the same four with K neighbours per instance, other_index [B,K]: the summed prediction
(BatchedNMPC.downwash_multi_device) into the external-force step, differentiated by BatchedNMPC.downwash_multi_vjp_device /
downwash_multi_jvp_device.

DownwashAdamSN (at the end of this file) is the optimiser those weight gradients were built for: the reference's full-batch Adam and
spectral-norm cap as one launch per step (BatchedNMPC.mlp_adam_sn_device).

downwash_rows / downwash_fit_rows (behind it) are the network on plain sample rows [R,6] float32, the form the reference trains and
evaluates on: the forward without autograd, and the weighted MSE whose forward is ONE fused call that also leaves the weight gradient
(BatchedNMPC.mlp_rows_device / mlp_fit_rows_device); mini-batches are index lists into a resident data set.

control_step_tunable / TunableControlStep (behind them) differentiate the controller's own numbers -- the cost weights Qd, Rd and the mass --
by the same adjoint (BatchedNMPC.set_model, step_vjp_device with gmodel).

plant_rollout / plant_step / plant_rollout_jvp (at the end of this file) are the plant: the rigid body over a given sequence of inputs and
forces in one launch, differentiable in the initial state, the inputs and the forces (BatchedNMPC.plant_rollout_device,
plant_rollout_vjp_device, plant_rollout_jvp_device).  plant_step is its one-tick case, the piece that chains with the control_step*
Functions: u0 -> plant_step -> the next tick's x0, with the values ndp_plant_step_device gives bit for bit.

closed_loop (behind plant_rollout_jvp) is the whole closed loop over given windows as ONE autograd Function: control step -> plant tick -> the
next tick's x0, `ticks` times in one call (BatchedNMPC.closed_loop_device), and one call back (closed_loop_vjp_device) for the gradients of
x_0, the windows, both forces, Qd, Rd and the mass -- what the chain control_step_trajectory -> plant_step gives link by link.
closed_loop_jvp (behind it) is the same flight with its forward mode: that one call forward with a tape, then one call
(closed_loop_jvp_device) for the tangents of x_{k+1}, u0_k and X_k along T directions of x_0, the windows and both forces -- what the chain
control_step_jvp -> plant_rollout_jvp(ticks = 1) gives tick by tick.  No autograd hookup.
closed_loop_formation (at the end of this file) is closed_loop for a formation: the force on the plant is made inside the loop from the
vehicles' actual states (plant_force's values at every tick), and the one call back (closed_loop_formation_vjp_device) carries the gradients
across the vehicles on the device and returns the network's weight gradient summed over the ticks -- what the chain plant_force ->
control_step_trajectory -> plant_step gives link by link.

plant_force / plant_force_jvp (at the end of this file) are the downwash force the neighbours' actual states put on the plant, differentiable
in the states and the network's weights (BatchedNMPC.plant_force_multi_device, plant_force_multi_vjp_device, plant_force_multi_jvp_device):
f = plant_force(engine, x, other_index); x = plant_step(engine, x, u, f) is a differentiable formation tick on the plant side.
"""
import torch

from . import _lib
from .params import nmpc_params as CP

_WHY_GATE = "the r_horiz gate is piecewise constant and is not differentiated (detach it)"
_WHY_NETWORK = "the fused downwash network is not differentiated (detach it, or leave it out of the graph)"


def _det(t):
    return t.detach().contiguous() if isinstance(t, torch.Tensor) else t


def _cast(t, dtype):
    return None if t is None else t.to(dtype).contiguous()


def _refuse_grad(who, name, t, why):
    """A silent zero gradient would be wrong, not approximate: e.g. "DownwashFunction: ego_xy requires grad, but the r_horiz gate is
    piecewise constant and is not differentiated (detach it)"."""
    if isinstance(t, torch.Tensor) and t.requires_grad:
        raise ValueError(f"{who}: {name} requires grad, but {why}")


def _cuda_stream(t):
    """(stream, is torch's default stream) for a tensor's device; (None, False) for CPU tensors (stub engines in the tests)."""
    if not t.is_cuda:
        return None, False
    s = torch.cuda.current_stream(t.device)
    return s, s.cuda_stream == 0


def _enter(engine, t, weights=None):
    """The prologue of an entry point whose call goes on t's current stream: (stream, default, key).  torch's default stream cannot be
    named through the C-ABI (a NULL stream is the engine's own): there the call runs on the engine's stream, so the inputs are waited for
    in front of it (here) and the caller waits for the engine behind it.  `weights`, when given, are installed first (_install_weights,
    whose key this returns)."""
    stream, default = _cuda_stream(t)
    if default:
        stream.synchronize()
    return stream, default, _install_weights(engine, weights, stream)


def _taped_step(engine, stream, default, x0, xr, ur, **kw):
    """The forward of the adjoint Functions: the tape of the step about to run, the step (update_device with kw) on `stream`, and clones of
    the new iterate ordered behind it (the next step overwrites it).  Returns (tape, u0, X, U)."""
    tape = engine.record_tape(stream)
    u0 = torch.empty((x0.shape[0], 4), dtype=x0.dtype, device=x0.device)
    engine.update_device(x0, xr, ur, u0, stream=stream, **kw)
    if default:                            # torch's default stream: the step went on the engine's own (the C-ABI's NULL)
        engine.synchronize()
    X, U = (t.clone() for t in engine.device_iterate())
    return tape, u0, X, U


def _taped_step_vjp(engine, x0, xr, ur, tape, force, upstream, need, stream, **kw):
    """The backward of the adjoint Functions: step_vjp_device (with kw) for the float64 casts of upstream = (g_u0, g_X, g_U) into newly
    allocated outputs.  need: which of (gx0, gxr, gur, gf) to compute; returns those four, None where not needed.  No synchronisation."""
    B, N = x0.shape[0], xr.shape[1] - 1
    gu0, gX, gU = (None if g is None else g.to(torch.float64).contiguous() for g in upstream)
    gx0, gxr, gur, gf = (torch.empty(*s, dtype=torch.float64, device=x0.device) if n else None
                         for n, s in zip(need, ((B, 10), (B, N + 1, 10), (B, N, 4), (B, N + 1, 3))))
    engine.step_vjp_device(x0, xr, ur, tape, gu0=gu0, gX=gX, gU=gU, f=force, gx0=gx0, gxr=gxr, gur=gur, gf=gf, stream=stream, **kw)
    return gx0, gxr, gur, gf


class ControlStepFunction(torch.autograd.Function):
    """forward(x0, engine, xr, ur, f, other, ego_xy) -> u0 [B,4] float64; backward: grad_x0 = K0' grad_u0 and, when the engine has parameter
    sensitivities on, the gradients of xr, ur and f (batched contractions on x0's device).  x0, xr, ur (and f / other / ego_xy when given)
    are contiguous CUDA tensors as update_device takes them."""

    @staticmethod
    def forward(ctx, x0, engine, xr, ur, f=None, other=None, ego_xy=None):
        params = bool(getattr(engine, "param_sensitivity_enabled", False))
        if not params:
            for name, t in (("xr", xr), ("ur", ur), ("f", f)):
                _refuse_grad("ControlStepFunction", name, t, "the engine's parameter sensitivities are off (engine.enable_param_sensitivity() "
                             "or ControlStep(engine, params=True)) (detach it, or leave it out of the graph)")
        for name, t in (("other", other), ("ego_xy", ego_xy)):
            _refuse_grad("ControlStepFunction", name, t, _WHY_NETWORK)
        if engine.sensitivity_level < 1:
            raise ValueError("ControlStepFunction: the engine's sensitivities are off (engine.enable_sensitivity(1) first)")
        x0 = x0.detach().contiguous()
        xr_d, ur_d, f_d = (t.detach() if isinstance(t, torch.Tensor) else t for t in (xr, ur, f))
        u0 = torch.empty((x0.shape[0], 4), dtype=x0.dtype, device=x0.device)
        stream, default, _ = _enter(engine, x0)
        engine.update_device(x0, xr_d, ur_d, u0, f=f_d, other=other, ego_xy=ego_xy, stream=stream)
        if default:
            engine.synchronize()
        # (copies ordered behind the step on the same stream: the engine's buffers are overwritten by its next step)
        K0 = engine.device_sensitivity()[0].clone()
        ctx.params = params
        ctx.dtypes = tuple(t.dtype if isinstance(t, torch.Tensor) else None for t in (xr, ur, f))
        if params:
            ctx.save_for_backward(K0, *(d.clone() for d in engine.device_param_sensitivity()))
        else:
            ctx.save_for_backward(K0)
        return u0

    @staticmethod
    def backward(ctx, grad_u0):
        K0 = ctx.saved_tensors[0]
        g = grad_u0.to(K0.dtype)
        grad_x0 = torch.bmm(K0.transpose(1, 2), g.unsqueeze(2)).squeeze(2)
        grads = [None, None, None]
        if ctx.params:
            for n, (J, dt) in enumerate(zip(ctx.saved_tensors[1:], ctx.dtypes)):
                if ctx.needs_input_grad[2 + n] and dt is not None:
                    grads[n] = torch.einsum("bi,bi...->b...", g, J).to(dt)
        return (grad_x0, None, *grads, None, None)


def control_step(engine, x0, xr, ur, f=None, other=None, ego_xy=None):
    """u0 = the engine's control step at x0, differentiable with respect to x0 and, with the engine's parameter sensitivities on, xr, ur
    and f (see ControlStepFunction)."""
    return ControlStepFunction.apply(x0, engine, xr, ur, f, other, ego_xy)


class ControlStepTrajectoryFunction(torch.autograd.Function):
    """forward(x0, engine, xr, ur, f, other, ego_xy) -> (u0 [B,4], X [B,N+1,10], U [B,N,4]) float64, the step's control and new iterate;
    backward: the adjoint of the step (BatchedNMPC.step_vjp_device) for the gradients of x0, xr, ur and f (f: float32, as given).  With
    neighbour windows the force is the fused network's output (its inputs are not differentiated: the layer raises if they require grad)."""

    @staticmethod
    def forward(ctx, x0, engine, xr, ur, f=None, other=None, ego_xy=None):
        for name, t in (("other", other), ("ego_xy", ego_xy)):
            _refuse_grad("ControlStepTrajectoryFunction", name, t, _WHY_NETWORK)
        x0, xr, ur, fd = _det(x0), _det(xr), _det(ur), _det(f)
        tape, u0, X, U = _taped_step(engine, *_cuda_stream(x0), x0, xr, ur, f=fd, other=other, ego_xy=ego_xy)
        force = engine.device_force().clone() if other is not None else fd
        ctx.engine = engine
        ctx.f_dtype = f.dtype if isinstance(f, torch.Tensor) else None
        ctx.save_for_backward(x0, xr, ur, force, *tape)
        return u0, X, U

    @staticmethod
    def backward(ctx, g_u0, g_X, g_U):
        x0, xr, ur, force, *tape = ctx.saved_tensors
        eng = ctx.engine
        if g_u0 is None and g_X is None and g_U is None:
            return (None,) * 7
        need = ctx.needs_input_grad
        stream, default = _cuda_stream(x0)
        gx0, gxr, gur, gf = _taped_step_vjp(eng, x0, xr, ur, tape, force, (g_u0, g_X, g_U),
                                            (need[0], need[2], need[3], need[4] and ctx.f_dtype is not None), stream)
        if default:
            eng.synchronize()
        return (gx0, None, gxr, gur, None if gf is None else gf.to(ctx.f_dtype), None, None)


def control_step_trajectory(engine, x0, xr, ur, f=None, other=None, ego_xy=None):
    """(u0, X, U) = the engine's control step at x0 and its new iterate (the predicted trajectory), differentiable with respect to x0, xr,
    ur and f through the adjoint of the step (see ControlStepTrajectoryFunction); needs no sensitivities on."""
    return ControlStepTrajectoryFunction.apply(x0, engine, xr, ur, f, other, ego_xy)


def model_tangent(tQd=None, tRd=None, tmass=None):
    """A direction of the model as the forward-mode calls take it (tmodel): [..., 16] float64 = tQd [..., 10] | tRd [..., 4] | tmass [...]
    twice -- column 14 is the controller's mass, column 15 the plant's, and an engine has one mass, so its direction goes into both.
    Each part may be None (= 0, not all three); the leading dimensions ([], [T] or [B,T]) must agree."""
    parts = [None if t is None else torch.as_tensor(t).detach().to(torch.float64) for t in (tQd, tRd, tmass)]
    leads = {tuple(p.shape[:-1]) if n else tuple(p.shape) for p, n in zip(parts, (10, 4, 0)) if p is not None}
    if len(leads) != 1:
        raise ValueError("model_tangent: " + ("no part given (tQd, tRd and tmass all None)" if not leads else
                                              f"the parts disagree on the leading dimensions ({sorted(leads)})"))
    first = next(p for p in parts if p is not None)
    out = torch.zeros(leads.pop() + (16,), dtype=torch.float64, device=first.device)
    if parts[0] is not None:
        out[..., 0:10] = parts[0]
    if parts[1] is not None:
        out[..., 10:14] = parts[1]
    if parts[2] is not None:
        out[..., 14] = parts[2]
        out[..., 15] = parts[2]
    return out


def _model_direction(who, tmodel, B, T, device):
    """tmodel [16], [T,16] or [B,T,16] as the contiguous float64 [B,T,16] the device calls take (T None: read from tmodel, 1 for [16]).
    Returns (tensor, whether it came with the T axis)."""
    tm = torch.as_tensor(tmodel).detach().to(device=device, dtype=torch.float64)
    if tm.dim() not in (1, 2, 3) or tm.shape[-1] != 16 or (tm.dim() == 3 and tm.shape[0] != B):
        raise ValueError(f"{who}: tmodel must be [16], [T,16] or [B,T,16], got {tuple(tm.shape)}")
    had = tm.dim() > 1
    Tm = int(tm.shape[-2]) if had else (1 if T is None else T)
    if T is not None and Tm != T:
        raise ValueError(f"{who}: tmodel has {Tm} directions, the other tangents {T}")
    return tm.expand(B, Tm, 16).contiguous(), had


def control_step_jvp(engine, x0, xr, ur, tangents, f=None, tmodel=None):
    """(u0, X, U, du0, dX, dU): the engine's control step at x0 with its new iterate, and the first-order change of all three along the
    directions tangents = (tx0, txr, tur, tf) (forward mode: BatchedNMPC.step_jvp_device; float64 CUDA tensors [B,T,...] or, for one
    direction, [B,...]; None = 0).  The tape is recorded, the ordinary step runs, then the derivative on the same stream.  The outputs carry
    the tangents' T axis: a tangent without it gives du0 [B,4], dX [B,N+1,10], dU [B,N,4].  No autograd hookup: nothing here is recorded in
    a graph.
    tmodel ([16], [T,16] or [B,T,16]; model_tangent builds one): the direction of the cost weights and the mass, added to the data's
    (ndp_step_jvp_model_device); with it `tangents` may be all None, and [16] counts as a direction without the T axis."""
    x0, xr, ur, fd = _det(x0), _det(xr), _det(ur), _det(f)
    tans = [None if t is None else _det(t).to(torch.float64) for t in tangents]
    given = [(t, n) for t, n in zip(tans, (2, 3, 3, 3)) if t is not None]
    if not given and tmodel is None:
        raise ValueError("control_step_jvp: no tangent (tx0, txr, tur and tf all None)")
    B, N = x0.shape[0], xr.shape[1] - 1
    lead = (B,) + tuple({int(t.shape[1]) for t, n in given if t.dim() == n + 1})[:1]
    tm = None
    if tmodel is not None:
        # every tensor of this call gets the T axis; the outputs lose it again if no direction came with it
        tm, had = _model_direction("control_step_jvp", tmodel, B, lead[1] if len(lead) > 1 else (1 if given else None), x0.device)
        tans = [None if t is None else (t.unsqueeze(1) if t.dim() == n else t).contiguous() for t, n in zip(tans, (2, 3, 3, 3))]
        squeeze, lead = len(lead) == 1 and not had, (B, int(tm.shape[1]))
    stream, default = _cuda_stream(x0)
    tape, u0, X, U = _taped_step(engine, stream, default, x0, xr, ur, f=fd)
    du0, dX, dU = (torch.empty(lead + s, dtype=torch.float64, device=x0.device) for s in ((4,), (N + 1, 10), (N, 4)))
    if tm is None:
        engine.step_jvp_device(x0, xr, ur, tape, *tans, f=fd, du0=du0, dX=dX, dU=dU, stream=stream)
    else:
        engine.step_jvp_device(x0, xr, ur, tape, *tans, f=fd, du0=du0, dX=dX, dU=dU, stream=stream, tmodel=tm)
    if default:
        engine.synchronize()
    if tm is not None and squeeze:
        du0, dX, dU = du0[:, 0], dX[:, 0], dU[:, 0]
    return u0, X, U, du0, dX, dU


class ControlStep(torch.nn.Module):
    """A thin module around control_step: holds the engine (a BatchedNMPC) and switches its sensitivities on (level 1) if they are
    off; params=True also switches its parameter sensitivities on, so that xr, ur and f may require grad.
    forward(x0, xr, ur, f=None, other=None, ego_xy=None) -> u0.  Each call advances the engine's warm start.
    backward="adjoint": u0 of control_step_trajectory instead -- the gradients of x0, xr, ur and f by the adjoint, no sensitivities
    switched on (params is then not needed)."""

    def __init__(self, engine, params=False, backward="sensitivity"):
        super().__init__()
        if backward not in ("sensitivity", "adjoint"):
            raise ValueError("ControlStep: backward must be 'sensitivity' or 'adjoint'")
        self.engine = engine
        self.backward = backward
        if backward == "adjoint":
            return
        if engine.sensitivity_level < 1:
            engine.enable_sensitivity(1)
        if params and not engine.param_sensitivity_enabled:
            engine.enable_param_sensitivity(True)

    def forward(self, x0, xr, ur, f=None, other=None, ego_xy=None):
        if self.backward == "adjoint":
            return control_step_trajectory(self.engine, x0, xr, ur, f=f, other=other, ego_xy=ego_xy)[0]
        return control_step(self.engine, x0, xr, ur, f=f, other=other, ego_xy=ego_xy)


# ---------------------------------------------------------------------------------------------- the downwash network, differentiated
# What is differentiated: the fp32 network the step ran (its own ReLU masks) with respect to its input rows (other - ego_ref)[..., 0:6] and its
# 17 859 weights (BatchedNMPC.downwash_vjp_device).  What is held fixed: the r_horiz gate (piecewise constant: ego_xy may not require grad)
# and, in control_step_ndp, everything the step's adjoint holds fixed -- linearisation point and active set.

def _install_weights(engine, weights, stream):
    """Installs `weights` (float32 CUDA tensor / nn.Parameter of 17 859 in blob order) as the engine's network unless they are the ones
    installed last (same storage, same version counter).  Returns the key that identifies what is installed.  The engine keeps a
    reference to the installed tensor, so its storage cannot be freed and handed to another tensor that would then pass for it; any other
    way of setting the engine's weights (set_mlp_weights, set_mlp_weights_device) forgets the key."""
    if weights is None:
        return None
    key = (weights.data_ptr(), weights._version)
    if getattr(engine, "_mlp_installed", None) != key:
        engine.set_mlp_weights_device(weights.detach(), stream=stream)
        engine._mlp_installed, engine._mlp_installed_tensor = key, weights
    return key


def _check_installed(engine, key, who):
    if key is not None and getattr(engine, "_mlp_installed", None) != key:
        raise RuntimeError(f"{who}: the engine's network weights were replaced between this forward and its backward (the backward "
                           "recomputes the forward from the installed weights): run the backward before the next forward with other weights")


def _scatter_gz(gz, other, other_index):
    """dL/d other from g_z [B,N+1,6]: columns 0..5, the rest 0; with other_index, instances that share a neighbour row add up."""
    g = torch.zeros_like(other)
    if other_index is None:
        g[:, :, :6] = gz
    else:
        has = other_index >= 0
        g[:, :, :6].index_add_(0, other_index[has].long(), gz[has])
    return g


def _minus_gz(gz, like):
    g = torch.zeros_like(like)
    g[:, :, :6] = -gz
    return g


# What differs between an entry point with one neighbour per instance (other_index None or [B]) and its K-slot sibling (other_index
# [B,K]) is held by a form: the engine's backward and forward-mode methods, the slot axis of gz / tz, the plumbing between those and the
# windows, and the forward itself.  Every shared body below is written once against a form.

def _force_single(engine, od, other_index, ed, ego_xy, stream, default):
    """The stand-alone single-neighbour forward: downwash_device takes dense [B,N+1,10] windows, so rows are gathered (plumbing) and
    neighbour-less instances zeroed behind it."""
    B, np1 = ed.shape[0], ed.shape[1]
    dense = od
    if other_index is not None or od.shape[2] != 10:
        rows = od if other_index is None else od[other_index.clamp(min=0).long()]
        dense = torch.zeros((B, np1, 10), dtype=od.dtype, device=od.device)
        dense[:, :, :od.shape[2]] = rows
    f = torch.empty((B, np1, 3), dtype=torch.float32, device=od.device)
    engine.downwash_device(dense, ed, f, ego_xy=ego_xy, stream=stream)
    if default:
        engine.synchronize()
    if other_index is not None:
        f[other_index < 0] = 0.0                              # no neighbour: no force
    return f


def _force_multi(engine, od, other_index, ed, ego_xy, stream, default):
    f = torch.empty((ed.shape[0], ed.shape[1], 3), dtype=torch.float32, device=od.device)
    engine.downwash_multi_device(od, other_index, ed, f, ego_xy=ego_xy, stream=stream)
    if default:
        engine.synchronize()
    return f


def _step_single(engine, stream, default, x0, xr, ur, od, other_index, ego_xy):
    """(tape, u0, X, U, force): the fused step (one launch); the force is the engine's buffer, which its next step overwrites."""
    return (*_taped_step(engine, stream, default, x0, xr, ur, other=od, ego_xy=ego_xy, other_index=other_index), engine.device_force())


def _step_multi(engine, stream, default, x0, xr, ur, od, other_index, ego_xy):
    """(tape, u0, X, U, force): the summed prediction into a force tensor of its own, then the external-force step."""
    force = _force_multi(engine, od, other_index, xr, ego_xy, stream, False)
    return (*_taped_step(engine, stream, default, x0, xr, ur, f=force), force)


class _Form:
    def __init__(self, vjp, jvp, slots, fold, scatter, network_tz, force, step, own_force):
        self.vjp, self.jvp = vjp, jvp                # (engine, other, other_index, ego_ref[, gf], **kw): the engine's backward pass / forward mode
        self.slots = slots                           # other_index -> the slot axis of gz [B,*slots,N+1,6] and tz [B,T,*slots,N+1,6]
        self.fold = fold                             # gz -> [B,N+1,6], ego_ref's share (negated by _minus_gz)
        self.scatter = scatter                       # (gz, other, other_index) -> dL/d other
        self.network_tz = network_tz                 # (t_other, t_ego, other_index) -> tz
        self.force, self.step = force, step          # the stand-alone forward and the control step
        self.own_force = own_force                   # the step's force is a tensor of the caller's (else the engine's buffer: clone to keep)


def _scatter_gz_multi(gz, other, other_index):
    """dL/d other from g_z [B,K,N+1,6]: columns 0..5, the rest 0; instances and slots that share a neighbour row add up."""
    g = torch.zeros_like(other)
    has = other_index >= 0
    g[:, :, :6].index_add_(0, other_index[has].long(), gz[has])
    return g


def _with_t_axis(tangents, dims, who):
    """The tangents (None, or tensors whose T axis -- position 0 for the weights' direction (dims 1), 1 for the others -- may be missing)
    as detached contiguous tensors that all have it.  Returns (list, T, whether any tangent came with the axis)."""
    out, Ts, had = [], set(), False
    for t, n in zip(tangents, dims):
        if t is None:
            out.append(None)
            continue
        t = t.detach()
        if t.dim() == n:
            t = t.unsqueeze(0 if n == 1 else 1)
        elif t.dim() == n + 1:
            had = True
        else:
            raise ValueError(f"{who}: a tangent has {t.dim()} dimensions, expected {n} or {n + 1}")
        Ts.add(int(t.shape[0 if n == 1 else 1]))
        out.append(t)
    if not Ts:
        raise ValueError(f"{who}: no tangent (all None)")
    if len(Ts) > 1:
        raise ValueError(f"{who}: the tangents disagree on the number of directions ({sorted(Ts)})")
    return out, Ts.pop(), had


def _network_tz(t_other, t_ego, other_index):
    """tz [B,T,N+1,6] = t_other[other_index] - t_ego on columns 0..5 (either may be None; both None: None): the direction of the
    network's input rows.  Plumbing, the mirror of _scatter_gz / _minus_gz."""
    tz = None
    if t_other is not None:
        rows = t_other if other_index is None else t_other[other_index.clamp(min=0).long()]
        tz = rows[..., :6].to(torch.float64)
    if t_ego is not None:
        e = t_ego[..., :6].to(torch.float64)
        tz = -e if tz is None else tz - e
    return None if tz is None else tz.contiguous()


def _network_tz_multi(t_other, t_ego, other_index):
    """tz [B,T,K,N+1,6] = t_other[other_index[:, k]] - t_ego on columns 0..5 per slot (either may be None; both None: None).  Plumbing, the
    mirror of _scatter_gz_multi; an empty slot's rows are never read by the device."""
    tz = None
    if t_other is not None:
        rows = t_other[other_index.clamp(min=0).long()]                   # [B,K,T,N+1,cols]
        tz = rows[..., :6].to(torch.float64).transpose(1, 2)
    if t_ego is not None:
        e = t_ego[..., :6].to(torch.float64).unsqueeze(2)                 # [B,T,1,N+1,6]
        tz = (-e).expand(-1, -1, other_index.shape[1], -1, -1) if tz is None else tz - e
    return None if tz is None else tz.contiguous()


_SINGLE = _Form(
    vjp=lambda eng, other, other_index, ego_ref, gf, **kw: eng.downwash_vjp_device(other, ego_ref, gf, other_index=other_index, **kw),
    jvp=lambda eng, other, other_index, ego_ref, **kw: eng.downwash_jvp_device(other, ego_ref, other_index=other_index, **kw),
    slots=lambda other_index: (), fold=lambda gz: gz, scatter=_scatter_gz, network_tz=_network_tz,
    force=_force_single, step=_step_single, own_force=False)
_MULTI = _Form(
    vjp=lambda eng, other, other_index, ego_ref, gf, **kw: eng.downwash_multi_vjp_device(other, other_index, ego_ref, gf, **kw),
    jvp=lambda eng, other, other_index, ego_ref, **kw: eng.downwash_multi_jvp_device(other, other_index, ego_ref, **kw),
    slots=lambda other_index: (other_index.shape[1],), fold=lambda gz: gz.sum(dim=1), scatter=_scatter_gz_multi, network_tz=_network_tz_multi,
    force=_force_multi, step=_step_multi, own_force=True)


def _save_network(ctx, engine, key, weights, tensors, ego_xy, other_index):
    ctx.engine, ctx.key, ctx.have_w = engine, key, weights is not None
    ctx.opt = (ego_xy is not None, other_index is not None)
    ctx.save_for_backward(*tensors, *(t for t in (ego_xy, other_index, weights) if t is not None))


def _saved_network(ctx, n):
    """(the first n saved tensors, ego_xy, other_index) of _save_network."""
    rest = list(ctx.saved_tensors[n:])
    ego_xy = rest.pop(0) if ctx.opt[0] else None
    return ctx.saved_tensors[:n], ego_xy, rest.pop(0) if ctx.opt[1] else None


def _downwash_forward(ctx, form, who, other, engine, ego_ref, ego_xy, weights, other_index):
    _refuse_grad(who, "ego_xy", ego_xy, _WHY_GATE)
    od, ed = other.detach().contiguous(), ego_ref.detach().contiguous()
    stream, default, key = _enter(engine, od, weights)
    f = form.force(engine, od, other_index, ed, ego_xy, stream, default)
    _save_network(ctx, engine, key, weights, (od, ed), ego_xy, other_index)
    return f


def _downwash_backward(ctx, form, who, g_f, need):
    """need: which of (other, ego_ref, weights) require a gradient; returns those three."""
    (od, ed), ego_xy, other_index = _saved_network(ctx, 2)
    eng = ctx.engine
    _check_installed(eng, ctx.key, who)
    gf = g_f.to(torch.float64).contiguous()
    B, np1 = ed.shape[0], ed.shape[1]
    gz = torch.empty((B, *form.slots(other_index), np1, 6), dtype=torch.float64, device=od.device) if need[0] or need[1] else None
    gw = torch.empty(_lib.MLP_NPARAM, dtype=torch.float32, device=od.device) if ctx.have_w and need[2] else None
    if gz is None and gw is None:
        return None, None, None
    stream, default = _cuda_stream(od)
    form.vjp(eng, od, other_index, ed, gf, ego_xy=ego_xy, gz=gz, gw=gw, stream=stream)
    if default:
        eng.synchronize()
    return form.scatter(gz, od, other_index) if need[0] else None, _minus_gz(form.fold(gz), ed) if need[1] else None, gw


def _ndp_step_forward(ctx, form, who, x0, engine, xr, ur, other, ego_xy, weights, other_index):
    _refuse_grad(who, "ego_xy", ego_xy, _WHY_GATE)
    x0, xr, ur, od = _det(x0), _det(xr), _det(ur), _det(other)
    stream, default, key = _enter(engine, x0, weights)
    tape, u0, X, U, force = form.step(engine, stream, default, x0, xr, ur, od, other_index, ego_xy)
    _save_network(ctx, engine, key, weights, (x0, xr, ur, od, force if form.own_force else force.clone(), *tape), ego_xy, other_index)
    return u0, X, U


def _ndp_step_backward(ctx, form, who, upstream, need):
    """need: which of (x0, xr, ur, other, weights) require a gradient; returns those five."""
    (x0, xr, ur, od, force, *tape), ego_xy, other_index = _saved_network(ctx, 8)
    eng = ctx.engine
    if all(g is None for g in upstream):
        return (None,) * 5
    _check_installed(eng, ctx.key, who)
    B, N = x0.shape[0], xr.shape[1] - 1
    net_w = ctx.have_w and need[4]
    net = need[1] or need[3] or net_w                        # anything behind the force
    stream, default = _cuda_stream(x0)
    gx0, gxr, gur, gf = _taped_step_vjp(eng, x0, xr, ur, tuple(tape), force, upstream, (need[0], need[1], need[2], net), stream)
    g_other = gw = None
    if net:
        if default:
            eng.synchronize()
        gz = torch.empty((B, *form.slots(other_index), N + 1, 6), dtype=torch.float64, device=x0.device) if need[1] or need[3] else None
        gw = torch.empty(_lib.MLP_NPARAM, dtype=torch.float32, device=x0.device) if net_w else None
        form.vjp(eng, od, other_index, xr, gf, ego_xy=ego_xy, gz=gz, gw=gw, stream=stream)
    if default:
        eng.synchronize()
    if net and need[1]:
        gxr[:, :, :6] -= form.fold(gz)
    if net and need[3]:
        g_other = form.scatter(gz, od, other_index)
    return gx0, gxr, gur, g_other, gw


def _downwash_jvp(form, who, engine, other, other_index, ego_ref, tangents, ego_xy, weights):
    od, ed = other.detach().contiguous(), ego_ref.detach().contiguous()
    (t_other, t_ego, t_w), T, had = _with_t_axis(tangents, (3, 3, 1), who)
    stream, default, _ = _enter(engine, od, weights)
    B, np1 = ed.shape[0], ed.shape[1]
    tz = form.network_tz(t_other, t_ego, other_index)
    f = torch.empty((B, np1, 3), dtype=torch.float32, device=od.device)
    df = torch.empty((B, T, np1, 3), dtype=torch.float64, device=od.device)
    form.jvp(engine, od, other_index, ed, tz=tz, tw=_cast(t_w, torch.float32), ego_xy=ego_xy, n_tan=T, df=df, f_check=f, stream=stream)
    if default:
        engine.synchronize()
    return f, df if had else df[:, 0]


def _ndp_step_jvp(form, who, engine, x0, xr, ur, other, other_index, tangents, ego_xy, weights):
    x0, xr, ur, od = _det(x0), _det(xr), _det(ur), _det(other)
    (tx0, txr, tur, t_other, t_w), T, had = _with_t_axis(tangents, (2, 3, 3, 3, 1), who)
    tx0, txr, tur = (_cast(t, torch.float64) for t in (tx0, txr, tur))
    B, N = x0.shape[0], xr.shape[1] - 1
    stream, default, _ = _enter(engine, x0, weights)
    tape, u0, X, U, force = form.step(engine, stream, default, x0, xr, ur, od, other_index, ego_xy)
    tz, tw = form.network_tz(t_other, txr, other_index), _cast(t_w, torch.float32)
    tf = None
    if tz is not None or tw is not None:
        tf = torch.empty((B, T, N + 1, 3), dtype=torch.float64, device=x0.device)
        form.jvp(engine, od, other_index, xr, tz=tz, tw=tw, ego_xy=ego_xy, n_tan=T, df=tf, stream=stream)
    du0, dX, dU = (torch.empty((B, T) + s, dtype=torch.float64, device=x0.device) for s in ((4,), (N + 1, 10), (N, 4)))
    engine.step_jvp_device(x0, xr, ur, tape, tx0, txr, tur, tf, f=force, du0=du0, dX=dX, dU=dU, stream=stream)
    if default:
        engine.synchronize()
    if not had:
        du0, dX, dU = du0[:, 0], dX[:, 0], dU[:, 0]
    return u0, X, U, du0, dX, dU


class DownwashFunction(torch.autograd.Function):
    """forward(other, engine, ego_ref, ego_xy, weights, other_index) -> f [B,N+1,3] float32, the gated downwash force (mlp_kernel);
    backward: BatchedNMPC.downwash_vjp_device for the gradients of other, ego_ref and weights."""

    @staticmethod
    def forward(ctx, other, engine, ego_ref, ego_xy=None, weights=None, other_index=None):
        return _downwash_forward(ctx, _SINGLE, "DownwashFunction", other, engine, ego_ref, ego_xy, weights, other_index)

    @staticmethod
    def backward(ctx, g_f):
        need = ctx.needs_input_grad
        g_other, g_ego, gw = _downwash_backward(ctx, _SINGLE, "DownwashFunction", g_f, (need[0], need[2], need[4]))
        return (g_other, None, g_ego, None, gw, None)


def downwash(engine, other, ego_ref, ego_xy=None, weights=None, other_index=None):
    """f [B,N+1,3] float32 = the engine's gated downwash network on (other - ego_ref)[..., 0:6], differentiable in `other` (columns 0..5;
    columns 6..9 get 0; with other_index [B] int32 the instances that share a neighbour row add up), `ego_ref` (the negative of the same
    on columns 0..5) and `weights` (a float32 CUDA tensor / nn.Parameter of 17 859 in blob order; when given, the forward first installs
    it in the engine unless it is what was installed last).  The gate is held fixed: ego_xy requiring grad raises.  A row whose upstream
    gradient is not finite adds nothing to the weights' gradient and has NaN in its own input gradient."""
    return DownwashFunction.apply(other, engine, ego_ref, ego_xy, weights, other_index)


class ControlStepNDPFunction(torch.autograd.Function):
    """forward(x0, engine, xr, ur, other, ego_xy, weights, other_index) -> (u0, X, U) float64: the fused control step (one launch);
    backward: the step's adjoint (step_vjp_device) for x0, xr, ur and the force's gradient gf, then the network's backward pass on that gf
    (downwash_vjp_device) for other, weights and xr's share (- g_z on columns 0..5)."""

    @staticmethod
    def forward(ctx, x0, engine, xr, ur, other, ego_xy=None, weights=None, other_index=None):
        return _ndp_step_forward(ctx, _SINGLE, "ControlStepNDPFunction", x0, engine, xr, ur, other, ego_xy, weights, other_index)

    @staticmethod
    def backward(ctx, g_u0, g_X, g_U):
        need = ctx.needs_input_grad
        gx0, gxr, gur, g_other, gw = _ndp_step_backward(ctx, _SINGLE, "ControlStepNDPFunction", (g_u0, g_X, g_U),
                                                        (need[0], need[2], need[3], need[4], need[6]))
        return (gx0, None, gxr, gur, g_other, None, gw, None)


def control_step_ndp(engine, x0, xr, ur, other, ego_xy=None, weights=None, other_index=None):
    """(u0, X, U) = the engine's control step with the fused downwash network, differentiable with respect to x0, xr, ur, the neighbour
    windows `other` and the network's `weights` (see downwash): the step's adjoint, then the network's backward pass on the force's
    gradient.  Held fixed: the step's linearisation point and active set, and the gate (ego_xy requiring grad raises).  Instances whose
    step failed (nonzero status) have NaN gradients of their own inputs and contribute nothing to the weights' gradient."""
    return ControlStepNDPFunction.apply(x0, engine, xr, ur, other, ego_xy, weights, other_index)


class NDPControlStep(torch.nn.Module):
    """control_step_ndp with the network's weights as this module's nn.Parameter `weights` (float32 [17859], blob order), initialised
    from the shipped blob on the engine's device.  forward(x0, xr, ur, other, ego_xy=None, other_index=None) -> (u0, X, U)."""

    def __init__(self, engine, weights=None):
        super().__init__()
        self.engine = engine
        w = torch.as_tensor(_lib.load_weights() if weights is None else weights, dtype=torch.float32).clone()
        dev = getattr(getattr(engine, "cfg", None), "device", None)
        if dev is not None and torch.cuda.is_available():
            w = w.to(torch.device("cuda", int(dev)))
        self.weights = torch.nn.Parameter(w)

    def forward(self, x0, xr, ur, other, ego_xy=None, other_index=None):
        return control_step_ndp(self.engine, x0, xr, ur, other, ego_xy=ego_xy, weights=self.weights, other_index=other_index)


# ---------------------------------------------------------------------------------------------- K neighbours per instance, differentiated
# The K-slot siblings of the block above: the force is the sum over the slots other_index [B,K] (< 0: an empty slot) of the network on
# (other[o_k] - ego_ref)[..., 0:6], each slot behind its own gate (BatchedNMPC.downwash_multi_device); its backward pass is one call
# (BatchedNMPC.downwash_multi_vjp_device).  The same things are held fixed.  The fused step is single-neighbour, so control_step_ndp_multi
# runs the summed prediction into a force tensor and then the external-force step: the route the multi-neighbour rollout takes.

class DownwashMultiFunction(torch.autograd.Function):
    """forward(other, engine, other_index, ego_ref, ego_xy, weights) -> f [B,N+1,3] float32, the summed gated downwash force
    (mlp_multi_kernel); backward: BatchedNMPC.downwash_multi_vjp_device for the gradients of other, ego_ref and weights."""

    @staticmethod
    def forward(ctx, other, engine, other_index, ego_ref, ego_xy=None, weights=None):
        return _downwash_forward(ctx, _MULTI, "DownwashMultiFunction", other, engine, ego_ref, ego_xy, weights, other_index)

    @staticmethod
    def backward(ctx, g_f):
        need = ctx.needs_input_grad
        g_other, g_ego, gw = _downwash_backward(ctx, _MULTI, "DownwashMultiFunction", g_f, (need[0], need[3], need[5]))
        return (g_other, None, None, g_ego, None, gw)


def downwash_multi(engine, other, other_index, ego_ref, ego_xy=None, weights=None):
    """f [B,N+1,3] float32 = the engine's summed downwash force from K neighbours per instance: other [rows,N+1,6 or 10] float64,
    other_index int32 [B,K] the rows of `other` instance i hears (< 0: an empty slot; the same row twice counts twice), each slot behind
    its own gate.  Differentiable in `other` (columns 0..5; instances and slots that share a row add up), `ego_ref` (minus the sum over
    the slots on columns 0..5) and `weights` (as `downwash`: installed first unless they are what was installed last).  The gate is held
    fixed: ego_xy requiring grad raises.  A row whose upstream gradient is not finite adds nothing to the weights' gradient and has NaN
    in the input gradients of its open slots."""
    return DownwashMultiFunction.apply(other, engine, other_index, ego_ref, ego_xy, weights)


class ControlStepNDPMultiFunction(torch.autograd.Function):
    """forward(x0, engine, xr, ur, other, other_index, ego_xy, weights) -> (u0, X, U) float64: the summed prediction (downwash_multi_device
    with ego_ref = xr) into a force tensor, then the external-force control step; backward: the step's adjoint (step_vjp_device) for x0,
    xr, ur and the force's gradient gf, then downwash_multi_vjp_device on that gf for other, weights and xr's share (minus the sum over
    the slots of g_z on columns 0..5)."""

    @staticmethod
    def forward(ctx, x0, engine, xr, ur, other, other_index, ego_xy=None, weights=None):
        return _ndp_step_forward(ctx, _MULTI, "ControlStepNDPMultiFunction", x0, engine, xr, ur, other, ego_xy, weights, other_index)

    @staticmethod
    def backward(ctx, g_u0, g_X, g_U):
        need = ctx.needs_input_grad
        gx0, gxr, gur, g_other, gw = _ndp_step_backward(ctx, _MULTI, "ControlStepNDPMultiFunction", (g_u0, g_X, g_U),
                                                        (need[0], need[2], need[3], need[4], need[7]))
        return (gx0, None, gxr, gur, g_other, None, None, gw)


def control_step_ndp_multi(engine, x0, xr, ur, other, other_index, ego_xy=None, weights=None):
    """(u0, X, U) = the engine's control step compensating the summed downwash of K neighbours per instance (see downwash_multi for
    other / other_index), differentiable with respect to x0, xr, ur, `other` and the network's `weights`: the step's adjoint, then the
    K-slot backward pass of the network on the force's gradient.  The forward is two launches (the summed prediction, then the
    external-force step): the fused step is single-neighbour.  Held fixed: the linearisation point, the active set and the gates (ego_xy
    requiring grad raises).  Instances whose step failed (nonzero status) have NaN gradients of their own inputs and contribute nothing
    to the weights' gradient."""
    return ControlStepNDPMultiFunction.apply(x0, engine, xr, ur, other, other_index, ego_xy, weights)


class NDPControlStepMulti(NDPControlStep):
    """control_step_ndp_multi with the network's weights as this module's nn.Parameter `weights` (see NDPControlStep).
    forward(x0, xr, ur, other, other_index, ego_xy=None) -> (u0, X, U)."""

    def forward(self, x0, xr, ur, other, other_index, ego_xy=None):
        return control_step_ndp_multi(self.engine, x0, xr, ur, other, other_index, ego_xy=ego_xy, weights=self.weights)


# ---------------------------------------------------------------------------------------------- the downwash network, forward mode
# The mirror of the single-neighbour block above (BatchedNMPC.downwash_jvp_device): the first-order change of the force along directions of the neighbour
# windows, of ego_ref and of the weights, and its composition with the step's forward mode.  Held fixed: what the backward holds fixed
# (gate, linearisation point, active set); ego_xy has no tangent.  Plain tensors, no autograd hookup, like control_step_jvp.

def downwash_jvp(engine, other, ego_ref, tangents, ego_xy=None, weights=None, other_index=None):
    """(f, df): the engine's gated downwash force f [B,N+1,3] float32 on (other - ego_ref)[..., 0:6] and its first-order change df
    [B,T,N+1,3] float64 along tangents = (t_other, t_ego_ref, t_weights) (forward mode: BatchedNMPC.downwash_jvp_device).  t_other is
    shaped like `other` ([rows,T,N+1,6 or 10]; columns 6..9 move nothing; with other_index every instance reads its neighbour row's
    direction), t_ego_ref like ego_ref ([B,T,N+1,10]), t_weights [T,17859] float32 in blob order; each may be None (= 0, not all three)
    and each may come without the T axis -- then df is [B,N+1,3] if none has it.  `weights`, when given, are installed first as
    `downwash` does.  The gate is held fixed: ego_xy has no tangent.  No autograd hookup."""
    return _downwash_jvp(_SINGLE, "downwash_jvp", engine, other, other_index, ego_ref, tangents, ego_xy, weights)


def control_step_ndp_jvp(engine, x0, xr, ur, other, tangents, ego_xy=None, weights=None, other_index=None):
    """(u0, X, U, du0, dX, dU): the engine's control step with the fused downwash network and its new iterate, and the first-order change
    of all three along tangents = (tx0, txr, tur, t_other, t_weights) -- control_step_jvp with the force's tangent produced by the
    network's forward mode instead of given.  On one stream: the taped fused step; the network's JVP with tz = t_other[other_index] -
    txr[..., 0:6] (and t_weights), giving tf; BatchedNMPC.step_jvp_device with (tx0, txr, tur, tf) and the force the step wrote.
    Shapes: tx0 [B,T,10], txr [B,T,N+1,10], tur [B,T,N,4], t_other like `other` with the T axis behind its first, t_weights [T,17859]
    float32; None = 0 (not all five); each may come without the T axis, and the outputs carry it unless none does.  Held fixed: the
    linearisation point, the active set and the gate (ego_xy has no tangent).  Instances whose step failed have NaN tangents.  No
    autograd hookup."""
    return _ndp_step_jvp(_SINGLE, "control_step_ndp_jvp", engine, x0, xr, ur, other, other_index, tangents, ego_xy, weights)


def downwash_multi_jvp(engine, other, other_index, ego_ref, tangents, ego_xy=None, weights=None):
    """(f, df): the engine's summed downwash force f [B,N+1,3] float32 from K neighbours per instance (see downwash_multi) and its
    first-order change df [B,T,N+1,3] float64 along tangents = (t_other, t_ego_ref, t_weights), shaped as downwash_jvp takes them (forward
    mode: BatchedNMPC.downwash_multi_jvp_device; every slot reads its neighbour row's direction).  The gates are held fixed.  No autograd
    hookup."""
    return _downwash_jvp(_MULTI, "downwash_multi_jvp", engine, other, other_index, ego_ref, tangents, ego_xy, weights)


def control_step_ndp_multi_jvp(engine, x0, xr, ur, other, other_index, tangents, ego_xy=None, weights=None):
    """(u0, X, U, du0, dX, dU): control_step_ndp_multi's step and new iterate, and the first-order change of all three along tangents =
    (tx0, txr, tur, t_other, t_weights), shaped as control_step_ndp_jvp takes them.  On one stream: the summed prediction, the taped
    external-force step, the network's K-slot JVP with tz[:, :, k] = t_other[other_index[:, k]] - txr[..., 0:6] (and t_weights), giving
    tf; BatchedNMPC.step_jvp_device with (tx0, txr, tur, tf) and the same force.  Held fixed: the linearisation point, the active set and
    the gates.  Instances whose step failed have NaN tangents.  No autograd hookup."""
    return _ndp_step_jvp(_MULTI, "control_step_ndp_multi_jvp", engine, x0, xr, ur, other, other_index, tangents, ego_xy, weights)


# ---------------------------------------------------------------------------------------------- the controller's own numbers, differentiated
# What is differentiated: the step's QP with respect to the cost weights Qd [10], Rd [4] and the mass (BatchedNMPC.step_vjp_device with
# gmodel: ndp_step_vjp_model_device), beside x0, xr, ur and f as control_step_trajectory gives them.  Held fixed: linearisation point, x0 and
# active set, as in every derivative here.  The network's backward (control_step_ndp) is not combined with this one: a caller who wants both
# runs the force through `downwash` and passes it as f.

def _model_values(Qd, Rd, mass):
    """(Qd, Rd, mass) as host tuples of Python floats (None = not given).  Tensors on a device are copied to the host: that synchronises."""
    h = lambda t, n: None if t is None else tuple(float(v) for v in torch.as_tensor(t).detach().to("cpu", torch.float64).reshape(n))  # noqa: E731
    m = h(mass, 1)
    return h(Qd, 10), h(Rd, 4), None if m is None else m[0]


def _engine_model(engine):
    return tuple(engine.cfg.Qd), tuple(engine.cfg.Rd), float(engine.cfg.mass)


def _install_model(engine, Qd, Rd, mass):
    """Installs the values through engine.set_model unless they are what the engine holds; returns the model the step then runs with."""
    q, r, m = _model_values(Qd, Rd, mass)
    eq, er, em = _engine_model(engine)
    new = (q if q is not None and q != eq else None, r if r is not None and r != er else None, m if m is not None and m != em else None)
    if any(v is not None for v in new):
        engine.set_model(Qd=new[0], Rd=new[1], mass=new[2])
    return _engine_model(engine)


class TunableControlStepFunction(torch.autograd.Function):
    """forward(x0, engine, xr, ur, Qd, Rd, mass, f) -> (u0, X, U) float64; backward: one call of the adjoint with the model gradient
    (BatchedNMPC.step_vjp_device, gmodel=) for the gradients of x0, xr, ur, f, Qd, Rd and mass."""

    @staticmethod
    def forward(ctx, x0, engine, xr, ur, Qd, Rd, mass=None, f=None):
        x0, xr, ur, fd = _det(x0), _det(xr), _det(ur), _det(f)
        ctx.model = _install_model(engine, Qd, Rd, mass)
        tape, u0, X, U = _taped_step(engine, *_cuda_stream(x0), x0, xr, ur, f=fd)
        ctx.engine = engine
        ctx.f_dtype = f.dtype if isinstance(f, torch.Tensor) else None
        ctx.like = tuple(None if not isinstance(t, torch.Tensor) else (t.shape, t.dtype, t.device) for t in (Qd, Rd, mass))
        ctx.save_for_backward(x0, xr, ur, *tape, *(() if fd is None else (fd,)))
        return u0, X, U

    @staticmethod
    def backward(ctx, g_u0, g_X, g_U):
        x0, xr, ur, t0, t1, t2, *rest = ctx.saved_tensors
        force = rest[0] if rest else None
        eng = ctx.engine
        if g_u0 is None and g_X is None and g_U is None:
            return (None,) * 8
        if _engine_model(eng) != ctx.model:
            raise RuntimeError("TunableControlStepFunction: the engine's model (Qd, Rd, mass) was changed between this forward and its "
                               "backward (the backward recomputes the step from the engine's model): run the backward before the next "
                               "forward with other values, or set the model back first")
        need = ctx.needs_input_grad
        gm = torch.empty(x0.shape[0], 16, dtype=torch.float64, device=x0.device)
        stream, default = _cuda_stream(x0)
        gx0, gxr, gur, gf = _taped_step_vjp(eng, x0, xr, ur, (t0, t1, t2), force, (g_u0, g_X, g_U),
                                            (need[0], need[2], need[3], need[7] and ctx.f_dtype is not None), stream, gmodel=gm)
        if default:
            eng.synchronize()
        # a failed step (NaN in its row) contributes nothing: control_step_ndp's convention for the network's weights
        tot = torch.where(torch.isfinite(gm).all(dim=1, keepdim=True), gm, torch.zeros_like(gm)).sum(dim=0)
        out = []
        for like, need_i, part in zip(ctx.like, need[4:7], (tot[0:10], tot[10:14], tot[14:15])):
            out.append(None if like is None or not need_i else part.reshape(like[0]).to(device=like[2], dtype=like[1]))
        return (gx0, None, gxr, gur, out[0], out[1], out[2], None if gf is None else gf.to(ctx.f_dtype))


def control_step_tunable(engine, x0, xr, ur, Qd, Rd, mass=None, f=None):
    """(u0, X, U) = the engine's control step with the cost weights Qd [10], Rd [4] and (optionally) the mass given as float64 tensors on
    any device, differentiable with respect to them and to x0, xr, ur and f (the latter as control_step_trajectory).
    Forward: the values are installed in the engine (BatchedNMPC.set_model) unless they are what it holds -- compared by value on the
    host, so 15 doubles move to the host on every call, which SYNCHRONISES when they live on the device -- then the tape is recorded
    and the step runs; the iterate and kept sets (the warm start) survive a change of the model.
    Backward: one adjoint launch; the gradients of Qd, Rd and mass are the sum over the instances of the per-instance rows, a failed step
    (nonzero status) contributing nothing.  If the engine's model was changed between a forward and its backward, the backward raises.
    The library refuses a negative Qd, a non-positive Rd or mass (NdpError): keeping parameters positive is the caller's business (project
    them after the optimiser's step, or optimise their logarithms) -- nothing is clamped here.
    The downwash network is not part of this entry point (no other / ego_xy): see control_step_ndp for its gradients."""
    return TunableControlStepFunction.apply(x0, engine, xr, ur, Qd, Rd, mass, f)


class TunableControlStep(torch.nn.Module):
    """control_step_tunable with Qd [10] and Rd [4] (and, with learn_mass=True, mass) as this module's float64 nn.Parameters, initialised
    from the engine's cfg.  forward(x0, xr, ur, f=None) -> (u0, X, U).  Parameters are not clamped: see control_step_tunable."""

    def __init__(self, engine, learn_mass=False):
        super().__init__()
        self.engine = engine
        self.Qd = torch.nn.Parameter(torch.tensor(list(engine.cfg.Qd), dtype=torch.float64))
        self.Rd = torch.nn.Parameter(torch.tensor(list(engine.cfg.Rd), dtype=torch.float64))
        self.mass = torch.nn.Parameter(torch.tensor(float(engine.cfg.mass), dtype=torch.float64)) if learn_mass else None

    def forward(self, x0, xr, ur, f=None):
        return control_step_tunable(self.engine, x0, xr, ur, self.Qd, self.Rd, mass=self.mass, f=f)


# ---------------------------------------------------------------------------------------------- training the downwash network
# The reference's loop (nn_train.py:129-157 with --SN): full-batch Adam, then every weight matrix scaled back onto a spectral-norm cap.  On the
# device both are ONE launch behind the weight gradient (BatchedNMPC.mlp_adam_sn_device): no singular value travels to the host.

class DownwashAdamSN(torch.optim.Optimizer):
    """torch.optim.Adam (its defaults: no weight decay, no amsgrad) followed by the spectral-norm cap `sn` on the four weight matrices
    (sn = 0: no cap), for ONE parameter: the downwash network's 17 859 float32 values in blob order on the engine's device -- the tensor
    handed to downwash(..., weights=w).  The reference's options: lr 1e-4, betas (0.9, 0.999), eps 1e-8 (nn_train.py:90,132).

    The state lives in tensors on the parameter's device: m, v (float32 [17859]), step (int64 [1], advanced by the kernel), sigma (float64
    [4]: the layers' norms after the last step) and info (int32 [4]: [0] the last step was skipped because its gradient was not finite,
    [1] bitmask of the layers it scaled); state_dict() / load_state_dict() carry them with their dtypes.  step() enqueues one call on the
    current stream and never synchronises; on torch's default stream, which the C interface cannot name, the call goes on the engine's
    own stream between two waits, as every layer of this module does it.  install=True: the engine's network is the updated parameter
    behind every step (also a skipped one), and the next downwash(weights=w) does not install it again.

    The kernel writes through the parameter's pointer, which does not move its version counter: step() bumps it, so that a following
    forward can tell the weights have changed."""

    _DTYPES = {"m": torch.float32, "v": torch.float32, "step": torch.int64, "sigma": torch.float64, "info": torch.int32}

    def __init__(self, params, engine, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, sn=0.0, install=True):
        if isinstance(params, torch.Tensor):
            params = [params]
        if not (lr == lr and abs(lr) != float("inf")):
            raise ValueError(f"DownwashAdamSN: lr = {lr} is not finite")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"DownwashAdamSN: betas = {betas} must lie in [0, 1)")
        if not eps > 0.0:
            raise ValueError(f"DownwashAdamSN: eps = {eps} must be positive")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, sn=float(sn), install=bool(install)))
        ps = [p for g in self.param_groups for p in g["params"]]
        if len(ps) != 1 or ps[0].numel() != _lib.MLP_NPARAM or ps[0].dim() != 1 or ps[0].dtype != torch.float32 or not ps[0].is_contiguous():
            raise ValueError(f"DownwashAdamSN: expected ONE contiguous float32 parameter of {_lib.MLP_NPARAM} values (the network's blob)")
        self.engine = engine

    def _state_of(self, p):
        st = self.state[p]
        if not st:
            st["m"], st["v"] = torch.zeros_like(p, memory_format=torch.preserve_format), torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] = torch.zeros(1, dtype=torch.int64, device=p.device)
            st["sigma"] = torch.zeros(4, dtype=torch.float64, device=p.device)
            st["info"] = torch.zeros(4, dtype=torch.int32, device=p.device)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        p = group["params"][0]
        if p.grad is None:
            return loss
        g = p.grad
        if g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape:
            raise ValueError("DownwashAdamSN: the gradient must be a contiguous float32 tensor of the parameter's shape")
        st = self._state_of(p)
        eng = self.engine
        stream, default = _cuda_stream(p)
        eng.mlp_adam_sn_device(p.detach(), g, st["m"], st["v"], st["step"], lr=group["lr"], betas=group["betas"], eps=group["eps"],
                               sn=group["sn"], sigma=st["sigma"], info=st["info"], install=group["install"], stream=stream)
        if default:
            eng.synchronize()
        torch.autograd.graph.increment_version(p)
        if group["install"]:                 # what _install_weights would note: the parameter as it now is IS the engine's network
            eng._mlp_installed, eng._mlp_installed_tensor = (p.data_ptr(), p._version), p
        return loss

    def load_state_dict(self, state_dict):
        """torch's loader casts floating-point state to the parameter's dtype (sigma is float64) and leaves `step` where it was saved: the
        five tensors are taken from `state_dict` again, as copies on the parameter's device with their own dtypes."""
        super().load_state_dict(state_dict)
        ps = [p for g in self.param_groups for p in g["params"]]
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        for p, i in zip(ps, ids):
            src = state_dict["state"].get(i)
            if src:
                self.state[p] = {k: torch.as_tensor(src[k]).detach().to(device=p.device, dtype=dt, copy=True) for k, dt in self._DTYPES.items()}


# ---------------------------------------------------------------------------------------------- the network on sample rows
# The form the reference trains and evaluates on (nn_train.py:99-108,131,142-147; nn_test.py's force-field grids): flat rows x [n,6],
# y [n,3] in float32, no prediction window, no gate, any n.  Any engine serves (its batch shape plays no part); mini-batches are index lists.

def downwash_rows(engine, z, weights=None, index=None):
    """f [M,3] float32 = the engine's network on the float32 CUDA rows z [R,6] (BatchedNMPC.mlp_rows_device): row m from data row
    index[m] (int32 [M]; None: every row in order); an index < 0 or >= R gives a row of exact zeros.  `weights`, when given, is
    installed first as downwash does it.  NO autograd: the result carries no graph, whatever requires grad -- this is for evaluation sets
    and the reference's force-field grids; fit through downwash_fit_rows."""
    zd = z.detach()
    stream, default, _ = _enter(engine, zd, weights)
    f = torch.empty((zd.shape[0] if index is None else index.shape[0], 3), dtype=torch.float32, device=zd.device)
    engine.mlp_rows_device(zd, f, index=index, stream=stream)
    if default:
        engine.synchronize()
    return f


class DownwashFitRowsFunction(torch.autograd.Function):
    """forward(weights, engine, z, y, index, row_weight, scale, groups, info) -> the float64 scalar loss, by the ONE fused call that
    also leaves the weight gradient (BatchedNMPC.mlp_fit_rows_device), which is kept; backward: that gradient times the upstream."""

    @staticmethod
    def forward(ctx, weights, engine, z, y, index, row_weight, scale, groups, info):
        stream, default, _ = _enter(engine, z, weights)
        loss = torch.empty(1, dtype=torch.float64, device=z.device)
        gw = torch.empty(_lib.MLP_NPARAM, dtype=torch.float32, device=z.device) if ctx.needs_input_grad[0] else None
        engine.mlp_fit_rows_device(z, y, scale, index=index, row_weight=row_weight, groups=groups, loss=loss, gw=gw, info=info, stream=stream)
        if default:
            engine.synchronize()
        ctx.gw = gw
        return loss[0]

    @staticmethod
    def backward(ctx, g_loss):
        gw = ctx.gw
        return (None if gw is None else gw * g_loss.to(gw.dtype),) + (None,) * 8


def downwash_fit_rows(engine, z, y, weights, index=None, row_weight=None, scale=None, groups=0, info=None):
    """The float64 scalar loss scale * sum_m rw |net(z[index[m]]) - y[index[m]]|^2 of the engine's network on sample rows, differentiable
    in `weights` only (a float32 CUDA tensor / nn.Parameter of 17 859 in blob order, installed first as downwash does it): loss and weight
    gradient come out of ONE fused call in the forward, the backward multiplies the kept gradient by its upstream.  z [R,6], y [R,3],
    row_weight [R] (None: 1) float32 CUDA, none of them differentiated; index int32 [M] (None: every row) -- an index < 0 or >= R is an
    empty slot, an index listed twice counts twice, fixed-size mini-batches pad with -1.  scale None: 1 / (3 M), nn.MSELoss over M rows
    (with padded mini-batches pass 1 / (3 M_real)).  groups: BatchedNMPC.mlp_fit_rows_device's.  info: an int32 CUDA [2] tensor that
    receives rows used / rows skipped (non-finite rows add nothing)."""
    M = z.shape[0] if index is None else index.shape[0]
    return DownwashFitRowsFunction.apply(weights, engine, z.detach(), y.detach(), index, None if row_weight is None else row_weight.detach(),
                                         1.0 / (3.0 * M) if scale is None else float(scale), int(groups), info)


# ---------------------------------------------------------------------------------------------- the plant over an input sequence
# The rigid body the closed-loop rollouts integrate (ndp_plant_step_device), over GIVEN inputs and forces: one launch for the whole
# sequence, and the derivative of exactly that arithmetic -- each force held over its tick, the quaternion renormalised once per tick.

class PlantRolloutFunction(torch.autograd.Function):
    """forward(x0, engine, u, f, dt, substeps) -> xs [ticks,B,10] float64, the state after every tick (BatchedNMPC.plant_rollout_device);
    backward: ONE BatchedNMPC.plant_rollout_vjp_device call on the saved log for the gradients of x0, u and f."""

    @staticmethod
    def forward(ctx, x0, engine, u, f, dt, substeps):
        x0d, ud = x0.detach().contiguous(), u.detach().contiguous()
        fd = None if f is None else f.detach().contiguous()
        stream, default, _ = _enter(engine, x0d)
        xs = torch.empty((ud.shape[0], ud.shape[1], 10), dtype=torch.float64, device=x0d.device)
        engine.plant_rollout_device(x0d, ud, xs, f=fd, dt=dt, substeps=substeps, stream=stream)
        if default:
            engine.synchronize()
        ctx.engine, ctx.dt, ctx.substeps, ctx.have_f = engine, dt, substeps, fd is not None
        ctx.save_for_backward(x0d, ud, xs, *(() if fd is None else (fd,)))
        return xs

    @staticmethod
    def backward(ctx, g_xs):
        x0d, ud, xs, *rest = ctx.saved_tensors
        fd = rest[0] if ctx.have_f else None
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.have_f and ctx.needs_input_grad[3])
        if not any(need):
            return (None,) * 6
        K, B = ud.shape[0], ud.shape[1]
        gx0, gu, gf = (torch.empty(s, dtype=torch.float64, device=x0d.device) if n else None
                       for n, s in zip(need, ((B, 10), (K, B, 4), (K, B, 3))))
        stream, default, _ = _enter(ctx.engine, x0d)
        ctx.engine.plant_rollout_vjp_device(x0d, ud, xs, g_xs.to(torch.float64).contiguous(), f=fd, gx0=gx0, gu=gu, gf=gf, dt=ctx.dt,
                                            substeps=ctx.substeps, stream=stream)
        if default:
            ctx.engine.synchronize()
        return gx0, None, gu, gf, None, None


def plant_rollout(engine, x0, u, f=None, dt=CP.ts_nmpc, substeps=4):
    """xs [ticks,B,10] float64 = the engine's plant from x0 [B,10] over the inputs u [ticks,B,4] and the external forces f [ticks,B,3]
    (None: none), float64 CUDA tensors: per tick RK4 with `substeps` over dt with the input and the force held, then the quaternion
    renormalised -- row k is what k + 1 ndp_plant_step_device calls give, bit for bit.  Differentiable in x0, u and f (reverse mode over
    the saved log, one call).  Mass and gravity are the engine's and are not differentiated.  The engine's state is not touched: unlike
    the control_step* Functions, two forward calls return the same values."""
    return PlantRolloutFunction.apply(x0, engine, u, f, float(dt), int(substeps))


def plant_step(engine, x, u, f=None, dt=CP.ts_nmpc, substeps=4):
    """[B,10] float64 = one tick of the plant from x [B,10] with the input u [B,4] and the force f [B,3] (None: none): plant_rollout's
    ticks = 1 case.  The piece that chains with control_step*: u0 = control_step(...); x = plant_step(engine, x, u0)."""
    return plant_rollout(engine, x, u.unsqueeze(0), None if f is None else f.unsqueeze(0), dt, substeps)[0]


def plant_rollout_jvp(engine, x0, u, tangents, f=None, dt=CP.ts_nmpc, substeps=4):
    """(xs, dxs): plant_rollout's log xs [ticks,B,10] and its first-order change dxs [ticks,B,T,10] along tangents = (tx0, tu, tf) (forward
    mode: BatchedNMPC.plant_rollout_jvp_device).  tx0 [B,T,10], tu [ticks,B,T,4], tf [ticks,B,T,3]; each may be None (= 0, not all three) and
    each may come without the T axis -- then dxs is [ticks,B,10] if none has it.  tf may be given with f None (the direction away from no
    force).  T <= 8.  No autograd hookup."""
    x0d, ud = x0.detach().contiguous(), u.detach().contiguous()
    fd = None if f is None else f.detach().contiguous()
    ts, Ts, had = [], set(), False
    for t, n in zip(tangents, (2, 3, 3)):                      # (dimensions without the T axis, which sits in front of the last)
        if t is not None:
            t = t.detach().to(torch.float64)
            if t.dim() == n:
                t = t.unsqueeze(-2)
            elif t.dim() == n + 1:
                had = True
            else:
                raise ValueError(f"plant_rollout_jvp: a tangent has {t.dim()} dimensions, expected {n} or {n + 1}")
            Ts.add(int(t.shape[-2]))
            t = t.contiguous()
        ts.append(t)
    if not Ts:
        raise ValueError("plant_rollout_jvp: no tangent (all None)")
    if len(Ts) > 1:
        raise ValueError(f"plant_rollout_jvp: the tangents disagree on the number of directions ({sorted(Ts)})")
    T, (K, B) = Ts.pop(), ud.shape[:2]
    stream, default, _ = _enter(engine, x0d)
    xs = torch.empty((K, B, 10), dtype=torch.float64, device=x0d.device)
    dxs = torch.empty((K, B, T, 10), dtype=torch.float64, device=x0d.device)
    engine.plant_rollout_jvp_device(x0d, ud, dxs, f=fd, tx0=ts[0], tu=ts[1], tf=ts[2], n_tan=T, xs_check=xs, dt=dt, substeps=substeps,
                                    stream=stream)
    if default:
        engine.synchronize()
    return xs, dxs if had else dxs[:, :, 0]


# ---------------------------------------------------------------------------------------------- the closed loop, one call per direction
class ClosedLoopFunction(torch.autograd.Function):
    """forward(x0, engine, xr, ur, f, fp, Qd, Rd, mass, dt, substeps) -> (xs [ticks,B,10], us [ticks,B,4], Xs [ticks,B,N+1,10]) float64:
    BatchedNMPC.closed_loop_device with its tape; backward: ONE BatchedNMPC.closed_loop_vjp_device call for the gradients of x0, xr, ur, f,
    fp, Qd, Rd and mass (only those that require one are computed)."""

    @staticmethod
    def forward(ctx, x0, engine, xr, ur, f, fp, Qd, Rd, mass, dt, substeps):
        x0, xr, ur, fd, fpd = _det(x0), _det(xr), _det(ur), _det(f), _det(fp)
        ctx.model = _install_model(engine, Qd, Rd, mass)
        ctx.set_materialize_grads(False)       # (an output the loss does not use arrives as None: the call's NULL upstream)
        K, B, N = xr.shape[0], xr.shape[1], xr.shape[2] - 1
        stream, default, _ = _enter(engine, x0)
        new = lambda *s: torch.empty(s, dtype=torch.float64, device=x0.device)  # noqa: E731
        xs, us, Xs, tape = new(K, B, 10), new(K, B, 4), new(K, B, N + 1, 10), engine.closed_loop_tape(K)
        engine.closed_loop_device(x0, xr, ur, xs, us, f=fd, fp=fpd, Xs=Xs, tape=tape, dt=dt, substeps=substeps, stream=stream)
        if default:                            # torch's default stream: the loop went on the engine's own (the C-ABI's NULL)
            engine.synchronize()
        ctx.engine, ctx.dt, ctx.substeps = engine, dt, substeps
        ctx.have = (fd is not None, fpd is not None)
        ctx.f_dtype = f.dtype if isinstance(f, torch.Tensor) else None
        ctx.like = tuple(None if not isinstance(t, torch.Tensor) else (t.shape, t.dtype, t.device) for t in (Qd, Rd, mass))
        ctx.save_for_backward(x0, xr, ur, xs, us, tape, *(t for t in (fd, fpd) if t is not None))
        return xs, us, Xs

    @staticmethod
    def backward(ctx, g_xs, g_us, g_Xs):
        x0, xr, ur, xs, us, tape, *rest = ctx.saved_tensors
        fd = rest[0] if ctx.have[0] else None
        fpd = rest[-1] if ctx.have[1] else None
        eng, need = ctx.engine, ctx.needs_input_grad
        want = (need[0], need[2], need[3], need[4] and fd is not None, need[5] and fpd is not None,
                any(n and like is not None for n, like in zip(need[6:9], ctx.like)))
        if (g_xs is None and g_us is None and g_Xs is None) or not any(want):
            return (None,) * 11
        if _engine_model(eng) != ctx.model:
            raise RuntimeError("ClosedLoopFunction: the engine's model (Qd, Rd, mass) was changed between this forward and its backward "
                               "(the backward recomputes every step from the engine's model): run the backward before the next forward "
                               "with other values, or set the model back first")
        K, B, N = xr.shape[0], xr.shape[1], xr.shape[2] - 1
        ups = tuple(None if g is None else g.to(torch.float64).contiguous() for g in (g_xs, g_us, g_Xs))
        gx0, gxr, gur, gf, gfp, gm = (torch.empty(*s, dtype=torch.float64, device=x0.device) if w else None for w, s in zip(
            want, ((B, 10), (K, B, N + 1, 10), (K, B, N, 4), (K, B, N + 1, 3), (K, B, 3), (B, 16))))
        stream, default = _cuda_stream(x0)
        eng.closed_loop_vjp_device(x0, xr, ur, xs, us, tape, f=fd, fp=fpd, gxs=ups[0], gus=ups[1], gXs=ups[2], gx0=gx0, gxr=gxr, gur=gur, gf=gf,
                                   gfp=gfp, gmodel=gm, dt=ctx.dt, substeps=ctx.substeps, stream=stream)
        if default:
            eng.synchronize()
        out = [None, None, None]
        if gm is not None:
            # a failed vehicle (NaN in its row) contributes nothing: control_step_tunable's convention
            tot = torch.where(torch.isfinite(gm).all(dim=1, keepdim=True), gm, torch.zeros_like(gm)).sum(dim=0)
            for i, (like, need_i, part) in enumerate(zip(ctx.like, need[6:9], (tot[0:10], tot[10:14], tot[14:15] + tot[15:16]))):
                if like is not None and need_i:
                    out[i] = part.reshape(like[0]).to(device=like[2], dtype=like[1])
        return (gx0, None, gxr, gur, None if gf is None else gf.to(ctx.f_dtype), gfp, out[0], out[1], out[2], None, None)


def closed_loop(engine, x0, xr, ur, f=None, fp=None, Qd=None, Rd=None, mass=None, dt=CP.ts_nmpc, substeps=4):
    """(xs, us, Xs) = the closed loop of the engine's controller and plant over given windows, `ticks` ticks in one call: from x0 [B,10] and
    the engine's warm start, per tick the control step with xr[k] [B,N+1,10], ur[k] [B,N,4] and the force f[k] [B,N+1,3] (float32; None:
    none) the controller sees, then the plant tick with u0_k and the force fp[k] [B,3] (None: none) on the plant.  xs [ticks,B,10] the
    states x_{k+1}, us [ticks,B,4] the inputs u0_k, Xs [ticks,B,N+1,10] the steps' predicted states -- the values the chain
    control_step_trajectory -> plant_step gives, bit for bit, and like it every call advances the engine's iterate and kept sets.
    Differentiable in x0, xr, ur, f, fp and -- given as float64 tensors, installed as control_step_tunable installs them -- the cost weights
    Qd [10], Rd [4] and the mass (its gradient: the controller's share plus the plant's); the backward is ONE call, with every tick's
    linearisation point and final active set held fixed as in every derivative here.  Gravity is not differentiated."""
    return ClosedLoopFunction.apply(x0, engine, xr, ur, f, fp, Qd, Rd, mass, float(dt), int(substeps))


def closed_loop_jvp(engine, x0, xr, ur, tangents, f=None, fp=None, dt=CP.ts_nmpc, substeps=4, tmodel=None):
    """(xs, us, Xs, dxs, dus, dXs): closed_loop's values and their first-order change along tangents = (tx0, txr, tur, tf, tfp) (forward
    mode: ONE BatchedNMPC.closed_loop_device call with a tape, then ONE BatchedNMPC.closed_loop_jvp_device call).  tx0 [B,T,10], txr
    [ticks,B,T,N+1,10], tur [ticks,B,T,N,4], tf [ticks,B,T,N+1,3] (the direction of the force the controller sees, float64; it needs a
    use_fd engine), tfp [ticks,B,T,3]; each may be None (= 0, not all five) and each may come without the T axis -- then dxs [ticks,B,10],
    dus [ticks,B,4] and dXs [ticks,B,N+1,10] come without it if none has it, else dxs [ticks,B,T,10], dus [ticks,B,T,4], dXs
    [ticks,B,T,N+1,10].  T <= 8.  Every tick's linearisation point and final active set are held fixed, as in every derivative here.  No
    autograd hookup.  Like closed_loop, every call advances the engine's iterate and kept sets.
    tmodel ([16], [T,16] or [B,T,16]; model_tangent builds one): the direction of the cost weights and the mass, constant over the ticks and
    added to the data's (ndp_closed_loop_jvp_model_device: column 14 the controller's mass, 15 the plant's); with it `tangents` may be all
    None, and [16] counts as a direction without the T axis."""
    x0d, xrd, urd, fd, fpd = _det(x0), _det(xr), _det(ur), _det(f), _det(fp)
    ts, Ts, had = [], set(), False
    for t, n, axis in zip(tangents, (2, 4, 4, 4, 3), (1, 2, 2, 2, 2)):   # (dimensions without the T axis, and where it sits)
        if t is not None:
            t = t.detach().to(torch.float64)
            if t.dim() == n:
                t = t.unsqueeze(axis)
            elif t.dim() == n + 1:
                had = True
            else:
                raise ValueError(f"closed_loop_jvp: a tangent has {t.dim()} dimensions, expected {n} or {n + 1}")
            Ts.add(int(t.shape[axis]))
            t = t.contiguous()
        ts.append(t)
    if not Ts and tmodel is None:
        raise ValueError("closed_loop_jvp: no tangent (all None)")
    if len(Ts) > 1:
        raise ValueError(f"closed_loop_jvp: the tangents disagree on the number of directions ({sorted(Ts)})")
    K, B, N = xrd.shape[0], xrd.shape[1], xrd.shape[2] - 1
    T, kw = (Ts.pop() if Ts else None), {}
    if tmodel is not None:
        kw["tmodel"], had_m = _model_direction("closed_loop_jvp", tmodel, B, T, x0d.device)
        T, had = int(kw["tmodel"].shape[1]), had or had_m
    stream, default, _ = _enter(engine, x0d)
    new = lambda *s: torch.empty(s, dtype=torch.float64, device=x0d.device)  # noqa: E731
    xs, us, Xs, tape = new(K, B, 10), new(K, B, 4), new(K, B, N + 1, 10), engine.closed_loop_tape(K)
    dxs, dus, dXs = new(K, B, T, 10), new(K, B, T, 4), new(K, B, T, N + 1, 10)
    engine.closed_loop_device(x0d, xrd, urd, xs, us, f=fd, fp=fpd, Xs=Xs, tape=tape, dt=dt, substeps=substeps, stream=stream)
    engine.closed_loop_jvp_device(x0d, xrd, urd, xs, us, tape, dxs, dus, f=fd, fp=fpd, tx0=ts[0], txr=ts[1], tur=ts[2], tf=ts[3], tfp=ts[4],
                                  dXs=dXs, n_tan=T, dt=dt, substeps=substeps, stream=stream, **kw)
    if default:
        engine.synchronize()
    return (xs, us, Xs) + ((dxs, dus, dXs) if had else (dxs[:, :, 0], dus[:, :, 0], dXs[:, :, 0]))



# ---------------------------------------------------------------------------------------------- the downwash force on the plant, differentiated
# The force the neighbours' ACTUAL states put on the ACTUAL vehicle (ndp_plant_force_multi_device): the link between the states and the `f`
# of plant_rollout / plant_step.  What is differentiated: scale x the fp32 network on the fp32-rounded (x[o] - x[v])[0:6] (the rounding
# counts as the identity), summed over the slots.  What is held fixed: the r_horiz gate (piecewise constant).

def _plant_index(other_index, who):
    """other_index None, [B] or [B,K] -> None or a contiguous int32 [B,K]."""
    if other_index is None:
        return None
    if other_index.dim() not in (1, 2):
        raise ValueError(f"{who}: other_index must be int32 [B] or [B,K]")
    idx = other_index if other_index.dim() == 2 else other_index.unsqueeze(1)
    return idx.to(torch.int32).contiguous()


def _scatter_gz_states(gz, x, idx):
    """dL/dx [B,10] from g_z [B,K,6]: + g_z[v][k] on x[o_k][0:6], - g_z[v][k] on x[v][0:6], columns 6..9 zero; vehicles and slots that share
    a neighbour add up.  A vehicle in its own slot sees z = x[v] - x[v]: its two shares cancel, so that slot is left out of both (an exactly
    zero contribution)."""
    B = x.shape[0]
    g = torch.zeros_like(x)
    own = idx == torch.arange(B, device=idx.device, dtype=idx.dtype)[:, None]
    has = (idx >= 0) & (idx < B) & ~own
    g[:, :6].index_add_(0, idx[has].long(), gz[has])
    g[:, :6] -= torch.where(has[:, :, None], gz, torch.zeros_like(gz)).sum(dim=1)
    return g


class PlantForceFunction(torch.autograd.Function):
    """forward(x, engine, other_index, gate, scale, weights) -> f [B,3] float64, the summed downwash force on the plant
    (BatchedNMPC.plant_force_multi_device); backward: ONE BatchedNMPC.plant_force_multi_vjp_device call and the scatter of its g_z onto
    the states."""

    @staticmethod
    def forward(ctx, x, engine, other_index, gate, scale, weights=None):
        xd = x.detach().contiguous()
        idx = _plant_index(other_index, "PlantForceFunction")
        stream, default, ctx.key = _enter(engine, xd, weights)
        f = torch.empty((xd.shape[0], 3), dtype=torch.float64, device=xd.device)
        if idx is None:
            f.zero_()
        else:
            engine.plant_force_multi_device(xd, idx, f, gate=gate, scale=scale, stream=stream)
            if default:
                engine.synchronize()
        ctx.engine, ctx.gate, ctx.scale = engine, gate, scale
        ctx.have_w, ctx.have_idx = weights is not None, idx is not None
        ctx.save_for_backward(xd, *(() if idx is None else (idx,)))
        return f

    @staticmethod
    def backward(ctx, g_f):
        xd, *rest = ctx.saved_tensors
        need = ctx.needs_input_grad
        want_w = ctx.have_w and need[5]
        if not ctx.have_idx:          # nobody has a neighbour: the force is the constant 0
            return (torch.zeros_like(xd) if need[0] else None, None, None, None, None,
                    torch.zeros(_lib.MLP_NPARAM, dtype=torch.float32, device=xd.device) if want_w else None)
        idx = rest[0]
        eng = ctx.engine
        _check_installed(eng, ctx.key, "PlantForceFunction")
        B, K = idx.shape
        gz = torch.empty((B, K, 6), dtype=torch.float64, device=xd.device) if need[0] else None
        gw = torch.empty(_lib.MLP_NPARAM, dtype=torch.float32, device=xd.device) if want_w else None
        if gz is None and gw is None:
            return (None,) * 6
        stream, default, _ = _enter(eng, xd)
        eng.plant_force_multi_vjp_device(xd, idx, g_f.to(torch.float64).contiguous(), gz=gz, gw=gw, gate=ctx.gate, scale=ctx.scale,
                                         stream=stream)
        if default:
            eng.synchronize()
        return (_scatter_gz_states(gz, xd, idx) if need[0] else None, None, None, None, None, gw)


def plant_force(engine, x, other_index, gate=True, scale=1.0, weights=None):
    """f [B,3] float64 = the downwash force the neighbours' states put on every vehicle: x [B,10] float64 the vehicles' actual states,
    other_index int32 [B] or [B,K] (vehicle v hears x[other_index[v][k]]; < 0 or >= B: an empty slot; the same index twice counts twice;
    None: nobody has a neighbour), each slot behind its own r_horiz gate (gate False: open), the slots' forces times `scale` summed in
    float64 -- the values of BatchedNMPC.plant_force_multi_device, bit for bit.  Differentiable in `x` (per slot + g_z on x[o][0:6] and
    - g_z on x[v][0:6]; columns 6..9 get 0) and `weights` (as `downwash_multi`: a float32 CUDA tensor / nn.Parameter of 17 859 in blob
    order, installed first unless it is what was installed last; replaced before the backward: RuntimeError).  The gate is held fixed.  A
    vehicle whose upstream gradient is not finite adds nothing to the weights' gradient and has NaN in the input gradients of its open
    slots.  With plant_step: f = plant_force(eng, x, idx); x = plant_step(eng, x, u, f) is a differentiable formation tick on the plant
    side."""
    return PlantForceFunction.apply(x, engine, other_index, bool(gate), float(scale), weights)


def plant_force_jvp(engine, x, other_index, tangents, gate=True, scale=1.0, weights=None):
    """(f, df): plant_force's f [B,3] float64 and its first-order change df [B,T,3] float64 along tangents = (tx, tw) (forward mode:
    BatchedNMPC.plant_force_multi_jvp_device).  tx [B,T,10] float64, directions of the states (the device gathers tx[o] - tx[v] per slot:
    nothing is scattered here); tw [T,17859] float32, directions of the weights; each may be None (= 0, not both) and each may come without
    the T axis -- then df is [B,3] if neither has it.  T <= 8.  The gates are held fixed.  No autograd hookup."""
    xd = x.detach().contiguous()
    idx = _plant_index(other_index, "plant_force_jvp")
    (tx, tw), T, had = _with_t_axis(tangents, (2, 1), "plant_force_jvp")
    stream, default, _ = _enter(engine, xd, weights)
    B = xd.shape[0]
    tx, tw = _cast(tx, torch.float64), _cast(tw, torch.float32)
    f = torch.empty((B, 3), dtype=torch.float64, device=xd.device)
    df = torch.empty((B, T, 3), dtype=torch.float64, device=xd.device)
    engine.plant_force_multi_jvp_device(xd, idx, tx=tx, tw=tw, n_tan=T, df=df, f_check=f, gate=gate, scale=scale, stream=stream)
    if default:
        engine.synchronize()
    return f, df if had else df[:, 0]


# ---------------------------------------------------------------------------------------------- the formation's closed loop, one call per direction
def _configure_formation(engine, index):
    """Configures `index` (a host int32 [B,K] array) on the engine unless it is what is configured (the configuration is synchronous)."""
    have = engine._form_index
    if have is None or have.shape != index.shape or not (have == index).all():
        engine.closed_loop_formation_config(index)


class ClosedLoopFormationFunction(torch.autograd.Function):
    """forward(x0, engine, xr, ur, other_index, f, weights, Qd, Rd, mass, gate, scale, dt, substeps) -> (xs, us, Xs, fps) float64:
    BatchedNMPC.closed_loop_formation_device with its tape; backward: ONE BatchedNMPC.closed_loop_formation_vjp_device call for the
    gradients of x0, xr, ur, f, the weights, Qd, Rd and mass (only those that require one are computed)."""

    @staticmethod
    def forward(ctx, x0, engine, xr, ur, other_index, f, weights, Qd, Rd, mass, gate, scale, dt, substeps):
        x0, xr, ur, fd = _det(x0), _det(xr), _det(ur), _det(f)
        idx = _plant_index(other_index, "ClosedLoopFormationFunction")
        if idx is None:
            raise ValueError("ClosedLoopFormationFunction: other_index is required (closed_loop is the form without neighbours)")
        ctx.model = _install_model(engine, Qd, Rd, mass)
        ctx.set_materialize_grads(False)
        K, B, N = xr.shape[0], xr.shape[1], xr.shape[2] - 1
        stream, default, ctx.key = _enter(engine, x0, weights)
        ctx.index = idx.cpu().numpy()
        _configure_formation(engine, ctx.index)
        new = lambda *s: torch.empty(s, dtype=torch.float64, device=x0.device)  # noqa: E731
        xs, us, Xs, fps, tape = new(K, B, 10), new(K, B, 4), new(K, B, N + 1, 10), new(K, B, 3), engine.closed_loop_tape(K)
        engine.closed_loop_formation_device(x0, xr, ur, xs, us, fps, f=fd, Xs=Xs, tape=tape, gate=gate, plant_scale=scale, dt=dt,
                                            substeps=substeps, stream=stream)
        if default:
            engine.synchronize()
        ctx.engine, ctx.dt, ctx.substeps, ctx.gate, ctx.scale = engine, dt, substeps, gate, scale
        ctx.have_w = weights is not None
        ctx.f_dtype = f.dtype if isinstance(f, torch.Tensor) else None
        ctx.like = tuple(None if not isinstance(t, torch.Tensor) else (t.shape, t.dtype, t.device) for t in (Qd, Rd, mass))
        ctx.save_for_backward(x0, xr, ur, xs, us, fps, tape, *(() if fd is None else (fd,)))
        return xs, us, Xs, fps

    @staticmethod
    def backward(ctx, g_xs, g_us, g_Xs, g_fps):
        x0, xr, ur, xs, us, fps, tape, *rest = ctx.saved_tensors
        fd = rest[0] if rest else None
        eng, need = ctx.engine, ctx.needs_input_grad
        want = (need[0], need[2], need[3], need[5] and fd is not None, need[6] and ctx.have_w,
                any(n and like is not None for n, like in zip(need[7:10], ctx.like)))
        if (g_xs is None and g_us is None and g_Xs is None and g_fps is None) or not any(want):
            return (None,) * 14
        if _engine_model(eng) != ctx.model:
            raise RuntimeError("ClosedLoopFormationFunction: the engine's model (Qd, Rd, mass) was changed between this forward and its "
                               "backward (the backward recomputes every step from the engine's model): run the backward before the next "
                               "forward with other values, or set the model back first")
        _check_installed(eng, ctx.key, "ClosedLoopFormationFunction")
        K, B, N = xr.shape[0], xr.shape[1], xr.shape[2] - 1
        ups = tuple(None if g is None else g.to(torch.float64).contiguous() for g in (g_xs, g_us, g_Xs, g_fps))
        gx0, gxr, gur, gf, gw, gm = (torch.empty(*s, dtype=dt, device=x0.device) if w else None for w, s, dt in zip(
            want, ((B, 10), (K, B, N + 1, 10), (K, B, N, 4), (K, B, N + 1, 3), (_lib.MLP_NPARAM,), (B, 16)),
            (torch.float64,) * 4 + (torch.float32, torch.float64)))
        stream, default = _cuda_stream(x0)
        _configure_formation(eng, ctx.index)             # (another formation may have been configured since the forward)
        eng.closed_loop_formation_vjp_device(x0, xr, ur, xs, us, fps, tape, f=fd, gxs=ups[0], gus=ups[1], gXs=ups[2], gfps=ups[3], gx0=gx0,
                                             gxr=gxr, gur=gur, gf=gf, gw=gw, gmodel=gm, gate=ctx.gate, plant_scale=ctx.scale, dt=ctx.dt,
                                             substeps=ctx.substeps, stream=stream)
        if default:
            eng.synchronize()
        out = [None, None, None]
        if gm is not None:
            # a failed vehicle (NaN in its row) contributes nothing: control_step_tunable's convention
            tot = torch.where(torch.isfinite(gm).all(dim=1, keepdim=True), gm, torch.zeros_like(gm)).sum(dim=0)
            for i, (like, need_i, part) in enumerate(zip(ctx.like, need[7:10], (tot[0:10], tot[10:14], tot[14:15] + tot[15:16]))):
                if like is not None and need_i:
                    out[i] = part.reshape(like[0]).to(device=like[2], dtype=like[1])
        return (gx0, None, gxr, gur, None, None if gf is None else gf.to(ctx.f_dtype), gw, out[0], out[1], out[2], None, None, None, None)


def closed_loop_formation(engine, x0, xr, ur, other_index, f=None, weights=None, Qd=None, Rd=None, mass=None, gate=True, scale=1.0,
                          dt=CP.ts_nmpc, substeps=4):
    """(xs, us, Xs, fps) = closed_loop with the downwash force on the plant made inside the loop from the vehicles' actual states: per tick
    fps[k] [B,3] = plant_force(engine, x_k, other_index, gate, scale) from the states of that tick before any of them moves, the control
    step with xr[k], ur[k] and the given force f[k] the controller sees (None: none), the plant tick with fps[k] held over the tick -- the
    values of the chain plant_force -> control_step_trajectory -> plant_step, bit for bit, in one call.  other_index int32 [B] or [B,K]
    (< 0 or >= B: an empty slot); it is configured on the engine (BatchedNMPC.closed_loop_formation_config: a host copy, synchronous).
    Differentiable in x0, xr, ur, f, `weights` (installed as plant_force installs them; replaced before the backward: RuntimeError) and
    Qd / Rd / mass (as closed_loop); the backward is ONE call that carries the gradients across the vehicles on the device.  Held fixed:
    every tick's linearisation point and final active set, and the r_horiz gates.  `scale` is not differentiated.  Behind a failed vehicle
    (a NaN state) the weights' gradient leaves out every vehicle that hears it through an open slot, which the per-tick chain does not
    (include/ndp_nmpc.h): the two routes' weight gradients differ there, and nowhere else by more than the summation's rounding."""
    return ClosedLoopFormationFunction.apply(x0, engine, xr, ur, other_index, f, weights, Qd, Rd, mass, bool(gate), float(scale), float(dt),
                                             int(substeps))
