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
"""
import torch


class ControlStepFunction(torch.autograd.Function):
    """forward(x0, engine, xr, ur, f, other, ego_xy) -> u0 [B,4] float64; backward: grad_x0 = K0' grad_u0 and, when the engine has parameter
    sensitivities on, the gradients of xr, ur and f (batched contractions on x0's device).  x0, xr, ur (and f / other / ego_xy when given)
    are contiguous CUDA tensors as update_device takes them."""

    @staticmethod
    def forward(ctx, x0, engine, xr, ur, f=None, other=None, ego_xy=None):
        params = bool(getattr(engine, "param_sensitivity_enabled", False))
        for name, t in (("xr", xr), ("ur", ur), ("f", f), ("other", other), ("ego_xy", ego_xy)):
            if isinstance(t, torch.Tensor) and t.requires_grad and not (params and name in ("xr", "ur", "f")):
                why = ("the fused downwash network is not differentiated" if name in ("other", "ego_xy") else
                       "the engine's parameter sensitivities are off (engine.enable_param_sensitivity() or ControlStep(engine, params=True))")
                raise ValueError(f"ControlStepFunction: {name} requires grad, but {why} (detach it, or leave it out of the graph)")
        if engine.sensitivity_level < 1:
            raise ValueError("ControlStepFunction: the engine's sensitivities are off (engine.enable_sensitivity(1) first)")
        x0 = x0.detach().contiguous()
        det = lambda t: t.detach() if isinstance(t, torch.Tensor) else t  # noqa: E731
        u0 = torch.empty((x0.shape[0], 4), dtype=x0.dtype, device=x0.device)
        stream = torch.cuda.current_stream(x0.device) if x0.is_cuda else None
        # torch's default stream cannot be named through the C-ABI (a NULL stream is the engine's own): there the step runs on the
        # engine's stream, so the inputs are waited for in front of it and the step behind it
        default = stream is not None and stream.cuda_stream == 0
        if default:
            stream.synchronize()
        engine.update_device(x0, det(xr), det(ur), u0, f=det(f), other=other, ego_xy=ego_xy, stream=stream)
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
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise ValueError(f"ControlStepTrajectoryFunction: {name} requires grad, but the fused downwash network is not differentiated "
                                 "(detach it, or leave it out of the graph)")
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t  # noqa: E731
        x0, xr, ur, fd = det(x0), det(xr), det(ur), det(f)
        stream = torch.cuda.current_stream(x0.device)
        tape = engine.record_tape(stream)
        u0 = torch.empty((x0.shape[0], 4), dtype=x0.dtype, device=x0.device)
        engine.update_device(x0, xr, ur, u0, f=fd, other=other, ego_xy=ego_xy, stream=stream)
        if stream.cuda_stream == 0:        # torch's default stream: the step went on the engine's own (the C-ABI's NULL)
            engine.synchronize()
        X, U = (t.clone() for t in engine.device_iterate())      # (ordered behind the step: the next step overwrites them)
        force = engine.device_force().clone() if other is not None else fd
        ctx.engine = engine
        ctx.f_dtype = f.dtype if isinstance(f, torch.Tensor) else None
        ctx.save_for_backward(x0, xr, ur, force, *tape)
        return u0, X, U

    @staticmethod
    def backward(ctx, g_u0, g_X, g_U):
        x0, xr, ur, force, *tape = ctx.saved_tensors
        eng = ctx.engine
        c = lambda g: None if g is None else g.to(torch.float64).contiguous()  # noqa: E731
        g_u0, g_X, g_U = c(g_u0), c(g_X), c(g_U)
        if g_u0 is None and g_X is None and g_U is None:
            return (None,) * 7
        z = lambda *s: torch.empty(*s, dtype=torch.float64, device=x0.device)  # noqa: E731
        B, N = x0.shape[0], xr.shape[1] - 1
        need = ctx.needs_input_grad
        gx0 = z(B, 10) if need[0] else None
        gxr = z(B, N + 1, 10) if need[2] else None
        gur = z(B, N, 4) if need[3] else None
        gf = z(B, N + 1, 3) if need[4] and ctx.f_dtype is not None else None
        stream = torch.cuda.current_stream(x0.device)
        eng.step_vjp_device(x0, xr, ur, tape, gu0=g_u0, gX=g_X, gU=g_U, f=force, gx0=gx0, gxr=gxr, gur=gur, gf=gf, stream=stream)
        if stream.cuda_stream == 0:
            eng.synchronize()
        return (gx0, None, gxr, gur, None if gf is None else gf.to(ctx.f_dtype), None, None)


def control_step_trajectory(engine, x0, xr, ur, f=None, other=None, ego_xy=None):
    """(u0, X, U) = the engine's control step at x0 and its new iterate (the predicted trajectory), differentiable with respect to x0, xr,
    ur and f through the adjoint of the step (see ControlStepTrajectoryFunction); needs no sensitivities on."""
    return ControlStepTrajectoryFunction.apply(x0, engine, xr, ur, f, other, ego_xy)


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
