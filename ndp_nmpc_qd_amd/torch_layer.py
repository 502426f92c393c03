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
        engine.update_device(x0, det(xr), det(ur), u0, f=det(f), other=other, ego_xy=ego_xy, stream=stream)
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


class ControlStep(torch.nn.Module):
    """A thin module around control_step: holds the engine (a BatchedNMPC) and switches its sensitivities on (level 1) if they are
    off; params=True also switches its parameter sensitivities on, so that xr, ur and f may require grad.
    forward(x0, xr, ur, f=None, other=None, ego_xy=None) -> u0.  Each call advances the engine's warm start."""

    def __init__(self, engine, params=False):
        super().__init__()
        self.engine = engine
        if engine.sensitivity_level < 1:
            engine.enable_sensitivity(1)
        if params and not engine.param_sensitivity_enabled:
            engine.enable_param_sensitivity(True)

    def forward(self, x0, xr, ur, f=None, other=None, ego_xy=None):
        return control_step(self.engine, x0, xr, ur, f=f, other=other, ego_xy=ego_xy)
