"""The batched control step as a differentiable torch layer: u0 = step(x0), backward grad_x0 = K0' grad_u0.

K0 = du0/dx0 is the initial-state sensitivity the step writes beside u0 (BatchedNMPC.enable_sensitivity, ndp_sens_enable): the
derivative of the QP the step solved, with its active set held fixed (exact: the solution is piecewise affine in x0) or, when the
interior-point loop finished it, of its last Newton system.  The linearisation point, xr, ur and the disturbance force are constants
of the layer: the layer raises if any of them requires grad (their sensitivities are not computed -- a silent zero gradient would be
wrong, not approximate).  Instances with a nonzero status have NaN in K0 and therefore in their gradient.

Every forward call IS a control step of the engine: it advances the engine's iterate and kept active sets (its warm start), exactly
as BatchedNMPC.update_device does.  Two forward calls on the same x0 therefore need not return the same u0.
"""
import torch


class ControlStepFunction(torch.autograd.Function):
    """forward(x0, engine, xr, ur, f, other, ego_xy) -> u0 [B,4] float64; backward: grad_x0 = K0' grad_u0 (a batched product on
    x0's device).  x0, xr, ur (and f / other / ego_xy when given) are contiguous float64 CUDA tensors as update_device takes them."""

    @staticmethod
    def forward(ctx, x0, engine, xr, ur, f=None, other=None, ego_xy=None):
        for name, t in (("xr", xr), ("ur", ur), ("f", f), ("other", other), ("ego_xy", ego_xy)):
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise ValueError(f"ControlStepFunction: {name} requires grad, but only the sensitivity with respect to x0 is computed "
                                 "(detach it, or leave it out of the graph)")
        if engine.sensitivity_level < 1:
            raise ValueError("ControlStepFunction: the engine's sensitivities are off (engine.enable_sensitivity(1) first)")
        x0 = x0.detach().contiguous()
        u0 = torch.empty((x0.shape[0], 4), dtype=x0.dtype, device=x0.device)
        stream = torch.cuda.current_stream(x0.device) if x0.is_cuda else None
        engine.update_device(x0, xr, ur, u0, f=f, other=other, ego_xy=ego_xy, stream=stream)
        # (a copy ordered behind the step on the same stream: the engine's buffer is overwritten by its next step)
        K0 = engine.device_sensitivity()[0].clone()
        ctx.save_for_backward(K0)
        return u0

    @staticmethod
    def backward(ctx, grad_u0):
        (K0,) = ctx.saved_tensors
        grad_x0 = torch.bmm(K0.transpose(1, 2), grad_u0.to(K0.dtype).unsqueeze(2)).squeeze(2)
        return grad_x0, None, None, None, None, None, None


def control_step(engine, x0, xr, ur, f=None, other=None, ego_xy=None):
    """u0 = the engine's control step at x0, differentiable with respect to x0 (see ControlStepFunction)."""
    return ControlStepFunction.apply(x0, engine, xr, ur, f, other, ego_xy)


class ControlStep(torch.nn.Module):
    """A thin module around control_step: holds the engine (a BatchedNMPC) and switches its sensitivities on (level 1) if they are
    off.  forward(x0, xr, ur, f=None, other=None, ego_xy=None) -> u0.  Each call advances the engine's warm start."""

    def __init__(self, engine):
        super().__init__()
        self.engine = engine
        if engine.sensitivity_level < 1:
            engine.enable_sensitivity(1)

    def forward(self, x0, xr, ur, f=None, other=None, ego_xy=None):
        return control_step(self.engine, x0, xr, ur, f=f, other=other, ego_xy=ego_xy)
