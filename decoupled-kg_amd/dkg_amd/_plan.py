"""What the acquisition mirrors share (``pareto``, ``jes``, ``jes_pareto``, ``hvkg``, ``boxes``): the device an entry
runs on, its workspace, the growth of a plan's capacity, the plan's evaluation call and the two autograd routes.

A plan entry pair of include/dkg.h (``dkg_jes_*``, ``dkg_hvkg_*``) evaluates B blocks of ``rows x d`` points each and
writes ``[acq | dacq/dX]``; joint entropy search is the ``rows = 1`` case.
"""

from __future__ import annotations

import ctypes
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from .errors import UnsupportedError
from .gp_state import current_stream_ptr


def hip_device(device, what: str, *tensors) -> torch.device:
    """The device an entry runs on: ``device``, else the first device tensor's, else the current one."""
    if device is None:
        for t in tensors:
            if t.device.type == "cuda":
                return t.device
        return torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise UnsupportedError(f"the {what} kernels run on a ROCm (HIP) device; got " + str(dev))
    return dev


def workspace(nbytes: int, device) -> Tensor:
    """A workspace of ``nbytes`` (a query's 0 outside the limits still gives a pointer: the call reports which)."""
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def grow(B: int, floor: int = 16, cap: Optional[int] = None) -> int:
    """The capacity that holds B: ``floor`` doubled until it does, at most ``cap``."""
    n = floor
    while n < B:
        n *= 2
    return n if cap is None else min(n, cap)


class Plan:
    """The host plan buffer and the workspace of an initialised plan, and its evaluation."""

    def __init__(self, device, plan_bytes: int, workspace_bytes: int, max_B: int):
        self.device = device
        self.max_B = int(max_B)
        self.host = ctypes.create_string_buffer(plan_bytes)
        self.ws = workspace(workspace_bytes, device)

    def _forward(self, fwd, what: str, X: Tensor, width: int, grad: bool, extra: Optional[Tensor]) -> Tensor:
        """``X``: device fp64, B blocks of ``width`` numbers.  -> ``out`` (device; with the gradient
        ``[B * (1 + width)]``: ``out[:B]`` the values, ``out[B:]`` dacq/dX row-major; else ``[B]``); ``extra``: the
        entry's optional diagnostic output."""
        B = X.shape[0]
        X = X.contiguous()
        out = torch.empty(B * (1 + width) if grad else B, dtype=torch.double, device=self.device)
        dacq = out.data_ptr() + 8 * B if grad else 0
        _lib.check(fwd(self.host, _lib.ptr(X), B, _lib.ptr(out), dacq, _lib.ptr(extra),
                       current_stream_ptr(self.device)), what)
        return out


class ForwardFn(torch.autograd.Function):
    """Device points ``[B, rows, d]``; with a gradient the same call also returns dacq(X_b)/dX_b, and backward
    scales it by the incoming gradient (acq(X_b) depends on X_b only: the Jacobian is block diagonal)."""

    @staticmethod
    def forward(ctx, X, acq):
        B = X.shape[0]
        if ctx.needs_input_grad[0]:
            out = acq._plan_for(B, X.shape[1]).forward(X, grad=True)
            ctx.save_for_backward(out[B:].view(X.shape))
            return out[:B]
        return acq._plan_for(B, X.shape[1]).forward(X)

    @staticmethod
    def backward(ctx, grad):
        (dacq,) = ctx.saved_tensors
        return grad.to(dacq)[:, None, None] * dacq, None


class HostForwardFn(torch.autograd.Function):
    """Host points ``[*batch, rows, d]`` (what ``optimize_acqf`` passes): one copy each way, a host backward, and
    the autograd graph is this one node.  The same kernels as ``ForwardFn``, so the same bits."""

    @staticmethod
    def forward(ctx, X, acq):
        if ctx.needs_input_grad[0]:
            val, dacq = acq.value_and_grad_host(X)
            ctx.save_for_backward(dacq)
            ctx.xdtype = X.dtype
            return val.to(X.dtype)
        return acq._values_host(X).to(X.dtype)

    @staticmethod
    def backward(ctx, grad):
        (dacq,) = ctx.saved_tensors  # shaped as X
        out = grad.to(dacq).reshape(grad.shape + (1, 1)) * dacq
        return out.to(ctx.xdtype), None
