"""torch.autograd plumbing around a run on a caller-supplied field: loss.backward() reaches the field.

field_run(field, params, ps) gives the displacements and velocities a field run delivers, as tensors that remember where they came
from: forward is api.generate_field (the records cross the host callback — plumbing, not the measured path), backward is
api.field_vjp, the exact adjoint of the linear map field -> (q, v) (definition: csrc/zd_kernels_field_adj.hip), on the device
cotangents.  Both are HIP kernels of the library; nothing here computes."""
import numpy as np
import torch

from . import api


def _records_params(params):
    """a copy of params that delivers float64 records with nothing else in them"""
    p = type(params).from_buffer_copy(params)
    p.icformat = api.ICFORMATS["RVdoubleZel"]
    p.qdensity = 0
    p.qoneslab = -1
    return p


class _FieldRun(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, params, ps, kind, eig):
        ctx.params, ctx.ps, ctx.kind, ctx.eig = params, ps, kind, eig
        ctx.field_dtype = field.dtype
        rec = api.generate_field(_records_params(params), ps, field.detach().contiguous(), kind=kind, eig=eig)["records"]
        q = torch.from_numpy(np.ascontiguousarray(rec["d"])).to(field.device)
        v = torch.from_numpy(np.ascontiguousarray(rec["v"])).to(field.device)
        return q, v

    @staticmethod
    def backward(ctx, g_q, g_v):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        g_q = None if g_q is None else g_q.to(torch.float64).contiguous()
        g_v = None if g_v is None else g_v.to(torch.float64).contiguous()
        grad = api.field_vjp(ctx.params, ctx.ps, g_q=g_q, g_v=g_v, kind=ctx.kind, eig=ctx.eig)
        return grad.to(ctx.field_dtype), None, None, None, None


def field_run(field, params, ps, kind="density", eig=None):
    """(q, v) of a field run as float64 [n, n, n, 3] tensors on field's device, components in the order of the records' d / v members,
    differentiable with respect to `field` (a float32 or float64 tensor of shape (n, n, n) on the GPU; the gradient comes back in its
    dtype).  params, ps, kind, eig as for api.generate_field."""
    if not isinstance(field, torch.Tensor):
        raise TypeError("field_run: a torch tensor on the GPU expected (got %s)" % type(field).__name__)
    api._field_arg(field.detach().contiguous(), params.ppd, kind)  # shape, dtype and device, before anything runs
    return _FieldRun.apply(field, params, ps, kind, eig)
