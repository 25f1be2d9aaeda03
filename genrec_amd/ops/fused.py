"""Fused elementwise ops: residual + dropout(x), dropout(relu(x)), and
residual + dropout(x) followed by the next RMSNorm.

GPU: single HIP kernel each way (masks saved for exact backward). CPU /
no-extension: eager composition with identical semantics.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor


def _seed_args(device, active: bool):
    from genrec_amd.ops.attention import _call_seed, _seed_counter

    if not active:
        return 0, None
    return _call_seed(), _seed_counter(device)


class _DropoutAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, residual: Tensor, p: float):
        from genrec_amd import ops

        seed, seed_dev = _seed_args(x.device, True)
        out, mask = ops.ext().dropout_add_fwd(
            x.contiguous(), residual.contiguous(), p, seed, seed_dev)
        ctx.save_for_backward(mask)
        ctx.p = p
        return out

    @staticmethod
    def backward(ctx, dy: Tensor):
        from genrec_amd import ops

        (mask,) = ctx.saved_tensors
        dx = ops.ext().dropout_fuse_bwd(dy, mask, ctx.p, False)
        return dx, dy, None


class _ReluDropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, p: float):
        from genrec_amd import ops

        seed, seed_dev = _seed_args(x.device, True)
        out, mask = ops.ext().relu_dropout_fwd(x.contiguous(), p, seed,
                                               seed_dev)
        ctx.save_for_backward(mask)
        ctx.p = p
        return out

    @staticmethod
    def backward(ctx, dy: Tensor):
        from genrec_amd import ops

        (mask,) = ctx.saved_tensors
        dx = ops.ext().dropout_fuse_bwd(dy, mask, ctx.p, True)
        return dx, None


class _PlainDropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, p: float):
        from genrec_amd import ops

        seed, seed_dev = _seed_args(x.device, True)
        out, mask = ops.ext().plain_dropout_fwd(x.contiguous(), p, seed,
                                                seed_dev)
        ctx.save_for_backward(mask)
        ctx.p = p
        return out

    @staticmethod
    def backward(ctx, dy: Tensor):
        from genrec_amd import ops

        (mask,) = ctx.saved_tensors
        dx = ops.ext().dropout_fuse_bwd(dy, mask, ctx.p, False)
        return dx, None


def plain_dropout(x: Tensor, p: float, training: bool) -> Tensor:
    """dropout(x, p), hipGraph-replay-safe on GPU (ATen native_dropout
    corrupts on replay, ROCm 7 — see BACKLOG hazard ledger)."""
    from genrec_amd import ops

    if training and p > 0.0 and ops.use_hip(x) \
            and hasattr(ops.ext(), "plain_dropout_fwd"):
        return _PlainDropoutFn.apply(x, p)
    return F.dropout(x, p=p, training=training)


def dropout_add(x: Tensor, residual: Tensor, p: float,
                training: bool) -> Tensor:
    """residual + dropout(x, p) — fused on GPU."""
    from genrec_amd import ops

    if training and p > 0.0 and ops.use_hip(x) \
            and hasattr(ops.ext(), "dropout_add_fwd"):
        return _DropoutAddFn.apply(x, residual, p)
    return residual + F.dropout(x, p=p, training=training)


class _DropoutAddRMSNormFn(torch.autograd.Function):
    """h = residual + dropout(y); n = rms_norm(h) in one kernel each way
    (csrc/kernels/norms.hip). Bit-identical to dropout_add -> rms_norm,
    including the bf16 add autograd inserts for h's two consumers."""

    @staticmethod
    def forward(ctx, y: Tensor, residual: Tensor, weight: Tensor, p: float,
                eps: float, t5_style: bool):
        from genrec_amd import ops

        ctx.set_materialize_grads(False)
        seed, seed_dev = _seed_args(y.device, True)
        h, n, mask, inv_rms = ops.ext().dropout_add_rms_norm_fwd(
            y.contiguous(), residual.contiguous(), weight, p, eps, t5_style,
            seed, seed_dev)
        ctx.save_for_backward(h, weight, inv_rms, mask)
        ctx.p = p
        return h, n

    @staticmethod
    def backward(ctx, dh, dn):
        from genrec_amd import ops

        h, weight, inv_rms, mask = ctx.saved_tensors
        if dn is None:
            # the norm output was not used: plain dropout_add backward
            if dh is None:
                return None, None, None, None, None, None
            dy = ops.ext().dropout_fuse_bwd(dh, mask, ctx.p, False)
            return dy, dh, None, None, None, None
        t, dy, dw = ops.ext().dropout_add_rms_norm_bwd(
            dn.contiguous(), None if dh is None else dh.contiguous(), h,
            weight, inv_rms, mask, ctx.p)
        return dy, t, dw, None, None, None


def _addnorm_eligible(y: Tensor, residual: Tensor, weight: Tensor) -> bool:
    """Inputs the fused kernels take: bf16 rows and bf16 weight (a fp32
    weight promotes the norm output to fp32, which the dword kernels do
    not produce), d even and within the backward's register budget."""
    d = y.shape[-1] if y.dim() else 0
    return (y.dtype == torch.bfloat16 and residual.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16
            and y.shape == residual.shape and weight.shape == (d,)
            and d > 0 and d % 2 == 0 and d <= 1024
            and residual.is_cuda and weight.is_cuda)


def dropout_add_rms_norm(y: Tensor, residual: Tensor, weight: Tensor,
                         p: float, eps: float, t5_style: bool,
                         training: bool) -> tuple[Tensor, Tensor]:
    """(h, n) with h = residual + dropout(y, p) and n = rms_norm(h).

    Fused on GPU for training with p > 0 and eligible inputs; every other
    case composes dropout_add and rms_norm, so inference and decode run
    the code they always ran. GENREC_DISABLE_ADDNORM=1 forces the
    composed path."""
    import os

    from genrec_amd import ops
    from genrec_amd.ops.norms import _hip_ok, rms_norm

    if training and p > 0.0 and _hip_ok(y) \
            and os.environ.get("GENREC_DISABLE_ADDNORM", "0") != "1" \
            and _addnorm_eligible(y, residual, weight) \
            and hasattr(ops.ext(), "dropout_add_rms_norm_fwd"):
        return _DropoutAddRMSNormFn.apply(y, residual, weight, p, eps,
                                          t5_style)
    h = dropout_add(y, residual, p, training)
    return h, rms_norm(h, weight, eps, t5_style)


def relu_dropout(x: Tensor, p: float, training: bool) -> Tensor:
    """dropout(relu(x), p) — fused on GPU."""
    from genrec_amd import ops

    if training and p > 0.0 and ops.use_hip(x) \
            and hasattr(ops.ext(), "relu_dropout_fwd"):
        return _ReluDropoutFn.apply(x, p)
    return F.dropout(F.relu(x), p=p, training=training)
