"""LoRA-adapted linear layer as one autograd node:

    lora_linear(x, weight, bias, lora_a, lora_b, scaling, p, training, seed)
        = x W^T + b + scaling * (dropout_p(x) A^T) B^T

The base product stays a hipBLASLt GEMM. On the GPU in bf16 the adapter's
rank-r side runs through the three kernels of csrc/kernels/lora.hip:

    forward    t  = lora_down(x, A)            dropout recomputed from a hash
               y += scaling * t B^T            lora_up_add_, in place
    backward   dt = lora_down(dy, B^T)
               dB = lora_grad(t, dy)^T,  dA = lora_grad(dt, x)
               dx = dy W, then dx += dropout'(dt A)   lora_up_add_, in place

Each reads or updates its big operand once; no dropped copy of x and no
mask is ever stored (the node saves x, t and the seed). The base weight's
and bias's gradients are computed only when they require grad.

Everything else (CPU, fp32, ranks other than 16/32/64, widths that are no
multiple of 8, rows that cannot be viewed with a 16-byte-aligned stride,
GENREC_DISABLE_LORA=1, read per call) runs `eager.lora_linear`: the same
node with torch matmuls and the same rounding points.
"""

from __future__ import annotations

import os
from typing import Optional

import torch
from torch import Tensor

from genrec_amd.ops import eager

LORA_RANKS = (16, 32, 64)


def _rows_or_none(t: Tensor, width: int) -> Optional[Tensor]:
    """t as the kernels take a wide operand: [rows, width] with unit column
    stride, a row stride that is a multiple of 8 and 16-byte alignment,
    without a copy; None when t has no such view."""
    if t.dim() < 1 or t.size(-1) != width:
        return None
    if t.dim() != 2:
        try:
            t = t.view(-1, width)
        except RuntimeError:
            return None
    ok = t.stride(1) == 1 and t.data_ptr() % 16 == 0 and (
        t.size(0) <= 1 or (t.stride(0) >= width and t.stride(0) % 8 == 0))
    return t if ok else None


class _KernelImpl:
    """The csrc/kernels/lora.hip side of eager.LoRALinearFn."""

    @staticmethod
    def lora_rows(t: Tensor, width: int) -> Tensor:
        rows = _rows_or_none(t, width)
        return rows if rows is not None \
            else t.reshape(-1, width).contiguous()

    @staticmethod
    def lora_down(x, p_mat, c, drop_p, seed):
        from genrec_amd import ops

        return ops.ext().lora_down(x, p_mat, c, drop_p, seed)

    @staticmethod
    def lora_up_add_(y, t, q, c, drop_p, seed):
        from genrec_amd import ops

        return ops.ext().lora_up_add_(y, t, q, c, drop_p, seed)

    @staticmethod
    def lora_grad(t, x, c, drop_p, seed):
        from genrec_amd import ops

        return ops.ext().lora_grad(t, x, c, drop_p, seed)


def lora_eligible(x: Tensor, weight: Tensor, bias: Optional[Tensor],
                  lora_a: Tensor, lora_b: Tensor) -> bool:
    """True when lora_linear takes the kernel route for these tensors."""
    from genrec_amd import ops

    if os.environ.get("GENREC_DISABLE_LORA", "0") == "1":
        return False
    tensors = (x, weight, lora_a, lora_b) + (() if bias is None else (bias,))
    if not all(t.is_cuda and t.dtype == torch.bfloat16 for t in tensors):
        return False
    if weight.dim() != 2 or lora_a.dim() != 2 or lora_b.dim() != 2:
        return False
    N, K = weight.shape
    r = lora_a.size(0)
    return (r in LORA_RANKS and K > 0 and N > 0 and K % 8 == 0
            and N % 8 == 0 and tuple(lora_a.shape) == (r, K)
            and tuple(lora_b.shape) == (N, r)
            and lora_a.is_contiguous() and lora_b.is_contiguous()
            and _rows_or_none(x, K) is not None and ops.use_hip(x))


def _autocast_dtype(x: Tensor) -> Optional[torch.dtype]:
    kind = x.device.type
    if torch.is_autocast_enabled(kind):
        return torch.get_autocast_dtype(kind)
    return None


def lora_linear(x: Tensor, weight: Tensor, bias: Optional[Tensor],
                lora_a: Tensor, lora_b: Tensor, scaling: float,
                p: float = 0.0, training: bool = False,
                seed: Optional[int] = None) -> Tensor:
    """x [..., K], weight [N, K], bias [N] | None, lora_a [r, K], lora_b
    [N, r] -> [..., N]. Dropout (on the adapter's input only) is active when
    `training` and p > 0; seed=None then draws one per call from torch's
    CPU generator. Under autocast every operand is cast to the autocast
    dtype with an autograd-tracked `.to`, so fp32 adapters get fp32
    gradients."""
    dtype = _autocast_dtype(x)
    if dtype is not None:
        x, weight, lora_a, lora_b = (t.to(dtype) for t in
                                     (x, weight, lora_a, lora_b))
        bias = None if bias is None else bias.to(dtype)
    if not lora_eligible(x, weight, bias, lora_a, lora_b):
        return eager.lora_linear(x, weight, bias, lora_a, lora_b, scaling,
                                 p, training, seed)
    p = float(p) if training else 0.0
    if p > 0.0 and seed is None:
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
    return eager.LoRALinearFn.apply(x, weight, bias, lora_a, lora_b,
                                    float(scaling), p, int(seed or 0),
                                    _KernelImpl)
