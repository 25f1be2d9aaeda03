"""The non-GEMM, non-attention pieces of a Qwen2 decoder layer:

    add_rms_norm(x, residual, weight, eps) -> (h, n)
    rope_qk(q, k, cos, sin)                -> (q, k)
    swiglu(gate, up)                       -> y

GPU, bf16 and the shapes below: one HIP kernel each way
(csrc/kernels/llm_layer.hip). Everything else, CPU included, runs the
stock transformers op sequence from ops/eager.py, so nothing that works
with the stock layer raises here. GENREC_DISABLE_LLM_LAYER=1 (read per
call) forces the stock sequence.
"""

from __future__ import annotations

import os
from typing import Optional

import torch
from torch import Tensor

from genrec_amd.ops import eager

NORM_MAX_D = 4096
ROPE_HEAD_DIMS = (64, 128)


def _kernels_on(*tensors: Tensor) -> bool:
    from genrec_amd import ops

    if os.environ.get("GENREC_DISABLE_LLM_LAYER", "0") == "1":
        return False
    return all(t.is_cuda and t.dtype == torch.bfloat16 for t in tensors) \
        and ops.use_hip(*tensors)


def _aligned16(t: Tensor) -> bool:
    return t.data_ptr() % 16 == 0


# ------------------------------------------------------------ add + RMSNorm

class _AddRMSNormFn(torch.autograd.Function):
    """residual given: returns (h, n); None: returns n (h is x)."""

    @staticmethod
    def forward(ctx, x: Tensor, residual: Optional[Tensor], weight: Tensor,
                eps: float):
        from genrec_amd import ops

        ctx.set_materialize_grads(False)
        ctx.has_res = residual is not None
        h, n, inv_rms = ops.ext().add_rms_norm_fwd(
            x.contiguous(),
            None if residual is None else residual.contiguous(), weight, eps)
        ctx.save_for_backward(h, weight, inv_rms)
        return (h, n) if ctx.has_res else n

    @staticmethod
    def backward(ctx, *grads):
        from genrec_amd import ops

        dh, dn = grads if ctx.has_res else (None, grads[0])
        if dn is None:
            # the norm output was not used: the add's gradient alone
            return dh, (dh if ctx.has_res else None), None, None
        h, weight, inv_rms = ctx.saved_tensors
        dx, dw = ops.ext().add_rms_norm_bwd(
            dn.contiguous(), None if dh is None else dh.contiguous(), h,
            weight, inv_rms)
        return dx, (dx if ctx.has_res else None), dw, None


def add_rms_norm_eligible(x: Tensor, residual: Optional[Tensor],
                          weight: Tensor) -> bool:
    d = x.shape[-1] if x.dim() else 0
    return (d > 0 and d % 8 == 0 and d <= NORM_MAX_D
            and weight.shape == (d,)
            and (residual is None or residual.shape == x.shape)
            and _kernels_on(x, weight, *(() if residual is None
                                         else (residual,))))


def add_rms_norm(x: Tensor, residual: Optional[Tensor], weight: Tensor,
                 eps: float) -> tuple[Tensor, Tensor]:
    """(h, n): h = x + residual (x itself when residual is None) and
    n = Qwen2RMSNorm(h). Kernel path: bf16 rows and weight on the GPU,
    d % 8 == 0, d <= 4096."""
    if add_rms_norm_eligible(x, residual, weight):
        if residual is None:
            return x, _AddRMSNormFn.apply(x, None, weight, eps)
        return _AddRMSNormFn.apply(x, residual, weight, eps)
    return eager.add_rms_norm(x, residual, weight, eps)


# ---------------------------------------------------------------------- RoPE

class _RopeQKFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, cos: Tensor, sin: Tensor):
        from genrec_amd import ops

        ctx.save_for_backward(cos, sin)
        q_out, k_out = ops.ext().rope_qk_fwd(_rope_view(q), _rope_view(k),
                                             cos, sin, False)
        return q_out, k_out

    @staticmethod
    def backward(ctx, dq: Tensor, dk: Tensor):
        from genrec_amd import ops

        cos, sin = ctx.saved_tensors
        dq, dk = ops.ext().rope_qk_fwd(_rope_view(dq), _rope_view(dk), cos,
                                       sin, True)
        return dq, dk, None, None


def _rope_view(t: Tensor) -> Tensor:
    """t as the kernel takes it: d innermost, every stepped stride a
    multiple of 8 elements, 16-byte aligned; copied only if it is not."""
    ok = t.stride(-1) == 1 and _aligned16(t) and all(
        t.size(i) == 1 or t.stride(i) % 8 == 0 for i in range(3))
    return t if ok else t.contiguous()


def rope_qk_eligible(q: Tensor, k: Tensor, cos: Tensor, sin: Tensor) -> bool:
    if q.dim() != 4 or k.dim() != 4 or cos.dim() != 3 \
            or cos.shape != sin.shape:
        return False
    B, _, L, D = q.shape
    return (D in ROPE_HEAD_DIMS and k.size(0) == B and k.size(2) == L
            and k.size(3) == D and cos.size(0) in (1, B)
            and tuple(cos.shape[1:]) == (L, D)
            and not cos.requires_grad and not sin.requires_grad
            and _kernels_on(q, k, cos, sin))


def rope_qk(q: Tensor, k: Tensor, cos: Tensor,
            sin: Tensor) -> tuple[Tensor, Tensor]:
    """Rotary embedding of q [B,Hq,L,D] and k [B,Hkv,L,D] with cos/sin
    [B|1,L,D] (transformers apply_rotary_pos_emb). Kernel path: bf16 on the
    GPU, D 64 or 128; results come back as [B,H,L,D] transpose views of
    contiguous [B,L,H,D] memory."""
    if rope_qk_eligible(q, k, cos, sin):
        return _RopeQKFn.apply(q, k, cos, sin)
    return eager.rope_qk(q, k, cos, sin)


# -------------------------------------------------------------------- SwiGLU

class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate: Tensor, up: Tensor):
        from genrec_amd import ops

        I = gate.size(-1)
        g2, u2 = _rows_view(gate, I), _rows_view(up, I)
        ctx.save_for_backward(g2, u2)
        ctx.shape = gate.shape
        return ops.ext().swiglu_fwd(g2, u2).view(gate.shape)

    @staticmethod
    def backward(ctx, dy: Tensor):
        from genrec_amd import ops

        g2, u2 = ctx.saved_tensors
        dgate, dup = ops.ext().swiglu_bwd(_rows_view(dy, g2.size(-1)), g2, u2)
        return dgate.view(ctx.shape), dup.view(ctx.shape)


def _rows_view(t: Tensor, I: int) -> Tensor:
    """t as [rows, I] with unit column stride and a row stride that is a
    multiple of 8 (a contiguous tensor, or one half of a [rows, 2I]
    buffer); copied only if it has another layout."""
    if t.dim() != 2:
        # leading dims fold without a copy when they are laid out densely
        try:
            t = t.view(-1, I)
        except RuntimeError:
            t = t.reshape(-1, I)
    ok = t.stride(1) == 1 and _aligned16(t) and (
        t.size(0) == 1 or (t.stride(0) >= I and t.stride(0) % 8 == 0))
    return t if ok else t.contiguous()


def swiglu_eligible(gate: Tensor, up: Tensor) -> bool:
    I = gate.shape[-1] if gate.dim() else 0
    return (gate.dim() >= 1 and gate.shape == up.shape and I > 0
            and I % 8 == 0 and _kernels_on(gate, up))


def swiglu(gate: Tensor, up: Tensor) -> Tensor:
    """silu(gate) * up. Kernel path: bf16 on the GPU, last dim % 8 == 0;
    the backward recomputes from gate and up (no third activation kept)."""
    if swiglu_eligible(gate, up):
        return _SwiGLUFn.apply(gate, up)
    return eager.swiglu(gate, up)
