"""Encoder memory -> every decoder layer's cross-attention K/V in one GEMM.

The decoder layers of a T5 stack all read the same encoder output. Projecting
it layer by layer costs 2*n narrow GEMMs forward, 2*n input-gradient GEMMs
whose bf16 results autograd then adds up, and 2*n split-K weight-gradient
GEMM + reduce pairs. Two ops replace that:

  * project_cross_kv: memory [B,Lk,d] and the layers' k/v weights (the
    parameters themselves, stacked per call) -> kv_all [B,Lk,n*2*d], column
    block 2*i = layer i's K, block 2*i+1 = its V. Backward is ONE batched
    input-gradient GEMM, whose per-block results one kernel sums in the
    order and with the roundings of autograd's accumulation on the
    per-layer route (so d_memory is what that route gives), and ONE
    split-K weight-gradient GEMM; the parameters' gradients are the
    contiguous row slices of its result.
  * cross_attention_kv: attention of q on layer i's two blocks of kv_all,
    taken as strided views. Backward has the kernel write dK/dV into layer
    i's blocks of ONE gradient buffer that all layers of the forward share
    (attn_bwd_mfma's dkv_out mode), so nothing is concatenated or added.

The two ops of one forward share a _KVGradState. The first cross-attention
backward that runs allocates the gradient buffer and returns it as the
gradient of kv_all; the others return None, so autograd accumulates
nothing. The projection's backward runs after all of them (it depends on
every consumer of kv_all), zero-fills the blocks of layers whose backward
did not run, and resets the state. All of this is host-side bookkeeping on
Python values: no device sync, no data-dependent branch, safe under
torch.cuda.graph capture.

kv_all must reach nothing but cross_attention_kv: any other consumer's
gradient would have to be added to the shared buffer, and the projection's
backward raises if what it is handed is not that buffer.

impl="torch" runs both ops in plain PyTorch on any device and dtype (the
autograd plumbing is the same); it is for tests, nothing selects it by
default.
"""

from __future__ import annotations

import os
from typing import Optional, Sequence

import torch
from torch import Tensor

from genrec_amd.ops import eager
from genrec_amd.ops.attention import (
    _ACT_SOFTMAX, _call_seed, _kernel_available, _seed_counter,
)
from genrec_amd.ops.linear import splitk_grad_weight

_ROUTING_KNOBS = ("GENREC_DISABLE_CROSS_KV_FUSE", "GENREC_DISABLE_ATTN",
                  "GENREC_DISABLE_MFMA", "GENREC_FORCE_FLASH")


def _new_grad_buffer(shape, dtype, device) -> Tensor:
    """The shared gradient of kv_all. Every column block is written before
    it is read (by a layer's kernel or by the zero fill), so it starts
    uninitialised."""
    return torch.empty(shape, dtype=dtype, device=device)


class _KVGradState:
    """Host-side state of one forward: which layers took their K/V from
    kv_all, and during backward the shared gradient buffer and the column
    blocks already written into it."""

    def __init__(self, n_blocks: int) -> None:
        self.n_blocks = n_blocks
        self.taken = [False] * (n_blocks // 2)
        self.buf: Optional[Tensor] = None
        self.written = [False] * n_blocks

    def take(self, layer: int) -> None:
        if not 0 <= layer < len(self.taken):
            raise IndexError(f"cross_attention_kv: layer {layer} outside "
                             f"kv_all's {len(self.taken)} layers")
        if self.taken[layer]:
            raise RuntimeError(
                f"cross_attention_kv: layer {layer} read kv_all twice in one "
                "forward; its gradient blocks have one writer")
        self.taken[layer] = True

    def buffer(self, like):
        """(buffer, first): first is True for the call that allocated it,
        which is the one that hands it to autograd."""
        if self.buf is not None:
            return self.buf, False
        self.buf = _new_grad_buffer(like.shape, like.dtype, like.device)
        return self.buf, True

    def finish(self, grad: Tensor) -> None:
        """Called by the projection's backward with the gradient autograd
        handed it: check it is the shared buffer, zero the blocks nobody
        wrote, reset for a further backward through the same graph."""
        buf, written = self.buf, self.written
        self.buf, self.written = None, [False] * self.n_blocks
        if buf is None or grad.data_ptr() != buf.data_ptr() \
                or grad.shape != buf.shape:
            raise RuntimeError(
                "project_cross_kv: kv_all received a gradient that is not "
                "the buffer of cross_attention_kv; kv_all must have no "
                "other consumer")
        if all(written):
            return
        blocks = grad.view(grad.size(0), grad.size(1), self.n_blocks, -1)
        for i, done in enumerate(written):
            if not done:
                blocks[:, :, i].zero_()


class CrossKV:
    """kv_all of one forward with the state its consumers share."""

    def __init__(self, kv_all: Tensor, n_layers: int,
                 state: Optional[_KVGradState], impl: str) -> None:
        self.kv_all = kv_all
        self.n_layers = n_layers
        self.state = state
        self.impl = impl


def _input_grad(d_kv_all: Tensor, w_all: Tensor, n_blocks: int) -> Tensor:
    """d_memory [rows, d] of kv_all = memory @ w_all^T, computed as the
    per-layer route computes it: one product per column block (here the
    batches of ONE strided batched GEMM, each rounded to the working
    dtype), summed in the order autograd accumulates them there — the last
    layer's v first, the first layer's k last — with a rounding after every
    add. On the GPU the sum is one seq_sum_bf16 launch instead of
    n_blocks - 1 tensor adds."""
    w = d_kv_all.size(-1)
    rows, hd = d_kv_all.numel() // w, w // n_blocks
    parts = torch.bmm(d_kv_all.view(rows, n_blocks, hd).transpose(0, 1),
                      w_all.view(n_blocks, hd, -1))        # [n, rows, d]
    if parts.is_cuda and parts.dtype == torch.bfloat16 \
            and parts.size(2) % 4 == 0:
        from genrec_amd import ops

        return ops.ext().seq_sum_bf16(parts.view(n_blocks, -1), True) \
            .view(rows, -1)
    acc = parts[n_blocks - 1]
    for i in range(n_blocks - 2, -1, -1):
        acc = acc + parts[i]
    return acc


class _ProjectKVFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, memory, state, *weights):
        w_all = torch.cat(weights, dim=0)          # [n*2*d, d]
        ctx.save_for_backward(memory, w_all)
        ctx.state = state
        ctx.rows = [w.size(0) for w in weights]
        return memory.matmul(w_all.t())

    @staticmethod
    def backward(ctx, d_kv_all):
        memory, w_all = ctx.saved_tensors
        ctx.state.finish(d_kv_all)
        d_mem = None
        if ctx.needs_input_grad[0]:
            d_mem = _input_grad(d_kv_all, w_all, len(ctx.rows)) \
                .view_as(memory)
        d_ws = [None] * len(ctx.rows)
        if any(ctx.needs_input_grad[2:]):
            dw_all = splitk_grad_weight(
                d_kv_all.reshape(-1, d_kv_all.size(-1)),
                memory.reshape(-1, memory.size(-1)), w_all.dtype)
            # contiguous row slices, one per parameter: autograd takes each
            # as that parameter's .grad without a copy
            parts = dw_all.split(ctx.rows, dim=0)
            d_ws = [p if need else None
                    for p, need in zip(parts, ctx.needs_input_grad[2:])]
        return (d_mem, None, *d_ws)


def _kv_views(kv_all: Tensor, layer: int, n_blocks: int, n_heads: int):
    """[B,H,Lk,D] k and v views of layer `layer`'s two column blocks."""
    b, lk, w = kv_all.shape
    blocks = kv_all.view(b, lk, n_blocks, n_heads, w // (n_blocks * n_heads))
    return (blocks[:, :, 2 * layer].transpose(1, 2),
            blocks[:, :, 2 * layer + 1].transpose(1, 2))


class _CrossAttnKVFn(torch.autograd.Function):
    """MFMA attention of q on two column blocks of kv_all. Forward is
    _FusedAttnFn's on strided views (every offset the kernels form is a
    multiple of 8 elements, as their 16-byte loads need: D % 32 == 0);
    backward writes dK/dV into the shared gradient buffer."""

    @staticmethod
    def forward(ctx, q, kv_all, state, layer, n_heads, key_pad_mask, scale,
                dropout_p, training):
        from genrec_amd import ops

        q = q if q.stride(-1) == 1 else q.contiguous()
        kv_all = kv_all if kv_all.is_contiguous() else kv_all.contiguous()
        k, v = _kv_views(kv_all, layer, state.n_blocks, n_heads)
        seed_dev = None
        seed = 0
        if dropout_p > 0 and training:
            seed = _call_seed()
            seed_dev = _seed_counter(q.device)
        out, probs, dmask = ops.ext().attn_fwd_mfma(
            q, k, v, None, key_pad_mask, None, None,
            scale, False, _ACT_SOFTMAX, dropout_p if training else 0.0, seed,
            seed_dev,
        )
        ctx.save_for_backward(q, kv_all, probs, dmask)
        ctx.state = state
        ctx.meta = (layer, n_heads, scale, dropout_p if training else 0.0,
                    seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        from genrec_amd import ops

        q, kv_all, probs, dmask = ctx.saved_tensors
        layer, n_heads, scale, dropout_p, seed = ctx.meta
        state = ctx.state
        k, v = _kv_views(kv_all, layer, state.n_blocks, n_heads)
        if dout.stride(-1) != 1:
            dout = dout.contiguous()
        args = (dout, q, k, v, probs, dmask, None, scale, _ACT_SOFTMAX,
                dropout_p, seed, False, 0, None, 0, None)
        if not ctx.needs_input_grad[1]:
            dq = ops.ext().attn_bwd_mfma(*args)[0]
            return (dq,) + (None,) * 8
        buf, first = state.buffer(kv_all)
        hd = kv_all.size(2) // state.n_blocks
        dq = ops.ext().attn_bwd_mfma(*args, buf, 2 * layer * hd,
                                     (2 * layer + 1) * hd)[0]
        state.written[2 * layer] = state.written[2 * layer + 1] = True
        return (dq, buf if first else None) + (None,) * 7


class _CrossAttnKVTorchFn(torch.autograd.Function):
    """The same node in plain PyTorch: the forward keeps the eager graph of
    this call on detached inputs, the backward differentiates it and copies
    dK/dV into the shared buffer's blocks."""

    @staticmethod
    def forward(ctx, q, kv_all, state, layer, n_heads, key_pad_mask, scale,
                dropout_p, training):
        with torch.enable_grad():
            qd = q.detach().requires_grad_()
            k, v = _kv_views(kv_all.detach(), layer, state.n_blocks, n_heads)
            kd, vd = k.requires_grad_(), v.requires_grad_()
            out = eager.fused_attention(
                qd, kd, vd, scale=scale, key_pad_mask=key_pad_mask,
                dropout_p=dropout_p, training=training)
        ctx.graph = (qd, kd, vd, out)
        ctx.state = state
        ctx.meta = (layer, n_heads, kv_all.shape, kv_all.dtype, kv_all.device)
        return out.detach()

    @staticmethod
    def backward(ctx, dout):
        qd, kd, vd, out = ctx.graph
        layer, n_heads, shape, dtype, device = ctx.meta
        state = ctx.state
        dq, dk, dv = torch.autograd.grad(out, (qd, kd, vd), dout,
                                         retain_graph=True)
        if not ctx.needs_input_grad[1]:
            return (dq,) + (None,) * 8
        buf, first = state.buffer(_Like(shape, dtype, device))
        bk, bv = _kv_views(buf, layer, state.n_blocks, n_heads)
        bk.copy_(dk)
        bv.copy_(dv)
        state.written[2 * layer] = state.written[2 * layer + 1] = True
        return (dq, buf if first else None) + (None,) * 7


class _Like:
    """shape / dtype / device of a tensor that is not kept"""

    def __init__(self, shape, dtype, device) -> None:
        self.shape, self.dtype, self.device = shape, dtype, device


def _cross_kv_fits(memory: Tensor, tgt: Tensor,
                   k_weights: Sequence[Tensor], v_weights: Sequence[Tensor],
                   biases: Sequence[Optional[Tensor]], n_heads: int,
                   kv_caches) -> bool:
    """the conditions of cross_kv_eligible that do not depend on the device
    or on the environment"""
    if kv_caches is not None or not k_weights \
            or len(k_weights) != len(v_weights):
        return False
    if memory.dim() != 3 or tgt.dim() != 3 or memory.size(0) != tgt.size(0):
        return False
    if any(b is not None for b in biases):
        return False
    shape = k_weights[0].shape
    if len(shape) != 2 or shape[1] != memory.size(2) \
            or shape[0] % n_heads != 0:
        return False
    for w in (*k_weights, *v_weights):
        if w.shape != shape or w.dtype != torch.bfloat16:
            return False
    if memory.dtype != torch.bfloat16 or tgt.dtype != torch.bfloat16:
        return False
    d = shape[0] // n_heads
    if d % 32 != 0 or d > 64:
        return False
    return 1 <= tgt.size(1) <= 64 and 1 <= memory.size(1) <= 64


def _route_enabled() -> bool:
    """none of the knobs that route cross attention elsewhere is set (read
    on every call)"""
    return all(os.environ.get(knob, "0") != "1" for knob in _ROUTING_KNOBS)


def cross_kv_eligible(memory: Tensor, tgt: Tensor,
                      k_weights: Sequence[Tensor],
                      v_weights: Sequence[Tensor],
                      biases: Sequence[Optional[Tensor]], n_heads: int,
                      kv_caches=None) -> bool:
    """True iff a decoder stack may take its cross-attention K/V from
    project_cross_kv: no kv_caches, bf16 on the GPU with the extension, all
    layers' k/v weights one shape and without bias, Lq, Lk and D within the
    MFMA attention kernels' range, and none of the knobs that route
    attention elsewhere (GENREC_DISABLE_CROSS_KV_FUSE=1 is this route's
    own; all are read on every call)."""
    if not _cross_kv_fits(memory, tgt, k_weights, v_weights, biases, n_heads,
                          kv_caches):
        return False
    if not (memory.is_cuda and tgt.is_cuda
            and all(w.is_cuda for w in (*k_weights, *v_weights))):
        return False
    return _route_enabled() and _kernel_available("attn_fwd_mfma", memory)


def project_cross_kv(memory: Tensor, k_weights: Sequence[Tensor],
                     v_weights: Sequence[Tensor],
                     impl: Optional[str] = None) -> CrossKV:
    """memory [B,Lk,d] x the layers' cross-attention k / v weights
    ([d_kv, d] each, no bias) -> CrossKV holding kv_all
    [B, Lk, n_layers*2*d_kv]: layer i's K in column block 2*i, its V in
    block 2*i+1. The caller checks cross_kv_eligible first (impl=None), or
    passes impl="torch" for the plain PyTorch route."""
    if impl not in (None, "torch"):
        raise ValueError(f"project_cross_kv: unknown impl {impl!r}")
    n = len(k_weights)
    weights = [w for pair in zip(k_weights, v_weights) for w in pair]
    if not torch.is_grad_enabled():
        # nothing is recorded: no state to share
        kv_all = memory.matmul(torch.cat(weights, dim=0).t())
        return CrossKV(kv_all, n, _KVGradState(2 * n), impl or "hip")
    state = _KVGradState(2 * n)
    kv_all = _ProjectKVFn.apply(memory, state, *weights)
    return CrossKV(kv_all, n, state, impl or "hip")


def cross_attention_kv(q: Tensor, ckv: CrossKV, layer: int,
                       key_pad_mask: Optional[Tensor], scale: float,
                       dropout_p: float, training: bool) -> Tensor:
    """Cross attention of q [B,H,Lq,D] on layer `layer`'s K/V blocks of
    ckv.kv_all -> [B,H,Lq,D]: scale -> key-padding mask -> softmax ->
    dropout -> @V, what t5_attention computes on the per-layer
    projections."""
    ckv.state.take(layer)
    kp = key_pad_mask.contiguous() if key_pad_mask is not None else None
    fn = _CrossAttnKVTorchFn if ckv.impl == "torch" else _CrossAttnKVFn
    return fn.apply(q, ckv.kv_all, ckv.state, layer, q.size(1), kp, scale,
                    dropout_p, training)
