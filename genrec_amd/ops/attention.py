"""Fused attention dispatch (K1 SASRec, K4 HSTU, K13 T5 — SURVEY.md §2.4).

One generic fused-attention op covers the three attention families of the
model zoo; the CDNA4 kernel (csrc/kernels/attention.hip) is templated on the
score activation (softmax vs SiLU) and fuses the bias adds, the reference's
exact masking semantics, and the PV matmul.

Reference semantics fused here:
  * SASRec (sasrec.py:201-245): scale -> key-mask(-1e9) -> causal(-1e9)
    -> softmax -> POST-softmax query mask -> dropout -> @V
  * T5 (transformer.py:106-159): scale -> +rel-bias -> key-pad-mask(-1e9)
    -> +additive attn mask -> softmax -> dropout -> @V
  * HSTU (hstu.py:232-276): QK^T (no scale) -> +pos bias -> +temporal bias
    -> causal(-1e9) -> key-pad(-1e9) -> SiLU (no softmax!) -> @V
"""

from __future__ import annotations

import os
from typing import Optional

import torch
from torch import Tensor

from genrec_amd.ops import eager

_ACT_SOFTMAX = 0
_ACT_SILU = 1


def _kernel_available(name: str, *tensors: Tensor) -> bool:
    from genrec_amd import ops

    if not ops.use_hip(*tensors):
        return False
    return hasattr(ops.ext(), name)


_seed_counters = {}
_call_salt = [0]


def _seed_counter(device) -> torch.Tensor:
    """Per-device dropout seed counter read by the fused kernels. Under
    hipGraph capture each CALL SITE bakes a distinct python-side salt into
    its seed, and advance_dropout_seeds() — captured ONCE per step by
    GraphedTrainStep — bumps this counter so masks vary across replays.
    (Per-call device increments cost ~40 tiny int-add kernels per TIGER
    step; one per step is enough for uniqueness.)"""
    t = _seed_counters.get(device)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=device)
        _seed_counters[device] = t
    return t


def advance_dropout_seeds(device) -> None:
    """One captured increment per training step (graph runners call this);
    eager paths get fresh python-random seeds per call and don't need it."""
    _seed_counter(device).add_(1)


def _call_seed() -> int:
    """Per-call seed: python-random when eager; a distinct per-call-site
    salt under capture (the capture-time constant differentiates sites,
    the device counter differentiates replays)."""
    _call_salt[0] = (_call_salt[0] + 1) & 0x7FFFFFFF
    if torch.cuda.is_available() and \
            torch.cuda.is_current_stream_capturing():
        return (12345 + _call_salt[0] * 2654435761) & 0x7FFFFFFF
    return int(torch.randint(0, 2**31 - 1, (1,)).item())


class _FusedAttnFn(torch.autograd.Function):
    """Autograd wrapper over the HIP fused-attention fwd/bwd kernels."""

    @staticmethod
    def forward(ctx, q, k, v, bias, key_pad_mask, additive_mask, query_mask,
                scale, causal, act, dropout_p, training):
        from genrec_amd import ops

        use_mfma = (q.dtype == torch.bfloat16 and q.size(3) % 32 == 0
                    and os.environ.get("GENREC_DISABLE_MFMA", "0") != "1")
        if use_mfma:
            # the MFMA kernels are stride-aware: [B,L,H,D] transpose views
            # (the layout GEMM outputs naturally produce) go in directly —
            # no .contiguous() copies on q/k/v, out, or the grads.
            q = q if q.stride(-1) == 1 else q.contiguous()
            k = k if k.stride(-1) == 1 else k.contiguous()
            v = v if v.stride(-1) == 1 else v.contiguous()
        else:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        seed_dev = None
        seed = 0
        if dropout_p > 0 and training:
            seed = _call_seed()
            seed_dev = _seed_counter(q.device)
        fwd = ops.ext().attn_fwd_mfma if use_mfma else ops.ext().attn_fwd
        out, probs, dmask = fwd(
            q, k, v, bias, key_pad_mask, additive_mask, query_mask,
            scale, causal, act, dropout_p if training else 0.0, seed,
            seed_dev,
        )
        ctx.use_mfma = use_mfma
        ctx.save_for_backward(q, k, v, probs, dmask,
                              query_mask if query_mask is not None else torch.empty(0))
        ctx.meta = (scale, causal, act, dropout_p if training else 0.0, seed,
                    bias is not None and bias.requires_grad,
                    bias.dim() if bias is not None else 0,
                    bias.dtype if bias is not None else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        from genrec_amd import ops

        q, k, v, probs, dmask, query_mask = ctx.saved_tensors
        (scale, causal, act, dropout_p, seed, bias_grad, bias_dim,
         bias_dtype) = ctx.meta
        bwd = ops.ext().attn_bwd_mfma if ctx.use_mfma else ops.ext().attn_bwd
        if not (ctx.use_mfma and dout.stride(-1) == 1):
            dout = dout.contiguous()
        dq, dk, dv, dbias = bwd(
            dout, q, k, v, probs, dmask,
            query_mask if query_mask.numel() else None,
            scale, act, dropout_p, seed, bias_grad, bias_dim,
        )
        if bias_grad and dbias.dtype != bias_dtype:
            dbias = dbias.to(bias_dtype)
        return (dq, dk, dv, dbias if bias_grad else None,
                None, None, None, None, None, None, None, None)


def _qkv_views(qkv: Tensor, n_heads: int):
    """[B,H,L,D] q/k/v views of a fused [B,L,3*H*D] projection output: what
    qkv.chunk(3, -1) followed by the head split and transpose gives."""
    b, l, w = qkv.shape
    parts = qkv.view(b, l, 3, n_heads, w // (3 * n_heads))
    return (parts[:, :, 0].transpose(1, 2), parts[:, :, 1].transpose(1, 2),
            parts[:, :, 2].transpose(1, 2))


class _PackedSelfAttnFn(torch.autograd.Function):
    """MFMA self-attention on the fused qkv projection output. Forward is
    _FusedAttnFn's; backward has the kernel write dq/dk/dv straight into
    the column blocks of ONE [B,L,3*H*D] gradient, so the concatenation
    that chunk's backward would launch never runs."""

    @staticmethod
    def forward(ctx, qkv, n_heads, bias, key_pad_mask, additive_mask, scale,
                dropout_p, training):
        from genrec_amd import ops

        qkv = qkv if qkv.is_contiguous() else qkv.contiguous()
        q, k, v = _qkv_views(qkv, n_heads)
        seed_dev = None
        seed = 0
        if dropout_p > 0 and training:
            seed = _call_seed()
            seed_dev = _seed_counter(qkv.device)
        out, probs, dmask = ops.ext().attn_fwd_mfma(
            q, k, v, bias, key_pad_mask, additive_mask, None,
            scale, False, _ACT_SOFTMAX, dropout_p if training else 0.0, seed,
            seed_dev,
        )
        ctx.save_for_backward(qkv, probs, dmask)
        ctx.meta = (n_heads, scale, dropout_p if training else 0.0, seed,
                    bias is not None and bias.requires_grad,
                    bias.dim() if bias is not None else 0,
                    bias.dtype if bias is not None else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        from genrec_amd import ops

        qkv, probs, dmask = ctx.saved_tensors
        (n_heads, scale, dropout_p, seed, bias_grad, bias_dim,
         bias_dtype) = ctx.meta
        q, k, v = _qkv_views(qkv, n_heads)
        if dout.stride(-1) != 1:
            dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        _, _, _, dbias = ops.ext().attn_bwd_mfma(
            dout, q, k, v, probs, dmask, None,
            scale, _ACT_SOFTMAX, dropout_p, seed, bias_grad, bias_dim,
            None, 0, dqkv,
        )
        if bias_grad and dbias.dtype != bias_dtype:
            dbias = dbias.to(bias_dtype)
        return (dqkv, None, dbias if bias_grad else None,
                None, None, None, None, None)


def _packed_qkv_fits(qkv: Tensor, n_heads: int,
                     additive_mask: Optional[Tensor], kv_cache: Optional[dict],
                     table_bias: bool) -> bool:
    """the conditions of packed_qkv_eligible that do not depend on the
    device or on the environment"""
    if kv_cache is not None or table_bias or qkv.dim() != 3:
        return False
    if qkv.dtype != torch.bfloat16 or qkv.size(2) % (3 * n_heads) != 0:
        return False
    d = qkv.size(2) // (3 * n_heads)
    if d % 32 != 0 or d > 64 or qkv.size(1) > 64 or qkv.size(1) < 1:
        return False
    return additive_mask is None or additive_mask.dim() == 2


def packed_qkv_eligible(qkv: Tensor, n_heads: int,
                        additive_mask: Optional[Tensor] = None,
                        kv_cache: Optional[dict] = None,
                        table_bias: bool = False) -> bool:
    """True iff t5_self_attention_packed would run the MFMA kernels on this
    fused [B,L,3*H*D] projection output: no kv_cache, bf16 on the GPU,
    D % 32 == 0, D <= 64, L <= 64, a 2-D additive mask or none, dense bias
    mode, and none of the knobs that route attention elsewhere."""
    if not _packed_qkv_fits(qkv, n_heads, additive_mask, kv_cache,
                            table_bias) or not qkv.is_cuda:
        return False
    for knob in ("GENREC_DISABLE_PACKED_QKV", "GENREC_DISABLE_ATTN",
                 "GENREC_FORCE_FLASH", "GENREC_DISABLE_MFMA"):
        if os.environ.get(knob, "0") == "1":
            return False
    return _kernel_available("attn_fwd_mfma", qkv)


def t5_self_attention_packed(qkv, n_heads, bias, key_pad_mask, additive_mask,
                             scale, dropout_p, training):
    """T5 self-attention on the fused projection output qkv [B,L,3*H*D]
    -> [B,H,L,D]. The caller checks packed_qkv_eligible first. Computes
    what t5_attention computes on the chunked views; the gradient of qkv
    comes back as one tensor."""
    b = bias.contiguous() if bias is not None else None
    kp = key_pad_mask.contiguous() if key_pad_mask is not None else None
    am = additive_mask.contiguous() if additive_mask is not None else None
    return _PackedSelfAttnFn.apply(qkv, n_heads, b, kp, am, scale, dropout_p,
                                   training)


class _FusedAttnTableBiasFn(torch.autograd.Function):
    """MFMA attention with the rel-bias TABLE gathered in-kernel
    (HSTU-style; round 2): no materialized [H,Lq,Lk] bias tensor in
    forward, and backward accumulates table grads via an LDS histogram
    + deterministic colsum instead of the [B,H,Lq,Lk] ds_saved
    round-trip. Caller guarantees the mfma path fits."""

    @staticmethod
    def forward(ctx, q, k, v, bias_table, bias_bucket, key_pad_mask,
                additive_mask, query_mask, scale, causal, dropout_p,
                training):
        from genrec_amd import ops

        q = q if q.stride(-1) == 1 else q.contiguous()
        k = k if k.stride(-1) == 1 else k.contiguous()
        v = v if v.stride(-1) == 1 else v.contiguous()
        table_f = bias_table.float()  # kernel reads fp32
        seed_dev = None
        seed = 0
        if dropout_p > 0 and training:
            seed = _call_seed()
            seed_dev = _seed_counter(q.device)
        out, probs, dmask = ops.ext().attn_fwd_mfma(
            q, k, v, table_f, key_pad_mask, additive_mask, query_mask,
            scale, causal, 0, dropout_p if training else 0.0, seed,
            seed_dev, bias_bucket)
        ctx.save_for_backward(
            q, k, v, probs, dmask,
            query_mask if query_mask is not None else torch.empty(0),
            bias_bucket)
        ctx.meta = (scale, dropout_p if training else 0.0,
                    bias_table.requires_grad,
                    bias_table.numel() // q.size(1), bias_table.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        from genrec_amd import ops

        q, k, v, probs, dmask, query_mask, bucket = ctx.saved_tensors
        scale, dropout_p, bias_grad, n_buckets, tab_dtype = ctx.meta
        if dout.stride(-1) != 1:
            dout = dout.contiguous()
        dq, dk, dv, dtab = ops.ext().attn_bwd_mfma(
            dout, q, k, v, probs, dmask,
            query_mask if query_mask.numel() else None,
            scale, 0, dropout_p, 0, bias_grad, 0, bucket, n_buckets)
        if bias_grad and dtab.dtype != tab_dtype:
            dtab = dtab.to(tab_dtype)
        return (dq, dk, dv, dtab if bias_grad else None, None,
                None, None, None, None, None, None, None)


class _FlashAttnFn(torch.autograd.Function):
    """Flash-tiled attention (Lk/Lq beyond one 64-tile): running-softmax
    forward, single-pass backward via the flash identity (tile math proven
    in tools/sim_flash_tiles.py; GPU-validated round 2 — default for
    Lk>64 softmax attention; GENREC_DISABLE_ATTN_FLASH=1 opts out)."""

    @staticmethod
    def forward(ctx, q, k, v, bias, key_pad_mask, additive_mask, query_mask,
                scale, causal, dropout_p, training):
        from genrec_amd import ops

        # stride-aware: [B,L,H,D] transpose views pass straight through
        # (the host copies only when d isn't innermost / strides are
        # unaligned), killing the q/k/v copy kernels per decoder layer
        seed_dev = None
        seed = 0
        if dropout_p > 0 and training:
            seed = _call_seed()
            seed_dev = _seed_counter(q.device)
        out, s_saved, ml, dmask = ops.ext().attn_fwd_flash(
            q, k, v, bias, key_pad_mask, additive_mask, query_mask,
            scale, causal, dropout_p if training else 0.0, seed, seed_dev)
        ctx.save_for_backward(
            q, k, v, out, s_saved, ml, dmask,
            query_mask if query_mask is not None else torch.empty(0))
        ctx.meta = (scale, dropout_p if training else 0.0,
                    bias is not None and bias.requires_grad,
                    bias.dim() if bias is not None else 0,
                    bias.dtype if bias is not None else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        from genrec_amd import ops

        q, k, v, out, s_saved, ml, dmask, query_mask = ctx.saved_tensors
        scale, dropout_p, bias_grad, bias_dim, bias_dtype = ctx.meta
        dq, dk, dv, dbias = ops.ext().attn_bwd_flash(
            dout, q, k, v, out, s_saved, ml, dmask,
            query_mask if query_mask.numel() else None,
            scale, dropout_p, bias_grad, bias_dim)
        if bias_grad and dbias.dtype != bias_dtype:
            dbias = dbias.to(bias_dtype)
        return (dq, dk, dv, dbias if bias_grad else None,
                None, None, None, None, None, None, None)


def fused_attention(
    q: Tensor,
    k: Tensor,
    v: Tensor,
    *,
    scale: float = 1.0,
    bias: Optional[Tensor] = None,
    bias_table: Optional[Tensor] = None,
    bias_bucket: Optional[Tensor] = None,
    key_pad_mask: Optional[Tensor] = None,
    additive_mask: Optional[Tensor] = None,
    causal: bool = False,
    query_mask: Optional[Tensor] = None,
    score_act: str = "softmax",
    dropout_p: float = 0.0,
    training: bool = False,
) -> Tensor:
    act = _ACT_SOFTMAX if score_act == "softmax" else _ACT_SILU
    fits = (k.size(2) <= 64 and q.size(2) <= 64 and q.size(3) <= 64
            and (additive_mask is None or additive_mask.dim() == 2)
            and os.environ.get("GENREC_DISABLE_ATTN", "0") != "1"
            # experiment knob: route even Lk<=64 through the flash
            # (recompute-P) kernels to trade HBM p_saved traffic for
            # recompute — measured per-config on GPU
            and os.environ.get("GENREC_FORCE_FLASH", "0") != "1")
    if bias_table is not None:
        # rel-bias TABLE mode: gather in-kernel when the mfma path fits
        # (bf16, D % 32 == 0); otherwise materialize the dense bias and
        # fall through to the ordinary paths
        if (fits and act == _ACT_SOFTMAX and q.dtype == torch.bfloat16
                and q.size(3) % 32 == 0
                and os.environ.get("GENREC_DISABLE_MFMA", "0") != "1"
                and _kernel_available("attn_fwd_mfma", q, k, v)):
            kp = key_pad_mask.contiguous() if key_pad_mask is not None \
                else None
            am = additive_mask.contiguous() if additive_mask is not None \
                else None
            qm = query_mask.contiguous() if query_mask is not None else None
            return _FusedAttnTableBiasFn.apply(
                q, k, v, bias_table, bias_bucket.contiguous(), kp, am, qm,
                scale, causal, dropout_p, training)
        h = q.size(1)
        bias = bias_table.view(h, -1)[:, bias_bucket.reshape(-1)] \
            .view(h, bias_bucket.size(0), bias_bucket.size(1))
    if fits and _kernel_available("attn_fwd", q, k, v):
        b = bias.contiguous() if bias is not None else None
        kp = key_pad_mask.contiguous() if key_pad_mask is not None else None
        am = additive_mask.contiguous() if additive_mask is not None else None
        qm = query_mask.contiguous() if query_mask is not None else None
        return _FusedAttnFn.apply(q, k, v, b, kp, am, qm,
                                  scale, causal, act, dropout_p, training)
    flash_ok = (os.environ.get("GENREC_DISABLE_ATTN_FLASH", "0") != "1"
                and act == _ACT_SOFTMAX and q.dtype == torch.bfloat16
                and q.size(3) % 32 == 0 and q.size(3) <= 64
                and (additive_mask is None or additive_mask.dim() == 2)
                and _kernel_available("attn_fwd_flash", q, k, v))
    if flash_ok:
        b = bias.contiguous() if bias is not None else None
        kp = key_pad_mask.contiguous() if key_pad_mask is not None else None
        am = additive_mask.contiguous() if additive_mask is not None else None
        qm = query_mask.contiguous() if query_mask is not None else None
        return _FlashAttnFn.apply(q, k, v, b, kp, am, qm,
                                  scale, causal, dropout_p, training)
    return eager.fused_attention(
        q, k, v, scale=scale, bias=bias, key_pad_mask=key_pad_mask,
        additive_mask=additive_mask, causal=causal, query_mask=query_mask,
        score_act=score_act, dropout_p=dropout_p, training=training,
    )


def sasrec_attention(q, k, v, valid_mask, scale, dropout_p, training):
    """K1: valid_mask [B, L] float (1=valid). Residual stays in the model."""
    key_pad = valid_mask == 0
    return fused_attention(
        q, k, v, scale=scale, key_pad_mask=key_pad, causal=True,
        query_mask=valid_mask, score_act="softmax",
        dropout_p=dropout_p, training=training,
    )


def t5_attention(q, k, v, bias, key_pad_mask, additive_mask, scale,
                 dropout_p, training, bias_table=None, bias_bucket=None):
    """K13: bias [H,Lq,Lk] or None; additive_mask [Lq,Lk] float or None.
    bias_table [H*nb] + bias_bucket [Lq,Lk] select the in-kernel
    rel-bias gather (no materialized bias tensor)."""
    return fused_attention(
        q, k, v, scale=scale, bias=bias, bias_table=bias_table,
        bias_bucket=bias_bucket, key_pad_mask=key_pad_mask,
        additive_mask=additive_mask, score_act="softmax",
        dropout_p=dropout_p, training=training,
    )


def hstu_pointwise_attention(q, k, v, pos_bias, time_bias, key_pad_mask):
    """K4 core: SiLU-score attention with two bias tensors, causal."""
    bias = pos_bias.unsqueeze(0) if pos_bias.dim() == 3 else pos_bias
    if time_bias is not None:
        bias = bias + time_bias
    return fused_attention(
        q, k, v, scale=1.0, bias=bias, key_pad_mask=key_pad_mask,
        causal=True, score_act="silu",
    )


class _HstuAttnFn(torch.autograd.Function):
    """Fully-fused HSTU attention: bias bucketing/gather + SiLU scores +
    table gradients all in-kernel (K4+K5+K6)."""

    @staticmethod
    def forward(ctx, q, k, v, pos_weight, time_weight, pos_bucket,
                timestamps, key_pad):
        from genrec_amd import ops

        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out, s_saved = ops.ext().hstu_attn_fwd(
            q, k, v, pos_bucket,
            pos_weight.contiguous(),
            time_weight.contiguous() if time_weight is not None else None,
            timestamps, key_pad)
        ctx.save_for_backward(q, k, v, s_saved, pos_bucket,
                              timestamps if timestamps is not None
                              else torch.empty(0))
        ctx.n_pos = pos_weight.size(0)
        ctx.n_time = time_weight.size(0) if time_weight is not None else 0
        ctx.dtypes = (pos_weight.dtype,
                      time_weight.dtype if time_weight is not None else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        from genrec_amd import ops

        q, k, v, s_saved, pos_bucket, ts = ctx.saved_tensors
        dq, dk, dv, dpos, dtime = ops.ext().hstu_attn_bwd(
            dout.contiguous(), q, k, v, s_saved, pos_bucket,
            ts if ts.numel() else None, ctx.n_pos, ctx.n_time)
        dpos = dpos.to(ctx.dtypes[0])
        dtime_out = dtime.to(ctx.dtypes[1]) if ctx.n_time else None
        return dq, dk, dv, dpos, dtime_out, None, None, None


def hstu_fused_attention(q, k, v, pos_bucket, pos_weight, time_weight,
                         timestamps, key_pad_mask):
    """Dispatch for the fully-fused HSTU kernel; falls back to the bias-
    tensor composition (hstu_pointwise_attention) off-GPU / odd shapes."""
    from genrec_amd import ops

    fits = (q.dtype == torch.bfloat16 and q.size(2) <= 64
            and q.size(3) % 32 == 0 and q.size(3) <= 64
            and pos_weight.dtype == torch.bfloat16
            and (time_weight is None or time_weight.dtype == torch.bfloat16)
            and os.environ.get("GENREC_DISABLE_MFMA", "0") != "1")
    if fits and _kernel_available("hstu_attn_fwd", q, k, v):
        ts = timestamps.contiguous() if timestamps is not None else None
        kp = key_pad_mask.contiguous() if key_pad_mask is not None else None
        return _HstuAttnFn.apply(q, k, v, pos_weight, time_weight,
                                 pos_bucket.contiguous(), ts, kp)
    return None  # caller composes the bias-tensor path


class _HstuFlashAttnFn(torch.autograd.Function):
    """Tiled HSTU attention (csrc/kernels/hstu_attn_flash.hip): saves only
    its inputs; backward recomputes the scores per tile, so nothing of
    size L x L exists forward or backward."""

    @staticmethod
    def forward(ctx, q, k, v, pos_weight, time_weight, rel_bucket,
                timestamps, key_pad):
        from genrec_amd import ops

        # The kernel reads bf16 tables. Under autocast the parameters are
        # fp32: they are rounded here, as autocast rounds a weight, and
        # their gradients go back in the parameters' dtype.
        pos_w = pos_weight.to(torch.bfloat16).contiguous()
        time_w = time_weight.to(torch.bfloat16).contiguous() \
            if time_weight is not None else None
        # q/k/v go in as they are: the host copies only what its 16-byte
        # loads cannot read. out is a [B,H,L,D] view of [B,L,H,D] memory.
        out = ops.ext().hstu_attn_flash_fwd(q, k, v, rel_bucket, pos_w,
                                            time_w, timestamps, key_pad)
        none = torch.empty(0)
        ctx.save_for_backward(
            q, k, v, rel_bucket, pos_w,
            time_w if time_w is not None else none,
            timestamps if timestamps is not None else none,
            key_pad if key_pad is not None else none)
        ctx.dtypes = (pos_weight.dtype,
                      time_weight.dtype if time_weight is not None else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        from genrec_amd import ops

        q, k, v, rel_bucket, pos_w, time_w, ts, key_pad = ctx.saved_tensors
        use_time = time_w.numel() > 0
        dq, dk, dv, dpos, dtime = ops.ext().hstu_attn_flash_bwd(
            dout, q, k, v, rel_bucket, pos_w,
            time_w if use_time else None, ts if use_time else None,
            key_pad if key_pad.numel() else None)
        dpos = dpos.to(ctx.dtypes[0])
        dtime_out = dtime.to(ctx.dtypes[1]) if use_time else None
        return dq, dk, dv, dpos, dtime_out, None, None, None


# Shortest sequence the tiled kernel takes; up to 64 rows the one-tile
# kernel of hstu_fused_attention runs.
HSTU_FLASH_MIN_L = 65


def hstu_flash_supported(q: Tensor, k: Tensor, v: Tensor, pos_weight: Tensor,
                         time_weight: Optional[Tensor] = None) -> bool:
    """True iff hstu_attention would run the tiled HIP kernel on these
    inputs (everything on the GPU, bf16 q/k/v, bf16 or fp32 tables (fp32
    ones, the parameters of a model under autocast, are rounded to bf16 for
    the kernel), D in {32,64}, L > 64, not disabled)."""
    if os.environ.get("GENREC_DISABLE_HSTU_FLASH", "0") == "1":
        return False
    if not (q.dim() == 4 and k.shape == q.shape and v.shape == q.shape):
        return False
    if not (q.dtype == k.dtype == v.dtype == torch.bfloat16):
        return False
    tables = (pos_weight,) if time_weight is None \
        else (pos_weight, time_weight)
    if any(t.dtype not in (torch.bfloat16, torch.float32) for t in tables):
        return False
    if q.size(3) not in (32, 64) or q.size(2) < HSTU_FLASH_MIN_L \
            or q.size(0) == 0 or q.size(1) == 0:
        return False
    return _kernel_available("hstu_attn_flash_fwd", q, k, v, *tables)


def hstu_attention(
    q: Tensor,  # [B, H, L, D]
    k: Tensor,
    v: Tensor,
    rel_bucket: Tensor,                     # [2L-1] int
    pos_weight: Tensor,                     # [n_pos, H]
    time_weight: Optional[Tensor] = None,   # [n_time, H]
    timestamps: Optional[Tensor] = None,    # [B, L] int
    key_pad_mask: Optional[Tensor] = None,  # [B, L] bool, True = PAD
) -> Tensor:
    """HSTU pointwise attention at any sequence length -> [B, H, L, D].

    QK^T (no scale) + position bias + temporal bias, causal and key-pad
    masks at -1e9, SiLU scores, @ V. The position bucket of (i, j) is
    rel_bucket[j - i + L - 1] (RelativePositionBias.rel_bucket_table); the
    time bias is used when time_weight and timestamps are both given. On the
    GPU, bf16 with D in {32,64} runs the tiled kernel for L > 64 (the result
    is then a view whose transpose(1,2) is contiguous) and the one-tile
    kernel of hstu_fused_attention up to 64; everything else is
    eager.hstu_attention. No [L,L] table is built for L > 64; up to 64 the
    one-tile kernel's [L,L] table is gathered from rel_bucket on every call
    (HSTULayer, which caches its bucket_table, does not come this way).
    rel_bucket, timestamps and key_pad_mask may sit on another device than
    q; they are moved.
    """
    L = q.size(2)
    if time_weight is None or timestamps is None:
        time_weight = timestamps = None
    rel_bucket = rel_bucket.to(q.device)
    if timestamps is not None:
        timestamps = timestamps.to(q.device)
    if key_pad_mask is not None:
        key_pad_mask = key_pad_mask.to(device=q.device, dtype=torch.bool)
    if L < HSTU_FLASH_MIN_L and q.is_cuda:
        pos = torch.arange(L, device=q.device)
        pos_bucket = rel_bucket[pos[None, :] - pos[:, None] + (L - 1)]
        out = hstu_fused_attention(q, k, v, pos_bucket, pos_weight,
                                   time_weight, timestamps, key_pad_mask)
        if out is not None:
            return out
    elif hstu_flash_supported(q, k, v, pos_weight, time_weight):
        ts = timestamps.contiguous() if timestamps is not None else None
        kp = key_pad_mask.contiguous() if key_pad_mask is not None else None
        return _HstuFlashAttnFn.apply(
            q, k, v, pos_weight, time_weight,
            rel_bucket.to(torch.int32).contiguous(), ts, kp)
    return eager.hstu_attention(q, k, v, rel_bucket, pos_weight, time_weight,
                                timestamps, key_pad_mask)


class _GqaFlashAttnFn(torch.autograd.Function):
    """Grouped-query flash attention (csrc/kernels/attention_gqa.hip):
    forward saves only out + lse; backward recomputes S per tile in two
    atomic-free kernels (bitwise run-to-run deterministic)."""

    @staticmethod
    def forward(ctx, q, k, v, key_pad_mask, scale, causal):
        from genrec_amd import ops

        out, lse = ops.ext().gqa_attn_fwd(q, k, v, key_pad_mask, scale,
                                          causal)
        ctx.save_for_backward(
            q, k, v, out, lse,
            key_pad_mask if key_pad_mask is not None else torch.empty(0))
        ctx.meta = (scale, causal)
        return out

    @staticmethod
    def backward(ctx, dout):
        from genrec_amd import ops

        q, k, v, out, lse, key_pad_mask = ctx.saved_tensors
        scale, causal = ctx.meta
        # dq/dk/dv come back as [B,H,L,D] views of [B,L,H,D] storage
        dq, dk, dv = ops.ext().gqa_attn_bwd(
            dout, q, k, v, out, lse,
            key_pad_mask if key_pad_mask.numel() else None, scale, causal)
        return dq, dk, dv, None, None, None


GQA_HEAD_DIMS = (64, 128)


def gqa_kernel_supported(q: Tensor, k: Tensor, v: Tensor) -> bool:
    """True iff gqa_flash_attention would run the HIP kernel on these
    inputs (GPU, bf16, D in {64,128}, Hq % Hkv == 0, not disabled)."""
    if os.environ.get("GENREC_DISABLE_ATTN_GQA", "0") == "1":
        return False
    if not (q.dim() == 4 and k.dim() == 4 and v.dim() == 4):
        return False
    if not (q.dtype == k.dtype == v.dtype == torch.bfloat16):
        return False
    if q.size(3) not in GQA_HEAD_DIMS or k.size(3) != q.size(3) \
            or v.shape != k.shape or k.size(0) != q.size(0):
        return False
    if k.size(1) == 0 or q.size(1) % k.size(1) != 0:
        return False
    if q.size(0) == 0 or q.size(2) == 0 or k.size(2) == 0:
        return False
    return _kernel_available("gqa_attn_fwd", q, k, v)


def gqa_flash_attention(
    q: Tensor,  # [B, Hq, Lq, D]
    k: Tensor,  # [B, Hkv, Lk, D]
    v: Tensor,  # [B, Hkv, Lk, D]
    *,
    key_pad_mask: Optional[Tensor] = None,  # [B, Lk] bool, True = PAD
    scale: float,
    causal: bool = True,
) -> Tensor:
    """Grouped-query causal attention for LLM backbones -> [B, Lq, Hq, D].

    Query head h reads KV head h // (Hq // Hkv); query row i sits at
    absolute position Lk - Lq + i. Exact (-inf) masking; rows with no
    visible key return 0. q/k/v may be [B,L,H,D] transpose views.
    """
    if gqa_kernel_supported(q, k, v):
        kp = None
        if key_pad_mask is not None:
            kp = key_pad_mask.to(torch.bool).contiguous()
        return _GqaFlashAttnFn.apply(q, k, v, kp, float(scale), bool(causal))
    return eager.gqa_attention(q, k, v, key_pad_mask=key_pad_mask,
                               scale=scale, causal=causal)


class _GqaVarlenAttnFn(torch.autograd.Function):
    """Packed-sequence causal GQA attention (the VARLEN instantiations of
    csrc/kernels/attention_gqa.hip). cu_seqlens stays on the device and
    max_seqlen only sizes the grid: no host sync, forward or backward."""

    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens, max_seqlen, scale):
        from genrec_amd import ops

        out, lse = ops.ext().gqa_varlen_fwd(q, k, v, cu_seqlens, max_seqlen,
                                            scale)
        ctx.save_for_backward(q, k, v, out, lse, cu_seqlens)
        ctx.meta = (max_seqlen, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        from genrec_amd import ops

        q, k, v, out, lse, cu_seqlens = ctx.saved_tensors
        max_seqlen, scale = ctx.meta
        dq, dk, dv = ops.ext().gqa_varlen_bwd(dout, q, k, v, out, lse,
                                              cu_seqlens, max_seqlen, scale)
        return dq, dk, dv, None, None, None


def gqa_varlen_supported(q: Tensor, k: Tensor, v: Tensor,
                         cu_seqlens: Tensor) -> bool:
    """True iff gqa_varlen_attention would run the HIP kernel on these
    inputs (GPU, bf16 [T,H,D], D in {64,128}, Hq % Hkv == 0, cu_seqlens on
    the same device, not disabled)."""
    if os.environ.get("GENREC_DISABLE_ATTN_GQA", "0") == "1":
        return False
    if not (q.dim() == 3 and k.dim() == 3 and v.dim() == 3
            and cu_seqlens.dim() == 1 and cu_seqlens.numel() >= 1):
        return False
    if not (q.dtype == k.dtype == v.dtype == torch.bfloat16):
        return False
    if cu_seqlens.is_floating_point() or cu_seqlens.device != q.device:
        return False
    if q.size(2) not in GQA_HEAD_DIMS or k.size(2) != q.size(2) \
            or v.shape != k.shape or k.size(0) != q.size(0):
        return False
    if k.size(1) == 0 or q.size(1) % k.size(1) != 0:
        return False
    return _kernel_available("gqa_varlen_fwd", q, k, v)


def gqa_varlen_attention(
    q: Tensor,  # [T, Hq, D]
    k: Tensor,  # [T, Hkv, D]
    v: Tensor,  # [T, Hkv, D]
    cu_seqlens: Tensor,  # [S+1] int32 on q's device
    max_seqlen: int,
    *,
    scale: float,
) -> Tensor:
    """Causal grouped-query self-attention over S packed sequences
    -> [T, Hq, D] (padding-free training).

    Sequence s owns tokens [cu_seqlens[s], cu_seqlens[s+1]) and attends
    only to itself; tokens beyond cu_seqlens[-1] and empty sequences give
    0 and zero gradients. max_seqlen (a host int, >= the longest sequence)
    only sizes the launch grid and cu_seqlens is never read on the host.
    Per sequence the result is bit-identical to gqa_flash_attention on that
    sequence alone. q/k/v may be column slices of a fused projection.
    """
    if gqa_varlen_supported(q, k, v, cu_seqlens):
        cu = cu_seqlens.to(torch.int32).contiguous()
        return _GqaVarlenAttnFn.apply(q, k, v, cu, int(max_seqlen),
                                      float(scale))
    return eager.gqa_varlen_attention(q, k, v, cu_seqlens, max_seqlen,
                                      scale=scale)


BEAM_MAX_SUFFIX = 16   # suffix slots the decode kernel unrolls over


def beam_decode_supported(q: Tensor, k_pre: Tensor, v_pre: Tensor,
                          k_suf: Tensor, v_suf: Tensor, anc: Tensor) -> bool:
    """True iff beam_decode_attention would run the HIP kernel on these
    inputs (GPU, bf16, D in {64,128}, Hq % Hkv == 0, T <= 16, d innermost
    with 8-element-aligned strides, not disabled)."""
    if os.environ.get("GENREC_DISABLE_ATTN_BEAM", "0") == "1":
        return False
    if not (q.dim() == 4 and k_pre.dim() == 4 and k_suf.dim() == 5
            and anc.dim() == 3 and q.size(2) == 1):
        return False
    if not (q.dtype == k_pre.dtype == v_pre.dtype == k_suf.dtype
            == v_suf.dtype == torch.bfloat16):
        return False
    B, Hkv, Lp, D = k_pre.shape
    if D not in GQA_HEAD_DIMS or q.size(3) != D or v_pre.shape != k_pre.shape:
        return False
    if B == 0 or Lp == 0 or Hkv == 0 or q.size(1) % Hkv != 0 \
            or q.size(0) == 0 or q.size(0) % B != 0:
        return False
    T, W = k_suf.size(1), q.size(0) // B
    if tuple(k_suf.shape) != (B, T, W, Hkv, D) or v_suf.shape != k_suf.shape \
            or tuple(anc.shape) != (B, W, T) or not 1 <= T <= BEAM_MAX_SUFFIX:
        return False
    if not (k_suf.is_contiguous() and v_suf.is_contiguous()):
        return False
    for x, dims in ((q, (0, 1)), (k_pre, (0, 1, 2)), (v_pre, (0, 1, 2))):
        if x.stride(3) != 1 or any(x.stride(d) % 8 for d in dims) \
                or x.data_ptr() % 16:
            return False
    return _kernel_available("beam_attn_fwd", q, k_pre, v_pre, k_suf, v_suf,
                             anc)


def beam_decode_attention(
    q: Tensor,      # [B*W, Hq, 1, D]
    k_pre: Tensor,  # [B, Hkv, Lp, D]   one copy per prompt
    v_pre: Tensor,  # [B, Hkv, Lp, D]
    k_suf: Tensor,  # [B, T, W, Hkv, D] slot s: what beam slot w wrote at step s
    v_suf: Tensor,  # [B, T, W, Hkv, D]
    anc: Tensor,    # [B, W, T] int: slot whose step-s K/V beam w inherits
    t: int,         # suffix slots 0..t-1 are live
    *,
    pre_pad: Optional[Tensor] = None,  # [B, Lp] bool, True = PAD
    scale: float,
    _splits: int = 0,
) -> Tensor:
    """One beam-search decode step over a shared prompt prefix
    -> [B*W, 1, Hq, D] (csrc/kernels/attention_beam.hip).

    Beam (b, w) attends to prompt b's Lp prefix keys and to its own t
    generated tokens, found through anc; no K/V is expanded or reordered.
    Inputs the kernel does not cover materialise the per-beam K/V and go
    through gqa_flash_attention. _splits (tests) fixes the prefix split
    count; 0 picks it from the device's CU count.
    """
    if beam_decode_supported(q, k_pre, v_pre, k_suf, v_suf, anc):
        from genrec_amd import ops

        pad = None
        if pre_pad is not None:
            pad = pre_pad.to(torch.bool).contiguous()
        return ops.ext().beam_attn_fwd(
            q, k_pre, v_pre, pad, k_suf, v_suf,
            anc.to(torch.int32).contiguous(), int(t), float(scale),
            int(_splits))
    if not q.is_cuda:
        return eager.beam_decode_attention(q, k_pre, v_pre, k_suf, v_suf,
                                           anc, t, pre_pad=pre_pad,
                                           scale=scale)
    k, v, key_pad = eager.beam_kv_expand(k_pre, v_pre, k_suf, v_suf, anc, t,
                                         pre_pad)
    return gqa_flash_attention(q, k, v, key_pad_mask=key_pad, scale=scale,
                               causal=True)


def beam_decode_varlen_supported(q: Tensor, k_pre: Tensor, v_pre: Tensor,
                                 cu_seqlens: Tensor, k_suf: Tensor,
                                 v_suf: Tensor, anc: Tensor) -> bool:
    """True iff beam_decode_varlen_attention would run the HIP kernel on
    these inputs (GPU, bf16, k_pre/v_pre [Ttot,Hkv,D] with D in {64,128},
    Hq % Hkv == 0, T <= 16, d innermost with 8-element-aligned strides,
    cu_seqlens an integer [B+1] tensor on the same device, not disabled)."""
    if os.environ.get("GENREC_DISABLE_ATTN_BEAM", "0") == "1":
        return False
    if not (q.dim() == 4 and k_pre.dim() == 3 and k_suf.dim() == 5
            and anc.dim() == 3 and q.size(2) == 1
            and cu_seqlens.dim() == 1 and cu_seqlens.numel() >= 2):
        return False
    if not (q.dtype == k_pre.dtype == v_pre.dtype == k_suf.dtype
            == v_suf.dtype == torch.bfloat16):
        return False
    if cu_seqlens.is_floating_point() or cu_seqlens.dtype == torch.bool \
            or cu_seqlens.device != q.device:
        return False
    B = cu_seqlens.numel() - 1
    _, Hkv, D = k_pre.shape
    if D not in GQA_HEAD_DIMS or q.size(3) != D or v_pre.shape != k_pre.shape:
        return False
    if Hkv == 0 or q.size(1) % Hkv != 0 or q.size(0) == 0 \
            or q.size(0) % B != 0:
        return False
    T, W = k_suf.size(1), q.size(0) // B
    if tuple(k_suf.shape) != (B, T, W, Hkv, D) or v_suf.shape != k_suf.shape \
            or tuple(anc.shape) != (B, W, T) or not 1 <= T <= BEAM_MAX_SUFFIX:
        return False
    if not (k_suf.is_contiguous() and v_suf.is_contiguous()):
        return False
    for x, dims in ((q, (0, 1)), (k_pre, (0, 1)), (v_pre, (0, 1))):
        if x.stride(-1) != 1 or any(x.stride(d) % 8 for d in dims) \
                or x.data_ptr() % 16:
            return False
    return _kernel_available("beam_attn_varlen_fwd", q, k_pre, v_pre, k_suf,
                             v_suf, anc)


def _packed_prefix_to_padded(k_pre: Tensor, v_pre: Tensor, cu_seqlens: Tensor,
                             max_prefix: int):
    """-> (k, v [B,Hkv,Lp,D], pre_pad [B,Lp] bool) with Lp = max_prefix:
    prompt b's tokens first, pads behind them. Device index arithmetic with
    the kernel's clamp of the offsets; cu_seqlens is not read on the host."""
    Ttot = k_pre.size(0)
    Lp = max(int(max_prefix), 1)
    cu = cu_seqlens.to(device=k_pre.device, dtype=torch.long)
    start = cu[:-1].clamp(0, Ttot)
    end = torch.maximum(cu[1:], start).clamp(max=Ttot)
    idx = start[:, None] + torch.arange(Lp, device=k_pre.device)[None, :]
    pad = idx >= end[:, None]
    if Ttot == 0:
        shape = (cu.numel() - 1, k_pre.size(1), Lp, k_pre.size(2))
        return k_pre.new_zeros(shape), v_pre.new_zeros(shape), pad
    idx = idx.clamp(max=Ttot - 1)
    return k_pre[idx].transpose(1, 2), v_pre[idx].transpose(1, 2), pad


def beam_decode_varlen_attention(
    q: Tensor,           # [B*W, Hq, 1, D]
    k_pre: Tensor,       # [Ttot, Hkv, D]   packed prefill, token-major
    v_pre: Tensor,       # [Ttot, Hkv, D]
    cu_seqlens: Tensor,  # [B+1] int32 on q's device
    max_prefix: int,     # host int >= the longest prompt
    k_suf: Tensor,       # [B, T, W, Hkv, D]
    v_suf: Tensor,       # [B, T, W, Hkv, D]
    anc: Tensor,         # [B, W, T] int
    t: int,
    *,
    scale: float,
    _splits: int = 0,
) -> Tensor:
    """beam_decode_attention over the K/V of a packed (padding-free)
    prefill -> [B*W, 1, Hq, D].

    Prompt b owns tokens [cu_seqlens[b], cu_seqlens[b+1]) of k_pre/v_pre,
    clamped into [0, Ttot]; there are no pad keys to mask or to stage. On the
    kernel, max_prefix only picks the split count and cu_seqlens is never
    read on the host; per prompt the result is bit-identical to
    beam_decode_attention on that prompt alone with the same _splits. A
    prompt of length 0 attends to its beams' suffixes only. GPU inputs the
    kernel does not cover are scattered into [B,Hkv,max_prefix,D] plus a
    pad mask on the device and go through beam_decode_attention.
    """
    if beam_decode_varlen_supported(q, k_pre, v_pre, cu_seqlens, k_suf,
                                    v_suf, anc):
        from genrec_amd import ops

        return ops.ext().beam_attn_varlen_fwd(
            q, k_pre, v_pre, cu_seqlens.to(torch.int32).contiguous(),
            int(max_prefix), k_suf, v_suf,
            anc.to(torch.int32).contiguous(), int(t), float(scale),
            int(_splits))
    if not q.is_cuda:
        return eager.beam_decode_varlen_attention(
            q, k_pre, v_pre, cu_seqlens, max_prefix, k_suf, v_suf, anc, t,
            scale=scale)
    k, v, pad = _packed_prefix_to_padded(k_pre, v_pre, cu_seqlens, max_prefix)
    return beam_decode_attention(q, k, v, k_suf, v_suf, anc, t, pre_pad=pad,
                                 scale=scale, _splits=_splits)
