"""Eager (plain PyTorch) reference implementations of every fused op.

These are the CPU execution path AND the numerics reference that the CDNA4
HIP kernels are tested against (tests/test_kernels_*.py). Semantics mirror
the reference implementations exactly; citations per function.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor
import torch.nn.functional as F

NEG_BIG = -1e9  # reference's mask value (sasrec.py:220, transformer.py:144)


def rms_norm(x: Tensor, weight: Tensor, eps: float, t5_style: bool) -> Tensor:
    if t5_style:
        # ref normalize.py:73-95 (RootMeanSquareLayerNorm)
        var = x.float().pow(2).mean(-1, keepdim=True)
        y = x * torch.rsqrt(var + eps)
        if weight.dtype in (torch.float16, torch.bfloat16):
            y = y.to(weight.dtype)
        return weight * y
    # ref normalize.py:38-55 (RMSNorm)
    xf = x.float()
    y = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype)
    return y * weight


def l2norm(x: Tensor, eps: float = 1e-12) -> Tensor:
    # ref normalize.py:11-16 — F.normalize semantics: x / max(||x||, eps)
    return F.normalize(x, p=2, dim=-1, eps=eps)


def swish_layer_norm(x: Tensor, weight: Tensor, bias: Tensor, eps: float) -> Tensor:
    # ref normalize.py:58-70
    return F.silu(F.layer_norm(x, x.shape[-1:], weight, bias, eps))


def fused_attention(
    q: Tensor,  # [B, H, Lq, D]
    k: Tensor,  # [B, H, Lk, D]
    v: Tensor,  # [B, H, Lk, D]
    *,
    scale: float = 1.0,
    bias: Optional[Tensor] = None,          # [H,Lq,Lk] or [B,H,Lq,Lk], added pre-mask
    key_pad_mask: Optional[Tensor] = None,  # [B, Lk] bool, True = PAD
    additive_mask: Optional[Tensor] = None,  # [Lq,Lk] float additive (-inf style)
    causal: bool = False,
    query_mask: Optional[Tensor] = None,    # [B, Lq] float, applied AFTER softmax
    score_act: str = "softmax",             # "softmax" (std) or "silu" (HSTU)
    dropout_p: float = 0.0,
    training: bool = False,
) -> Tensor:
    Lq, Lk = q.size(-2), k.size(-2)
    scores = torch.matmul(q, k.transpose(-2, -1))
    if scale != 1.0:
        scores = scores * scale
    if bias is not None:
        scores = scores + (bias if bias.dim() == 4 else bias.unsqueeze(0))
    if causal:
        cm = torch.triu(
            torch.ones(Lq, Lk, device=q.device, dtype=torch.bool), diagonal=1
        )
        scores = scores.masked_fill(cm, NEG_BIG)
    if key_pad_mask is not None:
        scores = scores.masked_fill(key_pad_mask[:, None, None, :], NEG_BIG)
    if additive_mask is not None:
        am = additive_mask
        while am.dim() < 4:
            am = am.unsqueeze(0)
        scores = scores + am.to(scores.dtype)
    if score_act == "softmax":
        attn = torch.softmax(scores, dim=-1)
    elif score_act == "silu":
        attn = F.silu(scores)
    else:
        raise ValueError(score_act)
    if query_mask is not None:
        attn = attn * query_mask[:, None, :, None]
    if dropout_p > 0.0 and training:
        if attn.is_cuda:  # replay-safe on GPU (ATen dropout corrupts
            from genrec_amd.ops.fused import plain_dropout  # in replay)

            attn = plain_dropout(attn, dropout_p, True)
        else:
            attn = F.dropout(attn, p=dropout_p, training=True)
    return torch.matmul(attn, v)


def _hstu_rows(qb: Tensor, kf: Tensor, vf: Tensor, rel_bucket: Tensor,
               pos_w: Tensor, time_w: Optional[Tensor],
               ts_rows: Optional[Tensor], ts: Optional[Tensor],
               key_pad_mask: Optional[Tensor], i0: int) -> Tensor:
    """query rows i0.. of hstu_attention: qb [B,H,n,D] against every key"""
    n, L = qb.size(2), kf.size(2)
    i = torch.arange(i0, i0 + n, device=qb.device)[:, None]
    j = torch.arange(L, device=qb.device)[None, :]
    scores = torch.matmul(qb, kf.transpose(-2, -1))
    # The gathers go through fp64 (exact on fp32 values) so that autograd
    # sums the B*n*L gradient terms of a bucket in fp64: this op is the
    # oracle of the table gradients, and an fp32 running sum of that length
    # is off by more than its last digits.
    bucket = rel_bucket.long()[j - i + (L - 1)]            # [n, L]
    scores = scores + pos_w.double()[bucket].float().permute(2, 0, 1) \
        .unsqueeze(0)
    if time_w is not None:
        diff = ts_rows.unsqueeze(2) - ts.unsqueeze(1)      # [B, n, L]
        tb = (torch.log(diff.abs().clamp(min=1).float()) / 0.693).long() \
            .clamp(min=0, max=time_w.size(0) - 1)
        scores = scores + time_w.double()[tb].float().permute(0, 3, 1, 2)
    scores = scores.masked_fill(j > i, NEG_BIG)
    if key_pad_mask is not None:
        scores = scores.masked_fill(key_pad_mask[:, None, None, :], NEG_BIG)
    return torch.matmul(F.silu(scores), vf)


def hstu_attention(
    q: Tensor,  # [B, H, L, D]
    k: Tensor,
    v: Tensor,
    rel_bucket: Tensor,                     # [2L-1] int: bucket of j - i + L - 1
    pos_weight: Tensor,                     # [n_pos, H]
    time_weight: Optional[Tensor] = None,   # [n_time, H]
    timestamps: Optional[Tensor] = None,    # [B, L] int
    key_pad_mask: Optional[Tensor] = None,  # [B, L] bool, True = PAD
    *,
    block: int = 128,
) -> Tensor:
    """HSTU pointwise attention, fp32 math -> [B, H, L, D] in q's dtype.

    What hstu_pointwise_attention computes on the materialised biases
    (ref hstu.py:232-276): QK^T (no scale) + position bias + temporal bias,
    causal and key-pad masks at -1e9, SiLU, @ V; the position bucket of
    (i, j) is rel_bucket[j - i + L - 1] and the time bucket the ln2 bucket
    of |ts_i - ts_j|. Computed `block` query rows at a time, each block
    recomputed in backward, so no [B,H,L,L] tensor exists: peak memory is
    O(B*H*block*L) with or without autograd.
    """
    from torch.utils.checkpoint import checkpoint

    L = q.size(2)
    if rel_bucket.numel() != 2 * L - 1:
        raise ValueError(f"rel_bucket has {rel_bucket.numel()} entries, "
                         f"needs 2L-1 = {2 * L - 1}")
    use_time = time_weight is not None and timestamps is not None
    qf, kf, vf = q.float(), k.float(), v.float()
    pos_w = pos_weight.float()
    time_w = time_weight.float() if use_time else None
    ts = timestamps if use_time else None
    recompute = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad
        for t in (q, k, v, pos_weight, time_weight))
    outs = []
    for i0 in range(0, L, block):
        args = (qf[:, :, i0:i0 + block], kf, vf, rel_bucket, pos_w, time_w,
                ts[:, i0:i0 + block] if use_time else None, ts, key_pad_mask,
                i0)
        if recompute:
            outs.append(checkpoint(_hstu_rows, *args, use_reentrant=False))
        else:
            outs.append(_hstu_rows(*args))
    return torch.cat(outs, dim=2).to(q.dtype)


def gqa_attention(
    q: Tensor,  # [B, Hq, Lq, D]
    k: Tensor,  # [B, Hkv, Lk, D]
    v: Tensor,  # [B, Hkv, Lk, D]
    *,
    key_pad_mask: Optional[Tensor] = None,  # [B, Lk] bool, True = PAD
    scale: float,
    causal: bool = True,
) -> Tensor:
    """Grouped-query softmax attention, fp32 math -> [B, Lq, Hq, D].

    Query head h reads KV head h // (Hq // Hkv) (no K/V expansion). Query
    row i sits at absolute position Lk - Lq + i and, when causal, sees keys
    j <= Lk - Lq + i (prefill, cached decode and chunked decode). Masking
    is exact (-inf); a row with no visible key returns 0 and has zero
    gradients.
    """
    B, Hq, Lq, D = q.shape
    Hkv, Lk = k.size(1), k.size(2)
    if Hq % Hkv != 0:
        raise ValueError(f"Hq={Hq} is not a multiple of Hkv={Hkv}")
    g = Hq // Hkv
    qf = q.float().reshape(B, Hkv, g, Lq, D)
    kf, vf = k.float(), v.float()
    scores = torch.einsum("bkgqd,bkld->bkgql", qf, kf) * scale
    visible = torch.ones(B, 1, 1, Lq, Lk, dtype=torch.bool, device=q.device)
    if causal:
        i = torch.arange(Lq, device=q.device)[:, None] + (Lk - Lq)
        j = torch.arange(Lk, device=q.device)[None, :]
        visible = visible & (j <= i)
    if key_pad_mask is not None:
        visible = visible & ~key_pad_mask.bool()[:, None, None, None, :]
    any_visible = visible.any(dim=-1, keepdim=True)
    scores = scores.masked_fill(~visible, float("-inf"))
    # rows with no visible key: softmax over zeros, then zeroed (no NaN)
    scores = torch.where(any_visible, scores, torch.zeros_like(scores))
    probs = torch.softmax(scores, dim=-1)
    probs = torch.where(any_visible, probs, torch.zeros_like(probs))
    out = torch.einsum("bkgql,bkld->bkgqd", probs, vf)
    out = out.reshape(B, Hq, Lq, D).transpose(1, 2).contiguous()
    return out.to(q.dtype)


def gqa_varlen_attention(
    q: Tensor,  # [T, Hq, D]
    k: Tensor,  # [T, Hkv, D]
    v: Tensor,  # [T, Hkv, D]
    cu_seqlens: Tensor,  # [S+1] int, sequence s = tokens [cu[s], cu[s+1])
    max_seqlen: int = 0,  # unused: the mask is built from cu_seqlens
    *,
    scale: float,
) -> Tensor:
    """Causal grouped-query attention over packed sequences, fp32 math
    -> [T, Hq, D].

    Token i sees the tokens j <= i of its own sequence (a block-diagonal
    causal mask built from cu_seqlens on the device, no host sync). Tokens
    of no sequence (beyond cu[S], before cu[0]) and so empty sequences
    return 0 and have zero gradients.
    """
    T, Hq, D = q.shape
    Hkv = k.size(1)
    if Hq % Hkv != 0:
        raise ValueError(f"Hq={Hq} is not a multiple of Hkv={Hkv}")
    g = Hq // Hkv
    cu = cu_seqlens.to(device=q.device, dtype=torch.long)
    tok = torch.arange(T, device=q.device)
    # sequence of token t: how many sequence ends are <= t
    seg = torch.bucketize(tok, cu[1:].contiguous(), right=True)
    live = (seg < cu.numel() - 1) & (tok >= cu[0])
    visible = (seg[:, None] == seg[None, :]) & (tok[None, :] <= tok[:, None]) \
        & live[:, None] & live[None, :]
    qf = q.float().reshape(T, Hkv, g, D)
    kf, vf = k.float(), v.float()
    scores = torch.einsum("qkgd,lkd->kgql", qf, kf) * scale
    any_visible = live[:, None]                      # the diagonal
    scores = scores.masked_fill(~visible, float("-inf"))
    scores = torch.where(any_visible, scores, torch.zeros_like(scores))
    probs = torch.softmax(scores, dim=-1)
    probs = torch.where(any_visible, probs, torch.zeros_like(probs))
    out = torch.einsum("kgql,lkd->qkgd", probs, vf)
    return out.reshape(T, Hq, D).contiguous().to(q.dtype)


def beam_kv_expand(k_pre: Tensor, v_pre: Tensor, k_suf: Tensor,
                   v_suf: Tensor, anc: Tensor, t: int,
                   pre_pad: Optional[Tensor] = None):
    """Per-beam K/V of a shared-prefix beam cache, materialised.

    -> (k, v [B*W, Hkv, Lp+t, D], key_pad [B*W, Lp+t] bool | None): beam
    (b, w) gets prompt b's prefix followed by k_suf[b, s, anc[b,w,s]] for
    s < t. Slots s >= t of k_suf/v_suf/anc are never read.
    """
    B, T, W, Hkv, D = k_suf.shape
    idx = anc[:, :, :t].long()[..., None, None].expand(B, W, t, Hkv, D)

    def one(pre, suf):
        # [B,T,W,Hkv,D] -> [B,slot,t,Hkv,D], pick slot anc[b,w,s] per (w,s)
        own = suf[:, :t].permute(0, 2, 1, 3, 4).gather(1, idx)
        own = own.reshape(B * W, t, Hkv, D).transpose(1, 2)
        return torch.cat([pre.repeat_interleave(W, dim=0), own], dim=2)

    key_pad = None
    if pre_pad is not None:
        key_pad = F.pad(pre_pad.bool().repeat_interleave(W, dim=0), (0, t),
                        value=False)
    return one(k_pre, k_suf), one(v_pre, v_suf), key_pad


def beam_decode_attention(
    q: Tensor,      # [B*W, Hq, 1, D]
    k_pre: Tensor,  # [B, Hkv, Lp, D]
    v_pre: Tensor,  # [B, Hkv, Lp, D]
    k_suf: Tensor,  # [B, T, W, Hkv, D]
    v_suf: Tensor,  # [B, T, W, Hkv, D]
    anc: Tensor,    # [B, W, T] int
    t: int,
    *,
    pre_pad: Optional[Tensor] = None,  # [B, Lp] bool, True = PAD
    scale: float,
) -> Tensor:
    """One beam-search decode step over a shared prompt prefix, fp32 math
    -> [B*W, 1, Hq, D]: each beam's suffix is gathered through anc, appended
    to its prompt's prefix, and attended with gqa_attention (Lq = 1)."""
    k, v, key_pad = beam_kv_expand(k_pre, v_pre, k_suf, v_suf, anc, t,
                                   pre_pad)
    return gqa_attention(q, k, v, key_pad_mask=key_pad, scale=scale,
                         causal=True)


def beam_decode_varlen_attention(
    q: Tensor,           # [B*W, Hq, 1, D]
    k_pre: Tensor,       # [Ttot, Hkv, D] packed prefill, token-major
    v_pre: Tensor,       # [Ttot, Hkv, D]
    cu_seqlens: Tensor,  # [B+1] int, prompt b = tokens [cu[b], cu[b+1])
    max_prefix: int,     # unused: the lengths are read from cu_seqlens
    k_suf: Tensor,       # [B, T, W, Hkv, D]
    v_suf: Tensor,       # [B, T, W, Hkv, D]
    anc: Tensor,         # [B, W, T] int
    t: int,
    *,
    scale: float,
) -> Tensor:
    """beam_decode_attention over a packed prefill, fp32 math
    -> [B*W, 1, Hq, D]: a per-prompt loop over slices of the packed K/V
    (reads cu_seqlens on the host). Offsets are clamped to [0, Ttot] and to
    end >= start as the kernel clamps them; an empty prompt's beams attend
    to their suffix only."""
    B = cu_seqlens.numel() - 1
    W = q.size(0) // B
    Ttot = k_pre.size(0)
    cu = cu_seqlens.tolist()
    outs = []
    for b in range(B):
        s = min(max(int(cu[b]), 0), Ttot)
        e = min(max(int(cu[b + 1]), s), Ttot)
        outs.append(beam_decode_attention(
            q[b * W:(b + 1) * W],
            k_pre[s:e].transpose(0, 1).unsqueeze(0),
            v_pre[s:e].transpose(0, 1).unsqueeze(0),
            k_suf[b:b + 1], v_suf[b:b + 1], anc[b:b + 1], t, scale=scale))
    return torch.cat(outs, dim=0)


def pairwise_sqdist(x: Tensor, codebook: Tensor) -> Tensor:
    """L2 distance matrix ||x||^2 + ||c||^2 - 2 x c^T (ref rqvae.py:186-192)."""
    return (
        (x ** 2).sum(dim=1, keepdim=True)
        + (codebook.T ** 2).sum(dim=0, keepdim=True)
        - 2 * x @ codebook.T
    )


def tied_softmax_ce(
    hidden: Tensor,      # [N, D] flattened
    emb_weight: Tensor,  # [V, D]
    targets: Tensor,     # [N]
    ignore_index: int = 0,
) -> Tensor:
    """logits = h @ E^T then mean-CE with ignore_index (ref sasrec.py:121-128)."""
    logits = hidden @ emb_weight.t()
    return F.cross_entropy(logits, targets, ignore_index=ignore_index)


def summed_ce(logits: Tensor, targets: Tensor) -> Tensor:
    """Per-sequence summed CE then batch mean (ref tiger.py:232-240)."""
    B = logits.size(0)
    loss = F.cross_entropy(
        logits.reshape(-1, logits.size(-1)), targets.reshape(-1), reduction="none"
    ).reshape(B, -1)
    return loss.sum(dim=1).mean()


def topk_hit_ranks(actual: Tensor, top_k: Tensor) -> Tensor:
    """Rank (0-based) of the first exact match of `actual` in `top_k`.

    Args:
        actual: [B, D] ground-truth id tuples
        top_k:  [B, K, D] ranked predictions
    Returns:
        [B] int64 ranks; K when no match. (ref metrics.py:26-66)
    """
    K = top_k.size(1)
    matches = (actual.unsqueeze(1) == top_k).all(dim=-1)  # [B, K]
    found = matches.any(dim=1)
    first = matches.float().argmax(dim=1)
    return torch.where(found, first, torch.full_like(first, K))


# ------------------------------------------------- linear + cross-entropy
#
# loss = CE(hidden @ weight^T, targets) without ever holding [N, V]: the
# supervised rows are gathered, the logits are formed a chunk of rows at a
# time, each chunk is turned into its own gradient in place, and the two
# gradient GEMMs run before the next chunk reuses the buffer. The loop below
# is shared by the HIP op (ops/losses.py passes the kernel pair as
# `chunk_fn`) and by the plain-PyTorch path, which is its CPU reference.

LCE_CHUNK_ELEMS = 1 << 29   # logits elements per chunk (docs/kernels.md)


def lce_default_chunk_rows(n_rows: int, vocab: int) -> int:
    return max(1, min(max(n_rows, 1), LCE_CHUNK_ELEMS // max(vocab, 1)))


def _lce_acc_dtype(dtype: torch.dtype) -> torch.dtype:
    return torch.float64 if dtype == torch.float64 else torch.float32


def lce_chunk_inplace(logits: Tensor, targets: Tensor, inv_n: Tensor,
                      ignore_index: int, slices: int = 0):
    """Plain-PyTorch twin of the lce_stats / lce_grad kernels: overwrite
    logits[R, V] with inv_n * (softmax - onehot) (zeros for ignored rows)
    and return (row_loss[R], lse[R])."""
    V = logits.size(1)
    x = logits.to(_lce_acc_dtype(logits.dtype))
    lse = torch.logsumexp(x, dim=1)
    ok = (targets != ignore_index) & (targets >= 0) & (targets < V)
    t = torch.where(ok, targets, torch.zeros_like(targets)).unsqueeze(1)
    row_loss = torch.where(ok, lse - x.gather(1, t).squeeze(1),
                           torch.zeros_like(lse))
    d = torch.exp(x - lse.unsqueeze(1))
    d.scatter_add_(1, t, -ok.to(d.dtype).unsqueeze(1))
    d.mul_(inv_n.to(d.dtype) * ok.unsqueeze(1))
    logits.copy_(d)
    return row_loss, lse


def _lce_accumulate(dw: Tensor, a: Tensor, b: Tensor) -> None:
    """dw += a @ b, with dw in the accumulation dtype."""
    if a.dtype == dw.dtype:
        dw.addmm_(a, b)
    elif a.is_cuda:
        # bf16 operands, fp32 accumulator updated in the GEMM epilogue
        torch.addmm(dw, a, b, out_dtype=dw.dtype, out=dw)
    else:
        dw.addmm_(a.to(dw.dtype), b.to(dw.dtype))


def lce_forward(hidden: Tensor, weight: Tensor, targets: Tensor,
                ignore_index: int, reduction: str,
                chunk_rows: Optional[int], compact: bool,
                need_dhidden: bool, need_dweight: bool,
                chunk_fn=lce_chunk_inplace, slices: int = 0):
    """Compaction + chunk loop. Returns (loss, dhidden | None,
    dweight | None); the gradients are those of `loss` itself."""
    if reduction not in ("mean", "sum"):
        raise ValueError(f"linear_cross_entropy: reduction {reduction!r}")
    N, H = hidden.shape
    V = weight.size(0)
    dev, dtype = hidden.device, hidden.dtype
    acc = _lce_acc_dtype(dtype)
    valid = targets != ignore_index
    idx = None
    h, t = hidden, targets
    if compact:
        idx = valid.nonzero(as_tuple=True)[0]          # the one host sync
        n_valid = idx.numel()
        if n_valid == N:
            idx = None
        else:
            h, t = hidden.index_select(0, idx), targets.index_select(0, idx)
        inv_n = torch.full((1,), 1.0 / max(n_valid, 1), dtype=acc, device=dev)
    else:
        inv_n = valid.sum().clamp_min(1).to(acc).reciprocal().reshape(1)
    if reduction == "sum":
        inv_n = torch.ones(1, dtype=acc, device=dev)

    n_rows = h.size(0)
    cr = chunk_rows or lce_default_chunk_rows(n_rows, V)
    cr = max(1, min(cr, max(n_rows, 1)))
    n_chunks = (n_rows + cr - 1) // cr
    # row stride padded to 8 elements: every row starts 16-byte aligned
    buf = torch.empty(cr, (V + 7) // 8 * 8, dtype=dtype, device=dev)
    w_t = weight.t()
    dh = torch.empty_like(h) if need_dhidden else None
    dw = None
    if need_dweight and n_chunks != 1:
        dw = torch.zeros(V, H, dtype=acc, device=dev)
    row_losses = []
    for i in range(0, n_rows, cr):
        j = min(i + cr, n_rows)
        lg = buf[:j - i, :V]
        torch.mm(h[i:j], w_t, out=lg)
        row_loss, _ = chunk_fn(lg, t[i:j], inv_n, ignore_index, slices)
        row_losses.append(row_loss)
        if need_dhidden:
            torch.mm(lg, weight, out=dh[i:j])
        if need_dweight:
            if n_chunks == 1:
                dw = lg.t() @ h[i:j]
            else:
                _lce_accumulate(dw, lg.t(), h[i:j])
    if row_losses:
        # one fixed-order reduce over all rows: bitwise reproducible
        loss = torch.cat(row_losses).sum() * inv_n[0].to(row_losses[0].dtype)
    else:
        loss = torch.zeros((), dtype=acc, device=dev)
    if need_dweight:
        dw = dw.to(weight.dtype)
    if need_dhidden and idx is not None:
        dh = torch.zeros_like(hidden).index_copy_(0, idx, dh)
    return loss, dh, dw


def lce_backward(ctx, dloss: Tensor):
    dh, dw = ctx.saved_tensors
    return (None if dh is None else dh * dloss.to(dh.dtype),
            None if dw is None else dw * dloss.to(dw.dtype))


class _LinearCEEagerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, weight, targets, ignore_index, reduction,
                chunk_rows, compact, grad_enabled):
        with torch.autocast(device_type=hidden.device.type, enabled=False):
            loss, dh, dw = lce_forward(
                hidden, weight, targets, ignore_index, reduction, chunk_rows,
                compact, grad_enabled and ctx.needs_input_grad[0],
                grad_enabled and ctx.needs_input_grad[1])
        ctx.save_for_backward(dh, dw)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        return lce_backward(ctx, dloss) + (None,) * 6


def linear_cross_entropy(hidden: Tensor, weight: Tensor, targets: Tensor,
                         ignore_index: int = -100, reduction: str = "mean",
                         chunk_rows: Optional[int] = None,
                         compact: bool = True) -> Tensor:
    """CE(hidden @ weight^T, targets) in plain PyTorch, same compaction
    and chunk loop as the HIP op. With every row ignored the loss is 0."""
    return _LinearCEEagerFn.apply(
        hidden.reshape(-1, hidden.size(-1)).contiguous(), weight.contiguous(),
        targets.reshape(-1).contiguous(), ignore_index, reduction,
        chunk_rows, compact, torch.is_grad_enabled())


# ---- Qwen2 decoder-layer pieces (ops/llm_layer.py): the stock transformers
# op sequences, same ops in the same order, so the CPU path is the stock
# model bit for bit.

def add_rms_norm(x: Tensor, residual: Optional[Tensor], weight: Tensor,
                 eps: float) -> tuple[Tensor, Tensor]:
    """(h, n): h = x + residual (x itself without one), n = Qwen2RMSNorm(h)
    (transformers modeling_qwen2.Qwen2RMSNorm.forward)."""
    h = x if residual is None else x + residual
    input_dtype = h.dtype
    hf = h.to(torch.float32)
    variance = hf.pow(2).mean(-1, keepdim=True)
    hf = hf * torch.rsqrt(variance + eps)
    return h, weight * hf.to(input_dtype)


def rotate_half(x: Tensor) -> Tensor:
    x1 = x[..., : x.shape[-1] // 2]
    x2 = x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def rope_qk(q: Tensor, k: Tensor, cos: Tensor,
            sin: Tensor) -> tuple[Tensor, Tensor]:
    """transformers apply_rotary_pos_emb: q, k [B,H,L,D]; cos, sin [B|1,L,D]."""
    cos = cos.unsqueeze(1)
    sin = sin.unsqueeze(1)
    q_embed = (q * cos) + (rotate_half(q) * sin)
    k_embed = (k * cos) + (rotate_half(k) * sin)
    return q_embed, k_embed


def swiglu(gate: Tensor, up: Tensor) -> Tensor:
    """Qwen2MLP's act_fn(gate) * up with the silu activation."""
    return F.silu(gate) * up


# ---- LoRA-adapted linear (ops/lora.py). The three products below are the
# torch forms of the csrc/kernels/lora.hip kernels, same signatures and the
# same rounding points: products accumulate in fp32 (the operands' own
# dtype for fp32 / fp64), T and G are rounded once to the operand dtype,
# up_add adds the fp32 product to the upcast Y and rounds once, the mask
# zeroes elements and c multiplies the fp32 product.

_U64 = 1 << 64


def _s64(c: int) -> int:
    """c mod 2^64 as the int64 with the same bits."""
    c %= _U64
    return c - _U64 if c >= (1 << 63) else c


def _lsr(z: Tensor, n: int) -> Tensor:
    """logical right shift of int64 bit patterns"""
    return (z >> n) & ((1 << (64 - n)) - 1)


def lora_dropout_mask(M: int, Kw: int, p: float, seed: int,
                      device=None) -> Tensor:
    """uint8 [M, Kw] keep mask of the lora kernels, bit for bit: hash_rng
    (csrc/core/common.h) of the position row * Kw + col in wrapping int64
    arithmetic, keep iff its low 24 bits are >= float32(p) * 2^24."""
    idx = torch.arange(M * Kw, dtype=torch.int64, device=device)
    s1 = ((int(seed) & 0xFFFFFFFF) + 1) & 0xFFFFFFFF
    z = idx + _s64(0x9E3779B97F4A7C15 * s1)
    z = (z ^ _lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _s64(0x94D049BB133111EB)
    h = (z ^ _lsr(z, 31)) & 0xFFFFFF
    thresh = int(torch.tensor(p, dtype=torch.float32).item() * 16777216.0)
    return (h >= thresh).to(torch.uint8).view(M, Kw)


def _lora_acc(dtype: torch.dtype) -> torch.dtype:
    return torch.float32 if dtype in (torch.bfloat16, torch.float16) \
        else dtype


def _lora_masked(x: Tensor, p: float, seed: int) -> Tensor:
    if p <= 0.0:
        return x
    keep = lora_dropout_mask(x.size(0), x.size(1), p, seed, x.device)
    return x * keep.to(x.dtype)


def lora_down(x: Tensor, p_mat: Tensor, c: float = 1.0, drop_p: float = 0.0,
              seed: int = 0) -> Tensor:
    """T[M,r] = round(c * (mask.x)[M,Kw] @ p_mat[r,Kw]^T)"""
    acc = _lora_acc(x.dtype)
    xm = _lora_masked(x, drop_p, seed)
    return (c * (xm.to(acc) @ p_mat.to(acc).t())).to(x.dtype)


def lora_up_add_(y: Tensor, t: Tensor, q: Tensor, c: float = 1.0,
                 drop_p: float = 0.0, seed: int = 0) -> Tensor:
    """in place: y[M,Kw] = round(y + c * mask.(t[M,r] @ q[Kw,r]^T))"""
    acc = _lora_acc(y.dtype)
    d = _lora_masked(c * (t.to(acc) @ q.to(acc).t()), drop_p, seed)
    y.copy_((y.to(acc) + d).to(y.dtype))
    return y


def lora_grad(t: Tensor, x: Tensor, c: float = 1.0, drop_p: float = 0.0,
              seed: int = 0) -> Tensor:
    """G[r,Kw] = round(c * t[M,r]^T @ (mask.x)[M,Kw])"""
    acc = _lora_acc(x.dtype)
    xm = _lora_masked(x, drop_p, seed)
    return (c * (t.to(acc).t() @ xm.to(acc))).to(x.dtype)


class LoRALinearFn(torch.autograd.Function):
    """y = x W^T + b + s * (drop(x) A^T) B^T as one node. `impl` supplies
    lora_down / lora_up_add_ / lora_grad: this module (torch) or the
    compiled extension (HIP); everything else is shared. Saves x, the
    rank-r activation t and the seed, never a mask; the base weight's and
    bias's gradients are computed only when asked for."""

    @staticmethod
    def forward(ctx, x, weight, bias, lora_a, lora_b, scaling, p, seed, impl):
        K, N = weight.size(1), weight.size(0)
        y = F.linear(x, weight, bias)
        x2 = impl.lora_rows(x, K)
        inv_keep = 1.0 / (1.0 - p) if p > 0.0 else 1.0
        t = impl.lora_down(x2, lora_a, inv_keep, p, seed)
        impl.lora_up_add_(y.view(-1, N), t, lora_b, scaling, 0.0, 0)
        ctx.save_for_backward(x2, t, weight, lora_a, lora_b)
        ctx.cfg = (scaling, p, seed, inv_keep, impl, x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, t, weight, lora_a, lora_b = ctx.saved_tensors
        scaling, p, seed, inv_keep, impl, x_shape = ctx.cfg
        need = ctx.needs_input_grad
        dy2 = impl.lora_rows(dy, weight.size(0))
        dt = impl.lora_down(dy2, lora_b.t().contiguous(), scaling, 0.0, 0)
        d_a = d_b = dx = dw = dbias = None
        if need[4]:
            d_b = impl.lora_grad(t, dy2, scaling, 0.0, 0).t().contiguous()
        if need[3]:
            d_a = impl.lora_grad(dt, x2, inv_keep, p, seed)
        if need[0]:
            dx2 = dy2 @ weight
            impl.lora_up_add_(dx2, dt, lora_a.t().contiguous(), inv_keep, p,
                              seed)
            dx = dx2.view(x_shape)
        if need[1]:
            dw = dy2.t() @ x2
        if need[2]:
            dbias = dy2.sum(0)
        return dx, dw, dbias, d_a, d_b, None, None, None, None


def lora_rows(t: Tensor, width: int) -> Tensor:
    """t as [rows, width]"""
    return t.reshape(-1, width)


def lora_linear(x: Tensor, weight: Tensor, bias: Optional[Tensor],
                lora_a: Tensor, lora_b: Tensor, scaling: float,
                p: float = 0.0, training: bool = False,
                seed: Optional[int] = None) -> Tensor:
    """The torch form of ops.lora_linear (CPU path and reference)."""
    import sys

    p = float(p) if training else 0.0
    if p > 0.0 and seed is None:
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
    return LoRALinearFn.apply(x, weight, bias, lora_a, lora_b,
                              float(scaling), p, int(seed or 0),
                              sys.modules[__name__])
