"""T5-style encoder-decoder transformer (parity: reference transformer.py).

Semantics preserved from the reference implementation:
  * bidirectional log-bucket relative position bias, one per self-attention
    layer, stored as a flat Embedding(n_heads*num_buckets, 1) gathered with
    per-head offsets (transformer.py:13-41, 84-104)
  * fused KV projection for self-attention (transformer.py:72)
  * 1/sqrt(head_dim) score scale (transformer.py:63)
  * key-padding mask at -1e9 then additive attention mask (transformer.py:144-151)
  * pre-norm blocks with optional cross attention, ReLU FFN
    (transformer.py:162-189, 256-324)

MI355X redesign notes:
  * the scores -> bias -> mask -> softmax -> PV chain dispatches to the fused
    CDNA4 attention kernel via genrec_amd.ops.t5_attention
  * bucket index tensors are input-independent per (Lq, Lk); they are cached
    per module instead of recomputed every layer call (reference recomputes
    per layer per forward, transformer.py:84-104)
"""

from __future__ import annotations

import math
import os
from typing import Optional

import torch
from torch import Tensor, nn

from genrec_amd import ops
from genrec_amd.ops.linear import SplitKLinear
from genrec_amd.modules.norms import RMSNorm, T5RMSNorm


def relative_position_bucket(relative_positions: Tensor, num_buckets: int = 32,
                             max_distance: int = 128,
                             bidirectional: bool = True) -> Tensor:
    """Log-bucketing of relative positions (ref transformer.py:13-41)."""
    ret = -relative_positions
    if bidirectional:
        num_buckets //= 2
        sign = (ret < 0).long()
        ret = ret.abs()
    else:
        ret = torch.clamp_min(ret, 0)
    max_exact = num_buckets // 2
    is_small = ret < max_exact
    # guard degenerate max_distance <= max_exact (log denominator -> 0)
    log_denom = math.log(max(max_distance / max_exact, 1.0 + 1e-6))
    large = max_exact + (
        (torch.log(ret.float() / max_exact + 1e-6) / log_denom)
        * (num_buckets - max_exact)
    ).long().clamp(min=0, max=num_buckets - max_exact - 1)
    ret = torch.where(is_small, ret, large)
    if bidirectional:
        ret = ret + sign * num_buckets
    return ret


class T5Attention(nn.Module):
    """Multi-head attention with optional per-layer relative bias."""

    def __init__(self, d_model: int, n_heads: int, dropout: float = 0.0,
                 is_cross_attention: bool = False, has_relative_bias: bool = True,
                 num_relative_buckets: int = 32, max_distance: int = 128) -> None:
        super().__init__()
        assert d_model % n_heads == 0
        self.d_model = d_model
        self.n_heads = n_heads
        self.head_dim = d_model // n_heads
        self.scale = 1.0 / math.sqrt(self.head_dim)
        self.is_cross_attention = is_cross_attention

        if is_cross_attention:
            self.q = SplitKLinear(d_model, d_model, bias=False)
            self.k = SplitKLinear(d_model, d_model, bias=False)
            self.v = SplitKLinear(d_model, d_model, bias=False)
        else:
            # fully-fused qkv projection (round 2): one 384->1152 GEMM
            # replaces the q + kv pair — fewer launches and a wider,
            # better-shaped hipBLASLt tile. (The reference fuses only kv,
            # transformer.py:72.) Old q/kv checkpoints load via
            # _load_from_state_dict below.
            self.qkv = SplitKLinear(d_model, 3 * d_model, bias=False)
        self.o = SplitKLinear(d_model, d_model, bias=False)
        self.dropout_p = dropout

        if has_relative_bias and not is_cross_attention:
            self.rel_bias = nn.Embedding(n_heads * num_relative_buckets, 1)
            self.num_relative_buckets = num_relative_buckets
            self.max_distance = max_distance
        else:
            self.rel_bias = None
        self._bucket_cache: dict = {}

    def _bias_indices(self, q_len: int, k_len: int, device) -> Tensor:
        key = (q_len, k_len, str(device))
        idx = self._bucket_cache.get(key)
        if idx is None:
            ctx = torch.arange(q_len, device=device)[:, None]
            mem = torch.arange(k_len, device=device)[None, :]
            buckets = relative_position_bucket(
                mem - ctx, self.num_relative_buckets, self.max_distance,
                bidirectional=True,
            )
            offs = (torch.arange(self.n_heads, device=device)
                    * self.num_relative_buckets)[:, None, None]
            idx = (buckets.unsqueeze(0) + offs).reshape(-1)
            self._bucket_cache[key] = idx
        return idx

    def compute_bias(self, q_len: int, k_len: int, device) -> Tensor:
        idx = self._bias_indices(q_len, k_len, device)
        return ops.embedding(self.rel_bias.weight, idx).view(
            self.n_heads, q_len, k_len)

    def _bucket_map(self, q_len: int, k_len: int, device) -> Tensor:
        """[q_len, k_len] int32 bucket indices WITHOUT head offsets (the
        kernel adds h*n_buckets) — cached per shape/device."""
        key = ("bm", q_len, k_len, str(device))
        bm = self._bucket_cache.get(key)
        if bm is None:
            ctx = torch.arange(q_len, device=device)[:, None]
            mem = torch.arange(k_len, device=device)[None, :]
            bm = relative_position_bucket(
                mem - ctx, self.num_relative_buckets, self.max_distance,
                bidirectional=True).to(torch.int32).contiguous()
            self._bucket_cache[key] = bm
        return bm

    def _split(self, x: Tensor) -> Tensor:
        b, l, _ = x.shape
        return x.view(b, l, self.n_heads, self.head_dim).transpose(1, 2)

    def forward(self, query: Tensor, key: Optional[Tensor] = None,
                value: Optional[Tensor] = None,
                attn_mask: Optional[Tensor] = None,
                key_padding_mask: Optional[Tensor] = None,
                kv_cache: Optional[dict] = None,
                cross_kv: Optional[tuple] = None) -> Tensor:
        """cross_kv = (CrossKV, layer index): a cross-attention layer then
        takes its K/V from the stack's one fused projection of the memory
        (ops.project_cross_kv) and leaves self.k / self.v to it."""
        if self.is_cross_attention:
            if cross_kv is not None:
                ckv, layer = cross_kv
                q = self._split(self.q(query))
                out = ops.cross_attention_kv(
                    q, ckv, layer, key_padding_mask, self.scale,
                    self.dropout_p, self.training)
                out = out.transpose(1, 2).reshape(q.size(0), -1,
                                                  self.d_model)
                return self.o(out)
            if kv_cache is not None and "k" in kv_cache:
                k, v = kv_cache["k"], kv_cache["v"]
            else:
                k, v = self._split(self.k(key)), self._split(self.v(value))
                if kv_cache is not None:
                    kv_cache["k"], kv_cache["v"] = k, v
        else:
            qkv = self.qkv(query)
            table_bias = self.rel_bias is not None and \
                os.environ.get("GENREC_ATTN_TABLE_BIAS", "0") == "1"
            if ops.packed_qkv_eligible(qkv, self.n_heads, attn_mask,
                                       kv_cache, table_bias):
                # the attention backward writes the gradient of qkv as one
                # tensor: no concatenation of dq, dk, dv
                seq = qkv.size(1)
                bias = None
                if self.rel_bias is not None:
                    bias = self.compute_bias(seq, seq, qkv.device)
                out = ops.t5_self_attention_packed(
                    qkv, self.n_heads, bias, key_padding_mask, attn_mask,
                    self.scale, self.dropout_p, self.training)
                out = out.transpose(1, 2).reshape(qkv.size(0), -1,
                                                  self.d_model)
                return self.o(out)
            q_flat, k, v = qkv.chunk(3, dim=-1)
            k, v = self._split(k), self._split(v)
            if kv_cache is not None:
                if "k" in kv_cache:
                    k = torch.cat([kv_cache["k"], k], dim=2)
                    v = torch.cat([kv_cache["v"], v], dim=2)
                kv_cache["k"], kv_cache["v"] = k, v
            q = self._split(q_flat)
            return self._attend(q, k, v, attn_mask, key_padding_mask)
        q = self._split(self.q(query))
        return self._attend(q, k, v, attn_mask, key_padding_mask)

    def _attend(self, q: Tensor, k: Tensor, v: Tensor,
                attn_mask: Optional[Tensor],
                key_padding_mask: Optional[Tensor]) -> Tensor:

        bias = None
        bias_table = bias_bucket = None
        if self.rel_bias is not None:
            if os.environ.get("GENREC_ATTN_TABLE_BIAS", "0") == "1" \
                    and q.is_cuda:
                # in-kernel rel-bias table gather (round 2): no
                # materialized [H,Lq,Lk] bias, backward accumulates table
                # grads directly (LDS histogram + deterministic colsum)
                bias_table = self.rel_bias.weight.view(-1)
                bm = self._bucket_map(k.size(2), k.size(2), q.device)
                if q.size(2) != k.size(2):  # cached incremental decode
                    bm = bm[k.size(2) - q.size(2):, :].contiguous()
                bias_bucket = bm
            else:
                # cached incremental decode: queries sit at the LAST
                # q_len positions of the k_len-long sequence, so take the
                # bottom rows of the full bias square
                bias = self.compute_bias(k.size(2), k.size(2), q.device)
                if q.size(2) != k.size(2):
                    bias = bias[:, k.size(2) - q.size(2):, :]

        out = ops.t5_attention(
            q, k, v, bias, key_padding_mask, attn_mask, self.scale,
            self.dropout_p, self.training,
            bias_table=bias_table, bias_bucket=bias_bucket,
        )
        b = out.size(0)
        out = out.transpose(1, 2).reshape(b, -1, self.d_model)
        return self.o(out)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # round-1 self-attn checkpoints stored separate q / kv weights
        qk, kvk = prefix + "q.weight", prefix + "kv.weight"
        if (not self.is_cross_attention and qk in state_dict
                and prefix + "qkv.weight" not in state_dict):
            state_dict[prefix + "qkv.weight"] = torch.cat(
                [state_dict.pop(qk), state_dict.pop(kvk)], dim=0)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class FeedForward(nn.Module):
    """T5-style FFN: wi -> relu -> dropout -> wo (ref transformer.py:162-189)."""

    def __init__(self, dim: int, hidden_dim: int = 2048,
                 dropout: float = 0.1) -> None:
        super().__init__()
        self.wi = SplitKLinear(dim, hidden_dim, bias=False)
        self.wo = SplitKLinear(hidden_dim, dim, bias=False)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x: Tensor) -> Tensor:
        return self.wo(ops.relu_dropout(self.wi(x), self.dropout.p,
                                        self.training))


class TransformerBlock(nn.Module):
    """Pre-norm block: self-attn [+ cross-attn] + FFN (ref transformer.py:256-324)."""

    def __init__(self, dim: int, num_heads: int, dropout: float = 0.1,
                 norm_cls: type = RMSNorm, ff_hidden_dim: int = 2048,
                 cross_attn: bool = False) -> None:
        super().__init__()
        self.cross_attn_enabled = cross_attn
        self.self_attn = T5Attention(dim, num_heads, dropout)
        self.norm1 = norm_cls(dim)
        self.dropout1 = nn.Dropout(dropout)
        if cross_attn:
            self.cross_attn = T5Attention(dim, num_heads, dropout,
                                          is_cross_attention=True,
                                          has_relative_bias=False)
            self.norm_cross = norm_cls(dim)
            self.dropout_cross = nn.Dropout(dropout)
        self.ff = FeedForward(dim, hidden_dim=ff_hidden_dim, dropout=dropout)
        self.norm2 = norm_cls(dim)
        self.dropout2 = nn.Dropout(dropout)

    def forward(self, x: Tensor, *, context: Optional[Tensor] = None,
                attn_mask: Optional[Tensor] = None,
                key_padding_mask: Optional[Tensor] = None,
                memory_key_padding_mask: Optional[Tensor] = None,
                kv_cache: Optional[dict] = None,
                normed: Optional[Tensor] = None,
                next_norm: Optional[nn.Module] = None,
                cross_kv: Optional[tuple] = None):
        """Returns the block output. `normed` and `next_norm` let a stack
        fuse across blocks: `normed` is norm1(x) already computed by the
        previous block, and with `next_norm` (the next block's norm1) the
        block returns (output, next_norm(output)). `cross_kv` goes to the
        cross-attention layer (T5Attention.forward)."""
        self_cache = cross_cache = None
        if kv_cache is not None:
            self_cache = kv_cache.setdefault("self", {})
            cross_cache = kv_cache.setdefault("cross", {})
        if normed is None:
            normed = self.norm1(x)
        use_cross = self.cross_attn_enabled and context is not None
        x, normed = _dropout_add_norm(self.self_attn(
            normed, attn_mask=attn_mask,
            key_padding_mask=key_padding_mask, kv_cache=self_cache,
        ), x, self.dropout1.p, self.training,
            self.norm_cross if use_cross else self.norm2)
        if use_cross:
            x, normed = _dropout_add_norm(self.cross_attn(
                normed, key=context, value=context,
                key_padding_mask=memory_key_padding_mask, kv_cache=cross_cache,
                cross_kv=cross_kv,
            ), x, self.dropout_cross.p, self.training, self.norm2)
        y = self.ff(normed)
        if next_norm is None:
            return ops.dropout_add(y, x, self.dropout2.p, self.training)
        return _dropout_add_norm(y, x, self.dropout2.p, self.training,
                                 next_norm)


def _dropout_add_norm(y: Tensor, x: Tensor, p: float, training: bool,
                      norm: nn.Module) -> tuple[Tensor, Tensor]:
    """(h, norm(h)) for h = x + dropout(y): one fused op when `norm` is one
    of the two RMS classes, the composed pair for any other norm_cls."""
    if type(norm) is RMSNorm:
        return ops.dropout_add_rms_norm(y, x, norm.weight, p, norm.eps,
                                        False, training)
    if type(norm) is T5RMSNorm:
        return ops.dropout_add_rms_norm(y, x, norm.weight, p,
                                        norm.variance_epsilon, True, training)
    h = ops.dropout_add(y, x, p, training)
    return h, norm(h)


def _run_layers(layers, x: Tensor, kv_caches: Optional[list] = None,
                cross_kv=None, **kwargs) -> Tensor:
    """Run a stack of blocks, handing each block's last residual add to the
    next block's norm1 so the pair runs fused. With `cross_kv` (a CrossKV)
    block i gets (cross_kv, i)."""
    normed = None
    last = len(layers) - 1
    for i, layer in enumerate(layers):
        kv = kv_caches[i] if kv_caches is not None else None
        if cross_kv is not None:
            kwargs["cross_kv"] = (cross_kv, i)
        if i < last:
            x, normed = layer(x, kv_cache=kv, normed=normed,
                              next_norm=layers[i + 1].norm1, **kwargs)
        else:
            x = layer(x, kv_cache=kv, normed=normed, **kwargs)
    return x


class TransformerEncoder(nn.Module):
    def __init__(self, dim: int, depth: int, num_heads: int,
                 dropout: float = 0.1, norm_cls: type = RMSNorm,
                 ff_hidden_dim: int = 2048) -> None:
        super().__init__()
        self.layers = nn.ModuleList([
            TransformerBlock(dim, num_heads, dropout, norm_cls=norm_cls,
                             ff_hidden_dim=ff_hidden_dim, cross_attn=False)
            for _ in range(depth)
        ])

    def forward(self, src: Tensor, *, attn_mask: Optional[Tensor] = None,
                key_padding_mask: Optional[Tensor] = None) -> Tensor:
        return _run_layers(self.layers, src, attn_mask=attn_mask,
                           key_padding_mask=key_padding_mask)


class TransformerDecoder(nn.Module):
    def __init__(self, dim: int, depth: int, num_heads: int,
                 dropout: float = 0.1, norm_cls: type = RMSNorm,
                 ff_hidden_dim: int = 2048) -> None:
        super().__init__()
        self.layers = nn.ModuleList([
            TransformerBlock(dim, num_heads, dropout, norm_cls=norm_cls,
                             ff_hidden_dim=ff_hidden_dim, cross_attn=True)
            for _ in range(depth)
        ])

    def forward(self, tgt: Tensor, *, memory: Tensor,
                attn_mask: Optional[Tensor] = None,
                key_padding_mask: Optional[Tensor] = None,
                memory_key_padding_mask: Optional[Tensor] = None,
                kv_caches: Optional[list] = None,
                cross_kv_impl: Optional[str] = None) -> Tensor:
        """When the stack is eligible (ops.cross_kv_eligible: training-
        style call without kv_caches, bf16 on the GPU, ...) the memory is
        projected to every layer's cross-attention K/V in one GEMM;
        GENREC_DISABLE_CROSS_KV_FUSE=1 keeps the per-layer projections.
        cross_kv_impl="torch" (tests) takes the fused route in plain
        PyTorch on any device and dtype."""
        if cross_kv_impl is not None and kv_caches is not None:
            raise ValueError("cross_kv_impl and kv_caches exclude each other")
        cross_kv = None
        attns = [layer.cross_attn for layer in self.layers]
        if cross_kv_impl is not None or (attns and ops.cross_kv_eligible(
                memory, tgt, [a.k.weight for a in attns],
                [a.v.weight for a in attns],
                [b for a in attns for b in (a.k.bias, a.v.bias)],
                attns[0].n_heads, kv_caches)):
            cross_kv = ops.project_cross_kv(
                memory, [a.k.weight for a in attns],
                [a.v.weight for a in attns], impl=cross_kv_impl)
        return _run_layers(self.layers, tgt, kv_caches, cross_kv,
                           context=memory,
                           attn_mask=attn_mask,
                           key_padding_mask=key_padding_mask,
                           memory_key_padding_mask=memory_key_padding_mask)


class TransformerEncoderDecoder(nn.Module):
    """Encoder-decoder wrapper (ref transformer.py:417-476)."""

    def __init__(self, d_model: int, nhead: int, num_encoder_layers: int,
                 num_decoder_layers: int, dim_feedforward: int = 2048,
                 dropout: float = 0.1, norm_cls: type = RMSNorm) -> None:
        super().__init__()
        self.encoder = TransformerEncoder(
            dim=d_model, depth=num_encoder_layers, num_heads=nhead,
            dropout=dropout, norm_cls=norm_cls, ff_hidden_dim=dim_feedforward)
        self.decoder = TransformerDecoder(
            dim=d_model, depth=num_decoder_layers, num_heads=nhead,
            dropout=dropout, norm_cls=norm_cls, ff_hidden_dim=dim_feedforward)

    def forward(self, src: Tensor, tgt: Tensor, *,
                src_key_padding_mask: Optional[Tensor] = None,
                tgt_key_padding_mask: Optional[Tensor] = None,
                memory_key_padding_mask: Optional[Tensor] = None,
                src_mask: Optional[Tensor] = None,
                tgt_mask: Optional[Tensor] = None) -> Tensor:
        if tgt_mask is None:
            t = tgt.size(1)
            tgt_mask = torch.triu(
                torch.full((t, t), float("-inf"), device=tgt.device), diagonal=1)
        memory = self.encoder(src, attn_mask=src_mask,
                              key_padding_mask=src_key_padding_mask)
        return self.decoder(tgt, memory=memory, attn_mask=tgt_mask,
                            key_padding_mask=tgt_key_padding_mask,
                            memory_key_padding_mask=memory_key_padding_mask)
