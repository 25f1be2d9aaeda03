"""`"genrec_gqa"`: the project's grouped-query flash attention as a
transformers attention implementation (Qwen2 backbone of LCRec / NoteLLM).

Importing this module registers

  * the adapter below with `transformers.AttentionInterface`, and
  * `sdpa_mask` under the same name with `AttentionMaskInterface`, so the
    adapter receives exactly what the stock `sdpa` path receives: `None`
    (pure causal) or a `[B,1,Lq,Lk]` mask equal to causal AND key-valid.

The kernel takes the causal part as a flag (with the Lk - Lq offset of
cached decode) and the padding part as a `[B,Lk]` key mask. The last query
row sees every valid key, so `key_pad = ~mask[:, 0, -1, :]` for left- and
right-padding, prefill and cached decode alike.

Select it with `attn_implementation="genrec_gqa"` on `LCRec` /
`Query2Embedding`, or `model.set_attn_implementation("genrec_gqa")`.
Configurations the kernel does not cover fall back to the stock `sdpa`
function; nothing that works with `sdpa` raises here.

Beam-search decode can hand the adapter a `SharedPrefixBeamCache` as the
extra forward keyword `genrec_beam_state`: the step's attention then runs
`ops.beam_decode_attention` on the cache's one-copy-per-prompt prefix and
its per-beam suffix slots (LCRec.generate_topk, beam_cache="shared_prefix").
A cache built from a packed prefill (`from_packed_prefill`, generate_topk's
prefill="packed") holds token-major prompt K/V without pads and goes through
`ops.beam_decode_varlen_attention`.

Packed ("padding-free") training hands it transformers' own keywords
`cu_seq_lens_q`, `cu_seq_lens_k`, `max_length_q`, `max_length_k` with one
row of T tokens: attention then runs `ops.gqa_varlen_attention`, confined to
each sequence. On that path nothing falls back to `sdpa`, which would attend
across sequences; a configuration it cannot honour raises `ValueError`.
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from genrec_amd.ops.attention import (
    BEAM_MAX_SUFFIX, beam_decode_attention, beam_decode_varlen_attention,
    gqa_flash_attention, gqa_kernel_supported, gqa_varlen_attention,
)

NAME = "genrec_gqa"


class SharedPrefixBeamCache:
    """KV cache of a beam search whose W beams per prompt share the prompt.

    Holds, per layer, the prefill's keys/values [B,Hkv,Lp,D] exactly as the
    prefill left them (no expansion to B*W) and suffix slots k_suf/v_suf
    [B,T,W,Hkv,D]: slot s is what the beam sitting in position w wrote at
    decode step s. One lineage table anc [B,W,T] (int32, shared by all
    layers) says whose slot-s entry beam w inherits, so a beam hop rewrites
    W*T integers instead of gathering every K/V tensor.

    Packed form (from_packed_prefill): k_pre/v_pre are [Ttot,Hkv,D] views of
    a packed prefill's K/V, prompt b owning tokens [cu_seqlens[b],
    cu_seqlens[b+1]); max_prefix is a host upper bound of the prompt
    lengths. There is no pre_pad. Suffix slots, anc, update and advance are
    the same.

    Duck-types the part of `transformers.Cache` a decoder layer uses:
    `update(k, v, layer_idx)` and `get_seq_length()`. Per decode step: every
    layer's `update` copies the step's projections into slot `t`, attention
    reads slots 0..t through `anc`, then `advance(parent)` is called once.
    """

    def __init__(self, k_pre: List[torch.Tensor], v_pre: List[torch.Tensor],
                 beam_width: int, max_suffix: int,
                 pre_pad: Optional[torch.Tensor] = None,
                 cu_seqlens: Optional[torch.Tensor] = None,
                 max_prefix: Optional[int] = None) -> None:
        if not 1 <= max_suffix <= BEAM_MAX_SUFFIX:
            raise ValueError(f"max_suffix {max_suffix}: expected 1.."
                             f"{BEAM_MAX_SUFFIX}")
        if cu_seqlens is None:
            B, Hkv, _, D = k_pre[0].shape
        else:
            if pre_pad is not None or max_prefix is None:
                raise ValueError("a packed prefix takes cu_seqlens and "
                                 "max_prefix, and no pre_pad")
            _, Hkv, D = k_pre[0].shape
            B = cu_seqlens.numel() - 1
        self.cu_seqlens = cu_seqlens              # [B+1] int32 | None
        self.max_prefix = max_prefix
        self.k_pre, self.v_pre = list(k_pre), list(v_pre)
        self.pre_pad = pre_pad                    # [B, Lp] bool | None
        self.beam_width, self.max_suffix = beam_width, max_suffix
        shape = (B, max_suffix, beam_width, Hkv, D)
        self.k_suf = [k.new_zeros(shape) for k in k_pre]
        self.v_suf = [v.new_zeros(shape) for v in v_pre]
        self.t = 0                                # committed suffix slots
        self._own = torch.arange(beam_width, dtype=torch.int32,
                                 device=k_pre[0].device)
        self.anc = torch.zeros(B, beam_width, max_suffix, dtype=torch.int32,
                               device=k_pre[0].device)
        self.anc[:, :, 0] = self._own

    @classmethod
    def from_prefill(cls, cache, beam_width: int, max_suffix: int,
                     pre_pad: Optional[torch.Tensor] = None):
        """From the DynamicCache a prefill over the B prompts filled."""
        return cls([layer.keys for layer in cache.layers],
                   [layer.values for layer in cache.layers],
                   beam_width, max_suffix, pre_pad)

    @classmethod
    def from_packed_prefill(cls, cache, cu_seqlens: torch.Tensor,
                            max_prefix: int, beam_width: int,
                            max_suffix: int):
        """From the DynamicCache a packed [1,T] prefill filled: each layer's
        [1,Hkv,T,D] keys/values become [T,Hkv,D] views, no copy."""
        return cls([layer.keys[0].transpose(0, 1) for layer in cache.layers],
                   [layer.values[0].transpose(0, 1)
                    for layer in cache.layers],
                   beam_width, max_suffix,
                   cu_seqlens=cu_seqlens.to(torch.int32).contiguous(),
                   max_prefix=int(max_prefix))

    @property
    def packed(self) -> bool:
        return self.cu_seqlens is not None

    def get_seq_length(self, layer_idx: int = 0) -> int:
        # packed: an upper bound; position ids are passed explicitly there
        if self.packed:
            return self.max_prefix + self.t
        return self.k_pre[layer_idx].size(2) + self.t

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor,
               layer_idx: int, *args, **kwargs):
        """Store one decode step's [B*W,Hkv,1,D] projections in slot t."""
        dst = self.k_suf[layer_idx][:, self.t]    # [B,W,Hkv,D]
        dst.copy_(key_states[:, :, 0].reshape(dst.shape))
        self.v_suf[layer_idx][:, self.t].copy_(
            value_states[:, :, 0].reshape(dst.shape))
        return key_states, value_states

    def advance(self, parent: torch.Tensor) -> None:
        """Commit slot t after a beam hop: beam w continues parent[b,w]."""
        idx = parent.unsqueeze(-1).expand(-1, -1, self.max_suffix)
        self.anc = self.anc.gather(1, idx)
        self.t += 1
        if self.t < self.max_suffix:
            self.anc[:, :, self.t] = self._own


def _key_pad_from_mask(attention_mask: torch.Tensor, batch: int,
                       lq: int, lk: int) -> Optional[torch.Tensor]:
    """[B,Lk] bool (True = PAD) from a [B|1,1,Lq,Lk] bool or additive float
    mask; None when the mask has another form."""
    if attention_mask.dim() != 4 or attention_mask.size(1) != 1 \
            or attention_mask.size(2) != lq or attention_mask.size(3) != lk \
            or attention_mask.size(0) not in (1, batch):
        return None
    last = attention_mask[:, 0, -1, :]
    if last.dtype == torch.bool:
        pad = ~last
    elif last.is_floating_point():
        pad = last < 0          # additive mask: < 0 = masked
    else:
        return None
    if pad.size(0) != batch:
        pad = pad.expand(batch, lk)
    return pad.contiguous()


def genrec_gqa_attention_forward(
    module: torch.nn.Module,
    query: torch.Tensor,                  # [B, Hq, Lq, D]
    key: torch.Tensor,                    # [B, Hkv, Lk, D]
    value: torch.Tensor,                  # [B, Hkv, Lk, D]
    attention_mask: Optional[torch.Tensor],
    dropout: float = 0.0,
    scaling: Optional[float] = None,
    **kwargs,
) -> Tuple[torch.Tensor, None]:
    from transformers.integrations.sdpa_attention import \
        sdpa_attention_forward

    def stock():
        return sdpa_attention_forward(module, query, key, value,
                                      attention_mask, dropout=dropout,
                                      scaling=scaling, **kwargs)

    beam_state = kwargs.pop("genrec_beam_state", None)
    if beam_state is not None:
        if kwargs.get("sliding_window") is not None or query.size(2) != 1:
            raise ValueError("genrec_beam_state serves single-token decode "
                             "steps of full-attention layers only")
        scale = scaling if scaling is not None else query.size(-1) ** -0.5
        i, st = module.layer_idx, beam_state
        if st.packed:
            out = beam_decode_varlen_attention(
                query, st.k_pre[i], st.v_pre[i], st.cu_seqlens,
                st.max_prefix, st.k_suf[i], st.v_suf[i], st.anc, st.t + 1,
                scale=scale)
        else:
            out = beam_decode_attention(
                query, st.k_pre[i], st.v_pre[i], st.k_suf[i], st.v_suf[i],
                st.anc, st.t + 1, pre_pad=st.pre_pad, scale=scale)
        return out, None                      # [B*W, 1, Hq, D]

    lq, lk = query.size(2), key.size(2)
    is_causal = kwargs.get("is_causal")
    if is_causal is None:
        is_causal = getattr(module, "is_causal", True)

    cu_q = kwargs.get("cu_seq_lens_q")
    if cu_q is not None:
        # packed sequences: one row of T tokens, attention confined to each
        # sequence by the offsets. sdpa would attend across sequences, so
        # whatever this path cannot honour raises.
        cu_k = kwargs.get("cu_seq_lens_k")
        if cu_k is None:
            cu_k = cu_q
        why = None
        if query.size(0) != 1 or lq != lk:
            why = "a batch of one row without a cache"
        elif cu_k is not cu_q and (cu_k.shape != cu_q.shape
                                   or cu_k.data_ptr() != cu_q.data_ptr()):
            why = "cu_seq_lens_q and cu_seq_lens_k to be the same offsets"
        elif kwargs.get("sliding_window") is not None:
            why = "full attention (no sliding window)"
        elif dropout > 0.0 and module.training:
            why = "no attention dropout"
        elif not is_causal:
            why = "causal attention"
        elif kwargs.get("position_bias") is not None:
            why = "no position_bias"
        elif kwargs.get("output_attentions", False):
            why = "output_attentions=False"
        elif query.size(1) % key.size(1) != 0:
            why = "Hq to be a multiple of Hkv"
        if why is not None:
            raise ValueError(f"{NAME}: packed sequences (cu_seq_lens_q) "
                             f"need {why}")
        max_q = kwargs.get("max_length_q")
        max_k = kwargs.get("max_length_k")
        max_len = max(int(max_q or 0), int(max_k or 0)) or lq
        scale = scaling if scaling is not None else query.size(-1) ** -0.5
        if query.is_cuda and torch.is_autocast_enabled("cuda"):
            # what autocast does to sdpa's inputs (RoPE leaves them fp32
            # under fp32 master weights): the kernel takes bf16
            dt = torch.get_autocast_dtype("cuda")
            query, key, value = query.to(dt), key.to(dt), value.to(dt)
        out = gqa_varlen_attention(
            query[0].transpose(0, 1), key[0].transpose(0, 1),
            value[0].transpose(0, 1), cu_q, max_len, scale=scale)
        return out.unsqueeze(0), None         # [1, T, Hq, D]

    if (kwargs.get("sliding_window") is not None
            or (dropout > 0.0 and module.training)
            or kwargs.get("output_attentions", False)
            or kwargs.get("position_bias") is not None
            or not is_causal
            or query.size(1) % key.size(1) != 0
            # on GPU the op must run the kernel: other dtypes / head dims
            # stay on sdpa rather than the fp32 eager composition
            or (query.is_cuda and not gqa_kernel_supported(query, key, value))):
        return stock()

    key_pad = None
    if attention_mask is None:
        # sdpa aligns `is_causal` upper-left; only these two shapes agree
        # with the kernel's cache-offset (lower-right) alignment
        if not (lq == lk or lq == 1):
            return stock()
    else:
        key_pad = _key_pad_from_mask(attention_mask, query.size(0), lq, lk)
        if key_pad is None:
            return stock()

    scale = scaling if scaling is not None else query.size(-1) ** -0.5
    out = gqa_flash_attention(query, key, value, key_pad_mask=key_pad,
                              scale=scale, causal=True)
    return out, None                      # [B, Lq, Hq, D]


def register() -> None:
    """Idempotent registration with transformers."""
    from transformers import AttentionInterface, AttentionMaskInterface
    from transformers.masking_utils import sdpa_mask

    AttentionInterface.register(NAME, genrec_gqa_attention_forward)
    AttentionMaskInterface.register(NAME, sdpa_mask)


register()
