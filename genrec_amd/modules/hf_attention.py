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
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from genrec_amd.ops.attention import gqa_flash_attention, gqa_kernel_supported

NAME = "genrec_gqa"


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

    lq, lk = query.size(2), key.size(2)
    is_causal = kwargs.get("is_causal")
    if is_causal is None:
        is_causal = getattr(module, "is_causal", True)
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
