"""`"genrec_fused"`: the project's layer kernels inside a transformers Qwen2
decoder layer (backbone of LCRec / NoteLLM).

`install(model)` switches every `Qwen2DecoderLayer`, its `Qwen2Attention`
and `Qwen2MLP`, and every `Qwen2RMSNorm` (the final `model.norm` included)
of one model instance to the subclasses below; `uninstall(model)` switches
them back. A layer then runs

    n1      = add_rms_norm(x, None, input_layernorm.weight)[1]
    q, k, v = the three projection modules, viewed as in the stock layer
    q, k    = rope_qk(q, k, cos, sin)
    attn    = the registered attention interface, unchanged
    h, n2   = add_rms_norm(o_proj(attn), x, post_attention_layernorm.weight)
    out     = h + down_proj(swiglu(gate_proj(n2), up_proj(n2)))

with the three ops of `genrec_amd.ops.llm_layer`. The switch swaps the
instances' `__class__`: no parameter, buffer or state-dict key changes,
`copy.deepcopy` of an installed model is installed, and a stock model in
the same process stays stock. Projections are called as modules, so a
wrapped (LoRA) linear keeps working. On CPU, in fp32 and for shapes the
kernels do not take, the ops are the stock op sequences and the layer
computes what the stock layer computes, bit for bit.

Written against transformers 5.x (`Qwen2DecoderLayer.forward` with
`position_embeddings`). The residual add that ends a layer is not fused
into the next layer's first norm: the layer loop belongs to transformers.

Select with `layer_implementation="genrec_fused"` on `LCRec` /
`Query2Embedding`.
"""

from __future__ import annotations

import logging
from typing import Callable

import torch
from torch import nn
from transformers.models.qwen2 import modeling_qwen2 as _hf

from genrec_amd.ops.llm_layer import add_rms_norm, rope_qk, swiglu

NAME = "genrec_fused"

logger = logging.getLogger("genrec_amd")


class FusedQwen2RMSNorm(_hf.Qwen2RMSNorm):
    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        return add_rms_norm(hidden_states, None, self.weight,
                            self.variance_epsilon)[1]


class FusedQwen2MLP(_hf.Qwen2MLP):
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not isinstance(self.act_fn, nn.SiLU) \
                and type(self.act_fn).__name__ != "SiLUActivation":
            return super().forward(x)
        return self.down_proj(swiglu(self.gate_proj(x), self.up_proj(x)))


class FusedQwen2Attention(_hf.Qwen2Attention):
    """Qwen2Attention.forward with the rotary embedding through rope_qk."""

    def forward(self, hidden_states, position_embeddings, attention_mask,
                past_key_values=None, **kwargs):
        input_shape = hidden_states.shape[:-1]
        hidden_shape = (*input_shape, -1, self.head_dim)

        query_states = self.q_proj(hidden_states).view(hidden_shape) \
            .transpose(1, 2)
        key_states = self.k_proj(hidden_states).view(hidden_shape) \
            .transpose(1, 2)
        value_states = self.v_proj(hidden_states).view(hidden_shape) \
            .transpose(1, 2)

        cos, sin = position_embeddings
        query_states, key_states = rope_qk(query_states, key_states, cos, sin)

        if past_key_values is not None:
            key_states, value_states = past_key_values.update(
                key_states, value_states, self.layer_idx)

        attention_interface: Callable = \
            _hf.ALL_ATTENTION_FUNCTIONS.get_interface(
                self.config._attn_implementation, _hf.eager_attention_forward)
        attn_output, attn_weights = attention_interface(
            self, query_states, key_states, value_states, attention_mask,
            dropout=0.0 if not self.training else self.attention_dropout,
            scaling=self.scaling, sliding_window=self.sliding_window,
            **kwargs)

        attn_output = attn_output.reshape(*input_shape, -1).contiguous()
        return self.o_proj(attn_output), attn_weights


class FusedQwen2DecoderLayer(_hf.Qwen2DecoderLayer):
    def forward(self, hidden_states, attention_mask=None, position_ids=None,
                past_key_values=None, use_cache=False,
                position_embeddings=None, **kwargs):
        attn, _ = self.self_attn(
            hidden_states=self.input_layernorm(hidden_states),
            attention_mask=attention_mask, position_ids=position_ids,
            past_key_values=past_key_values, use_cache=use_cache,
            position_embeddings=position_embeddings, **kwargs)
        norm = self.post_attention_layernorm
        h, n2 = add_rms_norm(attn, hidden_states, norm.weight,
                             norm.variance_epsilon)
        return h + self.mlp(n2)


# stock class -> fused subclass
_SWAP = {
    _hf.Qwen2DecoderLayer: FusedQwen2DecoderLayer,
    _hf.Qwen2Attention: FusedQwen2Attention,
    _hf.Qwen2MLP: FusedQwen2MLP,
    _hf.Qwen2RMSNorm: FusedQwen2RMSNorm,
}
_UNSWAP = {fused: stock for stock, fused in _SWAP.items()}

_warned: set = set()


def install(model: nn.Module) -> int:
    """Switch the Qwen2 layers under `model` to the fused route; returns
    how many decoder layers were switched. A model without any (another
    architecture) gets one logged warning per class and stays stock."""
    mods = list(model.modules())
    layers = sum(isinstance(m, _hf.Qwen2DecoderLayer) for m in mods)
    if layers:
        for m in mods:
            fused = _SWAP.get(type(m))
            if fused is not None:
                m.__class__ = fused
    else:
        name = type(model).__name__
        if name not in _warned:
            _warned.add(name)
            logger.warning(
                "layer_implementation='genrec_fused' needs transformers "
                "Qwen2 decoder layers; %s has none and stays stock", name)
    return layers


def uninstall(model: nn.Module) -> None:
    """Back to the stock transformers classes."""
    for m in model.modules():
        stock = _UNSWAP.get(type(m))
        if stock is not None:
            m.__class__ = stock


def installed(model: nn.Module) -> bool:
    return any(isinstance(m, FusedQwen2DecoderLayer) for m in model.modules())
