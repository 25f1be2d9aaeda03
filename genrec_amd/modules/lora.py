"""LoRA adapters for the transformers backbones (LCRec's Qwen2).

`apply_lora(model)` freezes the model and wraps the targeted `nn.Linear`
projections in `LoRALinear`, whose forward is `ops.lora_linear`: the base
GEMM plus the fused rank-r kernels on the GPU. The wrapping sits inside the
`PreTrainedModel`, so `loss_implementation="genrec_lce"`, packing and
`layer_implementation="genrec_fused"` (which calls the projections as
modules) see the model they saw before.

`merged_state_dict` folds every adapter into its base weight under the
plain transformers key names; `save_adapter` / `load_adapter` write and
read the adapter alone in the peft file layout (`adapter_model.safetensors`
+ `adapter_config.json`).
"""

from __future__ import annotations

import json
import math
import os
from typing import Dict, Iterable, Optional, Sequence

import torch
from torch import Tensor, nn

from genrec_amd import ops

# the reference trainer's targets: every projection of a Qwen2 layer
DEFAULT_TARGET_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj",
                          "gate_proj", "up_proj", "down_proj")

ADAPTER_WEIGHTS = "adapter_model.safetensors"
ADAPTER_CONFIG = "adapter_config.json"
_KEY_PREFIX = "base_model.model."


class LoRALinear(nn.Module):
    """base(x) + (alpha / r) * lora_B(lora_A(dropout(x))) with the base
    layer frozen. lora_A is kaiming-uniform, lora_B zero, so a fresh
    adapter leaves the layer's output unchanged."""

    def __init__(self, base: nn.Linear, r: int = 16, alpha: float = 32,
                 dropout: float = 0.05) -> None:
        super().__init__()
        if not isinstance(base, nn.Linear):
            raise TypeError(f"LoRALinear wraps nn.Linear, got {type(base)}")
        if r <= 0:
            raise ValueError(f"rank must be positive, got {r}")
        self.base_layer = base
        for prm in base.parameters():
            prm.requires_grad_(False)
        kw = dict(bias=False, device=base.weight.device,
                  dtype=base.weight.dtype)
        self.lora_A = nn.Linear(base.in_features, r, **kw)
        self.lora_B = nn.Linear(r, base.out_features, **kw)
        nn.init.kaiming_uniform_(self.lora_A.weight, a=math.sqrt(5))
        nn.init.zeros_(self.lora_B.weight)
        self.r = r
        self.lora_alpha = alpha
        self.lora_dropout = float(dropout)
        self.scaling = alpha / r

    # code that inspects a projection keeps working
    @property
    def weight(self) -> Tensor:
        return self.base_layer.weight

    @property
    def bias(self) -> Optional[Tensor]:
        return self.base_layer.bias

    @property
    def in_features(self) -> int:
        return self.base_layer.in_features

    @property
    def out_features(self) -> int:
        return self.base_layer.out_features

    def forward(self, x: Tensor) -> Tensor:
        return ops.lora_linear(x, self.base_layer.weight,
                               self.base_layer.bias, self.lora_A.weight,
                               self.lora_B.weight, self.scaling,
                               p=self.lora_dropout, training=self.training)

    def merged_weight(self) -> Tensor:
        """W + scaling * B A in fp32, rounded once to W's dtype."""
        w = self.base_layer.weight
        delta = self.lora_B.weight.detach().float() \
            @ self.lora_A.weight.detach().float()
        return (w.detach().float() + self.scaling * delta).to(w.dtype)

    def extra_repr(self) -> str:
        return (f"r={self.r}, alpha={self.lora_alpha}, "
                f"dropout={self.lora_dropout}")


def _adapters(model: nn.Module) -> Dict[str, LoRALinear]:
    return {name: m for name, m in model.named_modules()
            if isinstance(m, LoRALinear)}


def apply_lora(model: nn.Module, r: int = 16, alpha: float = 32,
               dropout: float = 0.05,
               target_modules: Optional[Iterable[str]] = None,
               modules_to_save: Sequence[str] = ()) -> int:
    """Freeze `model`, wrap every nn.Linear whose attribute name is in
    `target_modules` (default: the seven Qwen2 projections) and re-enable
    gradients of the modules named in `modules_to_save`. Returns the number
    of wrapped modules."""
    targets = set(DEFAULT_TARGET_MODULES if target_modules is None
                  else target_modules)
    saved = tuple(modules_to_save)
    for prm in model.parameters():
        prm.requires_grad_(False)
    wrapped = 0
    for parent in list(model.modules()):
        if isinstance(parent, LoRALinear):
            continue
        for name, child in list(parent.named_children()):
            if name in targets and isinstance(child, nn.Linear):
                setattr(parent, name, LoRALinear(child, r, alpha, dropout))
                wrapped += 1
    for name, mod in model.named_modules():
        if name.rsplit(".", 1)[-1] in saved and not isinstance(mod, LoRALinear):
            for prm in mod.parameters():
                prm.requires_grad_(True)
    # with the embedding frozen nothing that enters the first layer would
    # require grad, and a checkpointed layer would then record no graph
    embed_trains = any(prm.requires_grad for prm in
                       model.get_input_embeddings().parameters()) \
        if hasattr(model, "get_input_embeddings") else True
    if wrapped and not embed_trains \
            and hasattr(model, "enable_input_require_grads"):
        model.enable_input_require_grads()
    model._genrec_lora_config = dict(
        peft_type="LORA", r=r, lora_alpha=alpha, lora_dropout=dropout,
        target_modules=sorted(targets), modules_to_save=list(saved))
    return wrapped


def lora_config(model: nn.Module) -> Optional[dict]:
    """The config apply_lora left on `model`, or None."""
    return getattr(model, "_genrec_lora_config", None)


def _plain_key(key: str) -> Optional[str]:
    """state-dict key of a wrapped model -> plain transformers key; None
    for the adapter's own tensors."""
    if ".lora_A." in key or ".lora_B." in key:
        return None
    return key.replace(".base_layer.", ".")


@torch.no_grad()
def merged_state_dict(model: nn.Module) -> Dict[str, Tensor]:
    """State dict in the plain (unwrapped) key layout with every adapter
    folded into its base weight: bf16/fp32(W + scaling * B @ A), computed in
    fp32 one layer at a time. The live model is not modified."""
    adapters = _adapters(model)
    out: Dict[str, Tensor] = {}
    for key, val in model.state_dict().items():
        plain = _plain_key(key)
        if plain is None:
            continue
        if key.endswith(".base_layer.weight"):
            val = adapters[key[: -len(".base_layer.weight")]].merged_weight()
        out[plain] = val
    return out


def _saved_modules(model: nn.Module, names: Sequence[str]):
    for name, mod in model.named_modules():
        if name.rsplit(".", 1)[-1] in names \
                and not isinstance(mod, LoRALinear):
            yield name, mod


def save_adapter(model: nn.Module, save_dir: str) -> None:
    """Write the adapter alone: adapter_model.safetensors with keys
    base_model.model.<module path>.lora_{A,B}.weight (plus the tensors of
    modules_to_save modules) and adapter_config.json."""
    from safetensors.torch import save_file

    cfg = lora_config(model)
    if cfg is None:
        raise ValueError("save_adapter: model has no adapters (apply_lora)")
    tensors = {}
    for name, mod in _adapters(model).items():
        for part in ("lora_A", "lora_B"):
            tensors[f"{_KEY_PREFIX}{name}.{part}.weight"] = \
                getattr(mod, part).weight.detach().cpu().contiguous()
    for name, mod in _saved_modules(model, cfg["modules_to_save"]):
        for pname, prm in mod.state_dict().items():
            tensors[f"{_KEY_PREFIX}{name}.{pname}"] = \
                prm.detach().cpu().contiguous().clone()
    os.makedirs(save_dir, exist_ok=True)
    save_file(tensors, os.path.join(save_dir, ADAPTER_WEIGHTS))
    with open(os.path.join(save_dir, ADAPTER_CONFIG), "w") as f:
        json.dump(cfg, f, indent=2)


@torch.no_grad()
def load_adapter(model: nn.Module, load_dir: str) -> dict:
    """Copy a saved adapter into an already wrapped model (apply_lora with
    the same targets); returns the saved config."""
    from safetensors.torch import load_file

    with open(os.path.join(load_dir, ADAPTER_CONFIG)) as f:
        cfg = json.load(f)
    tensors = load_file(os.path.join(load_dir, ADAPTER_WEIGHTS))
    adapters = _adapters(model)
    saved = dict(_saved_modules(model, cfg.get("modules_to_save", ())))
    used = set()
    for name, mod in adapters.items():
        for part in ("lora_A", "lora_B"):
            key = f"{_KEY_PREFIX}{name}.{part}.weight"
            if key not in tensors:
                raise KeyError(f"load_adapter: {key} missing in {load_dir}")
            getattr(mod, part).weight.copy_(tensors[key])
            used.add(key)
    for name, mod in saved.items():
        for pname, prm in mod.state_dict().items():
            key = f"{_KEY_PREFIX}{name}.{pname}"
            if key in tensors:
                prm.copy_(tensors[key])
                used.add(key)
    extra = set(tensors) - used
    if extra:
        raise KeyError(f"load_adapter: no module for {sorted(extra)[:4]}")
    return cfg
