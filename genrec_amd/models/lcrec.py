"""LCRec: LLM + collaborative semantics (arXiv:2311.09049).

Parity target: /root/reference/genrec/models/lcrec.py (243 LoC). A causal
LLM backbone (Qwen2-family) extended with `<Ci_j>` codebook special tokens
(lcrec.py:48-60), SFT tokenization helpers (lcrec.py:88-112), HF-format
save/load (lcrec.py:135-162), and constrained top-k beam generation.

MI355X redesign:
  * offline-first: with no pretrained directory (this environment has no
    network), the backbone is a random-init Qwen2 built from a config and
    the tokenizer is a from-scratch byte-level BPE — the full pipeline
    (vocab resize, SFT, constrained decode) runs identically
  * generate_topk is a BATCHED KV-cached beam search: the reference
    re-runs the full forward per beam per step with no cache
    (lcrec.py:164-243 — B*W forwards of the whole prefix each step); here
    all beams advance in one forward on the incremental token with a
    DynamicCache reordered per beam hop, and the per-position legal-token
    mask is a device tensor rather than a Python callable per token.
"""

from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Tuple

import logging

import torch
import torch.nn.functional as F
from torch import nn

from genrec_amd.config import ginlite

logger = logging.getLogger("genrec_amd")


def default_qwen_config(vocab_size: int = 512, hidden_size: int = 1536,
                        num_layers: int = 28, num_heads: int = 12,
                        num_kv_heads: int = 2, intermediate_size: int = 8960,
                        max_position_embeddings: int = 4096):
    """Qwen2.5-1.5B-shaped config (the reference's shipped backbone,
    config/base.gin:19) buildable offline."""
    from transformers import Qwen2Config

    return Qwen2Config(
        vocab_size=vocab_size, hidden_size=hidden_size,
        intermediate_size=intermediate_size, num_hidden_layers=num_layers,
        num_attention_heads=num_heads, num_key_value_heads=num_kv_heads,
        max_position_embeddings=max_position_embeddings, tie_word_embeddings=True)


def _attn_kwargs(attn_implementation: Optional[str]) -> Dict[str, str]:
    """from_config / from_pretrained kwargs for an attention switch. None
    passes nothing (the transformers default); "genrec_gqa" is registered
    by importing genrec_amd.modules.hf_attention."""
    if attn_implementation is None:
        return {}
    from genrec_amd.modules import hf_attention  # noqa: F401  (registers)

    return {"attn_implementation": attn_implementation}


LOSS_IMPLEMENTATIONS = (None, "genrec_lce")
LAYER_IMPLEMENTATIONS = (None, "genrec_fused")
BEAM_CACHES = (None, "shared_prefix")
PREFILLS = (None, "packed")


def _check_layer_implementation(layer_implementation: Optional[str]) -> None:
    if layer_implementation not in LAYER_IMPLEMENTATIONS:
        raise ValueError(
            f"layer_implementation {layer_implementation!r}: expected one "
            f"of {LAYER_IMPLEMENTATIONS}")


def _apply_layer_implementation(model: nn.Module,
                                layer_implementation: Optional[str]) -> None:
    """None leaves the transformers layers alone; "genrec_fused" switches
    this model instance's Qwen2 layers to genrec_amd.modules.hf_layers."""
    if layer_implementation == "genrec_fused":
        from genrec_amd.modules import hf_layers

        hf_layers.install(model)


@ginlite.configurable(name="LCRec")
class LCRec(nn.Module):
    def __init__(self, pretrained_path: Optional[str] = None,
                 config=None,
                 attn_implementation: Optional[str] = None,
                 loss_implementation: Optional[str] = None,
                 layer_implementation: Optional[str] = None) -> None:
        super().__init__()
        from transformers import AutoModelForCausalLM, AutoTokenizer

        _check_layer_implementation(layer_implementation)
        # None = the transformers decoder layer; "genrec_fused" = fused
        # add+RMSNorm, RoPE and SwiGLU kernels inside every layer
        self.layer_implementation = layer_implementation

        if loss_implementation not in LOSS_IMPLEMENTATIONS:
            raise ValueError(
                f"loss_implementation {loss_implementation!r}: expected one "
                f"of {LOSS_IMPLEMENTATIONS}")
        # None = the backbone's own loss over full [B, L, V] logits;
        # "genrec_lce" = ops.linear_cross_entropy on the hidden states
        self.loss_implementation = loss_implementation
        self._lce_fallback_logged = False
        self.attn_implementation = attn_implementation
        attn_kw = _attn_kwargs(attn_implementation)
        if pretrained_path and os.path.isdir(pretrained_path):
            self.tokenizer = AutoTokenizer.from_pretrained(pretrained_path)
            self.model = AutoModelForCausalLM.from_pretrained(
                pretrained_path, **attn_kw)
        else:
            from genrec_amd.utils.tokenizer import build_offline_tokenizer

            self.tokenizer = build_offline_tokenizer()
            cfg = config or default_qwen_config(
                vocab_size=max(len(self.tokenizer), 512))
            if cfg.vocab_size < len(self.tokenizer):
                cfg.vocab_size = len(self.tokenizer)
            self.model = AutoModelForCausalLM.from_config(cfg, **attn_kw)
        _apply_layer_implementation(self.model, layer_implementation)

    def gradient_checkpointing_enable(self):
        self.model.gradient_checkpointing_enable()

    def add_codebook_tokens(self, num_codebooks: int, codebook_size: int):
        """Append <Ci_j> special tokens and resize embeddings
        (ref lcrec.py:48-60)."""
        new_tokens = [f"<C{i}_{j}>" for i in range(num_codebooks)
                      for j in range(codebook_size)]
        num_added = self.tokenizer.add_special_tokens(
            {"additional_special_tokens": new_tokens})
        if num_added > 0:
            self.model.resize_token_embeddings(len(self.tokenizer))
            self.model.config.vocab_size = len(self.tokenizer)

    def codebook_token_ids(self, num_codebooks: int,
                           codebook_size: int) -> torch.Tensor:
        """[C, V] token ids of the codebook special tokens."""
        ids = [[self.tokenizer.convert_tokens_to_ids(f"<C{i}_{j}>")
                for j in range(codebook_size)] for i in range(num_codebooks)]
        return torch.tensor(ids, dtype=torch.long)

    def tokenize(self, prompt: str, *args, **kwargs):
        return self.tokenizer(prompt, *args, **kwargs)

    def decode(self, ids: torch.Tensor, *args, **kwargs) -> str:
        return self.tokenizer.decode(ids, *args, **kwargs)

    def tokenize_sft_format(self, prompt: str, response: str = "",
                            device=torch.device("cpu")) -> Dict:
        prompt_ids = self.tokenizer(prompt).input_ids
        response_ids = self.tokenizer(response).input_ids
        input_ids = prompt_ids + response_ids + [self.tokenizer.eos_token_id]
        t = torch.LongTensor([input_ids]).to(device)
        return {"input_ids": t, "prompt_seq_length": len(prompt_ids),
                "attention_mask": torch.ones_like(t)}

    def _lce_parts(self):
        """(backbone, lm_head) when the wrapped model exposes them in the
        plain causal-LM layout, else None (a PEFT wrapper, a biased head)."""
        from transformers import PreTrainedModel

        backbone = getattr(self.model, "model", None)
        head = getattr(self.model, "lm_head", None)
        # a PEFT wrapper forwards .model to the wrapped causal LM itself,
        # so only a bare transformers model is taken apart
        if isinstance(self.model, PreTrainedModel) \
                and isinstance(backbone, nn.Module) \
                and not hasattr(backbone, "lm_head") \
                and isinstance(head, nn.Linear) and head.bias is None:
            return backbone, head
        if not self._lce_fallback_logged:
            self._lce_fallback_logged = True
            logger.warning(
                "loss_implementation='genrec_lce' needs .model and a "
                "bias-free .lm_head on %s; using the backbone's own loss",
                type(self.model).__name__)
        return None

    def _packed_kwargs(self, input_ids, position_ids, cu_seq_lens,
                       max_length) -> Dict:
        """Backbone kwargs of a packed [1,T] row: attention is confined to
        each sequence by the genrec_gqa adapter through transformers' own
        cu_seq_lens_* / max_length_* names; no [1,1,T,T] mask is built."""
        if self.attn_implementation != "genrec_gqa":
            raise ValueError(
                'cu_seq_lens (packed sequences) requires '
                'attn_implementation="genrec_gqa", got '
                f"{self.attn_implementation!r}")
        if input_ids.dim() != 2 or input_ids.size(0) != 1:
            raise ValueError("cu_seq_lens (packed sequences) needs input_ids "
                             f"[1,T], got {tuple(input_ids.shape)}")
        if position_ids is None:
            raise ValueError("cu_seq_lens (packed sequences) needs "
                             "position_ids that restart at every sequence")
        cu = cu_seq_lens.to(device=input_ids.device, dtype=torch.int32)
        max_length = int(max_length) if max_length else input_ids.size(1)
        return dict(attention_mask={"full_attention": None},
                    position_ids=position_ids, use_cache=False,
                    cu_seq_lens_q=cu, cu_seq_lens_k=cu,
                    max_length_q=max_length, max_length_k=max_length)

    def forward(self, input_ids, attention_mask=None, labels=None,
                position_ids=None, cu_seq_lens=None, max_length=None, **kw):
        """cu_seq_lens (int32 [S+1]) marks input_ids [1,T] as S packed
        sequences with position_ids restarting at each and max_length >=
        the longest; attention_mask is then unused. It needs
        attn_implementation="genrec_gqa"."""
        if cu_seq_lens is not None:
            extra = self._packed_kwargs(input_ids, position_ids, cu_seq_lens,
                                        max_length)
        else:
            extra = {"attention_mask": attention_mask}
            if position_ids is not None:
                extra["position_ids"] = position_ids
        if labels is not None and self.loss_implementation == "genrec_lce":
            parts = self._lce_parts()
            if parts is not None:
                return self._forward_lce(parts, input_ids, labels, extra)
        return self.model(input_ids=input_ids, labels=labels, **extra)

    def _forward_lce(self, parts, input_ids, labels, extra):
        from transformers.modeling_outputs import CausalLMOutputWithPast

        from genrec_amd import ops

        backbone, head = parts
        hidden = backbone(input_ids=input_ids, **extra).last_hidden_state
        # the causal-LM shift: position i is scored against token i+1
        shifted = F.pad(labels, (0, 1), value=-100)[..., 1:]
        loss = ops.linear_cross_entropy(
            hidden.reshape(-1, hidden.size(-1)), head.weight,
            shifted.reshape(-1), ignore_index=-100)
        return CausalLMOutputWithPast(loss=loss, logits=None)

    def apply_lora(self, **kw) -> int:
        """Freeze the backbone and wrap its projections in LoRA adapters
        (genrec_amd.modules.lora.apply_lora; same keyword arguments).
        Returns the number of wrapped modules."""
        from genrec_amd.modules import lora

        wrapped = lora.apply_lora(self.model, **kw)
        self.lora_config = lora.lora_config(self.model)
        return wrapped

    def save_pretrained(self, save_dir: str, **kwargs):
        """With adapters on, the checkpoint is the merged model in the plain
        transformers layout (load_pretrained and eval_only read it as any
        other) and the adapter files are written next to it."""
        from genrec_amd.modules import lora

        if lora.lora_config(self.model) is not None:
            self.model.save_pretrained(
                save_dir, state_dict=lora.merged_state_dict(self.model),
                **kwargs)
            lora.save_adapter(self.model, save_dir)
            self.tokenizer.save_pretrained(save_dir)
            return
        self.model.save_pretrained(save_dir, **kwargs)
        self.tokenizer.save_pretrained(save_dir)

    def load_pretrained(self, load_dir: str):
        from transformers import AutoModelForCausalLM, AutoTokenizer

        self.tokenizer = AutoTokenizer.from_pretrained(load_dir)
        self.model = AutoModelForCausalLM.from_pretrained(
            load_dir, torch_dtype=torch.bfloat16,
            **_attn_kwargs(self.attn_implementation))
        _apply_layer_implementation(self.model, self.layer_implementation)
        logger.info("Loaded checkpoint from %s", load_dir)

    @torch.no_grad()
    def generate_topk(
        self,
        input_ids: torch.Tensor,      # [B, L] (left-padded)
        attention_mask: Optional[torch.Tensor] = None,
        max_new_tokens: int = 3,
        beam_width: int = 10,
        topk: Optional[int] = None,
        allowed_token_ids: Optional[List[torch.Tensor]] = None,
        allowed_token_fn: Optional[Callable[[int], bool]] = None,
        eos_token_id: Optional[int] = None,
        temperature: float = 1.0,
        beam_cache: Optional[str] = None,
        prefill: Optional[str] = None,
    ) -> List[List[Tuple[torch.Tensor, float]]]:
        """Batched KV-cached constrained beam search.

        beam_cache: None expands the prefill's KV cache W times and
        reorders all of it after every step; "shared_prefix" keeps one copy
        of the prompt's K/V per prompt plus per-beam suffix slots and a
        lineage table (SharedPrefixBeamCache) and runs each decode step's
        attention through ops.beam_decode_attention. It needs
        attn_implementation="genrec_gqa" and max_new_tokens <= 16.

        prefill: None prefills the left-padded batch as given. "packed"
        (with beam_cache="shared_prefix") drops the pads on the device: the
        real tokens of all prompts run as one [1,T] row with restarting
        position ids (ops.gqa_varlen_attention), the cache keeps the
        token-major K/V (SharedPrefixBeamCache.from_packed_prefill) and the
        decode steps read each prompt's own length through
        ops.beam_decode_varlen_attention. Arguments and return value are
        the same; every prompt needs at least one real token.

        allowed_token_ids: per-step 1-D tensors of legal token ids (the
        device-mask replacement for the reference's per-token Python
        callable); allowed_token_fn is still honored for parity when
        given (applied as a precomputed vocab mask).
        """
        from transformers import DynamicCache

        if beam_cache not in BEAM_CACHES:
            raise ValueError(f"beam_cache {beam_cache!r}: expected one of "
                             f"{BEAM_CACHES}")
        if prefill not in PREFILLS:
            raise ValueError(f"prefill {prefill!r}: expected one of "
                             f"{PREFILLS}")
        if prefill == "packed":
            if beam_cache != "shared_prefix":
                raise ValueError(
                    'prefill="packed" requires beam_cache="shared_prefix", '
                    f"got {beam_cache!r}")
            if self.attn_implementation != "genrec_gqa":
                raise ValueError(
                    'prefill="packed" requires '
                    'attn_implementation="genrec_gqa", got '
                    f"{self.attn_implementation!r}")
        if beam_cache == "shared_prefix":
            from genrec_amd.ops.attention import BEAM_MAX_SUFFIX

            if self.attn_implementation != "genrec_gqa":
                raise ValueError(
                    'beam_cache="shared_prefix" requires '
                    'attn_implementation="genrec_gqa", got '
                    f"{self.attn_implementation!r}")
            if max_new_tokens > BEAM_MAX_SUFFIX:
                raise ValueError(
                    'beam_cache="shared_prefix" supports max_new_tokens <= '
                    f"{BEAM_MAX_SUFFIX}, got {max_new_tokens}")

        device = input_ids.device
        B, L = input_ids.shape
        W = beam_width
        topk = topk or beam_width
        eos = eos_token_id if eos_token_id is not None \
            else self.tokenizer.eos_token_id
        V = self.model.config.vocab_size
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)

        fn_mask = None
        if allowed_token_fn is not None:
            keep = [allowed_token_fn(t) for t in range(V)]
            fn_mask = torch.tensor(keep, dtype=torch.bool, device=device)

        # prefill once per batch row; decode(last, step) -> [B*W, V] logits
        # of one step, hop(parent) moves the cache to the surviving beams
        cache = DynamicCache()
        if prefill == "packed":
            from genrec_amd.modules.hf_attention import SharedPrefixBeamCache

            # the real tokens of every prompt as one row; offsets, ids and
            # restarting positions are built on the device (the boolean
            # gather is the one sync: T is the backbone's input shape)
            real = attention_mask.bool()
            lens = real.sum(dim=1)                            # [B]
            cu = F.pad(lens.cumsum(0), (1, 0)).to(torch.int32)
            flat_ids = input_ids[real].unsqueeze(0)           # [1, T]
            flat_pos = (real.long().cumsum(1) - 1)[real].unsqueeze(0)
            kw = self._packed_kwargs(flat_ids, flat_pos, cu, L)
            kw["use_cache"] = True
            out = self.model(input_ids=flat_ids, past_key_values=cache,
                             logits_to_keep=cu[1:].long() - 1, **kw)
            logits = out.logits[0] / temperature              # [B, V]
            # L bounds every prompt's length without reading lens
            beams = SharedPrefixBeamCache.from_packed_prefill(
                cache, cu, L, W, max(max_new_tokens - 1, 1))
            beam_len = lens.repeat_interleave(W).unsqueeze(1)  # [B*W, 1]

            def decode(last: torch.Tensor, step: int) -> torch.Tensor:
                out = self.model(input_ids=last,
                                 attention_mask={"full_attention": None},
                                 position_ids=beam_len + (step - 1),
                                 past_key_values=beams,
                                 use_cache=True, logits_to_keep=1,
                                 genrec_beam_state=beams)
                return out.logits[:, -1, :]

            hop = beams.advance
        elif beam_cache == "shared_prefix":
            from genrec_amd.modules.hf_attention import SharedPrefixBeamCache

            out = self.model(input_ids=input_ids,
                             attention_mask=attention_mask,
                             past_key_values=cache, use_cache=True,
                             logits_to_keep=1)
            logits = out.logits[:, -1, :] / temperature      # [B, V]
            beams = SharedPrefixBeamCache.from_prefill(
                cache, W, max(max_new_tokens - 1, 1),
                pre_pad=attention_mask == 0)

            def decode(last: torch.Tensor, step: int) -> torch.Tensor:
                # the position the expanded cache's length would give: pads
                # counted, the same for every beam
                pos = torch.full((1, 1), L + step - 1, dtype=torch.long,
                                 device=device)
                out = self.model(input_ids=last,
                                 attention_mask={"full_attention": None},
                                 position_ids=pos, past_key_values=beams,
                                 use_cache=True, logits_to_keep=1,
                                 genrec_beam_state=beams)
                return out.logits[:, -1, :]

            hop = beams.advance
        else:
            out = self.model(input_ids=input_ids,
                             attention_mask=attention_mask,
                             past_key_values=cache, use_cache=True)
            logits = out.logits[:, -1, :] / temperature      # [B, V]
            if hasattr(cache, "batch_repeat_interleave"):
                cache.batch_repeat_interleave(W)
            else:  # older transformers: expand via legacy tuples
                idx = torch.arange(B, device=device).repeat_interleave(W)
                legacy = tuple(
                    (k.index_select(0, idx), v.index_select(0, idx))
                    for k, v in cache.to_legacy_cache())
                cache = DynamicCache.from_legacy_cache(legacy)
            attn = attention_mask.repeat_interleave(W, dim=0)  # [B*W, L]

            def decode(last: torch.Tensor, step: int) -> torch.Tensor:
                nonlocal attn
                attn = torch.cat([attn, torch.ones(
                    B * W, 1, dtype=attn.dtype, device=device)], dim=1)
                out = self.model(input_ids=last, attention_mask=attn,
                                 past_key_values=cache, use_cache=True)
                return out.logits[:, -1, :]

            def hop(parent: torch.Tensor) -> None:
                nonlocal attn
                flat_parent = (torch.arange(B, device=device).unsqueeze(1)
                               * W + parent).reshape(-1)
                cache.reorder_cache(flat_parent)
                attn = attn.index_select(0, flat_parent)

        def legal(step_logits: torch.Tensor, step: int) -> torch.Tensor:
            lp = F.log_softmax(step_logits, dim=-1)
            mask = torch.zeros(V, dtype=torch.bool, device=device)
            if allowed_token_ids is not None and step < len(allowed_token_ids):
                mask[allowed_token_ids[step].to(device)] = True
            else:
                mask[:] = True
            if fn_mask is not None:
                mask &= fn_mask
            return lp.masked_fill(~mask, float("-inf"))

        lp0 = legal(logits, 0)                                # [B, V]
        first_scores, first_tok = torch.topk(lp0, W, dim=-1)  # [B, W]
        beam_scores = first_scores.clone()                    # [B, W]
        beam_tokens = first_tok.unsqueeze(-1)                 # [B, W, 1]
        finished = first_tok == eos                           # [B, W]

        for step in range(1, max_new_tokens):
            if bool(finished.all()):
                break
            last = beam_tokens[:, :, -1].reshape(B * W, 1)
            logits = decode(last, step) / temperature         # [B*W, V]
            lp = legal(logits, step).view(B, W, V)
            # finished beams keep their score and emit only eos
            lp = torch.where(
                finished.unsqueeze(-1),
                torch.full_like(lp, float("-inf")).scatter(
                    -1, torch.full((B, W, 1), eos, dtype=torch.long,
                                   device=device), 0.0),
                lp)
            total = beam_scores.unsqueeze(-1) + lp            # [B, W, V]
            flat = total.view(B, W * V)
            beam_scores, pos = torch.topk(flat, W, dim=-1)
            parent = pos // V                                 # [B, W]
            tok = pos % V
            beam_tokens = torch.cat([
                beam_tokens.gather(1, parent.unsqueeze(-1).expand(
                    B, W, beam_tokens.size(-1))),
                tok.unsqueeze(-1),
            ], dim=-1)
            finished = finished.gather(1, parent) | (tok == eos)
            hop(parent)

        results: List[List[Tuple[torch.Tensor, float]]] = []
        for b in range(B):
            order = beam_scores[b].argsort(descending=True)
            row = []
            for w in order[:topk].tolist():
                seq = torch.cat([input_ids[b], beam_tokens[b, w]])
                row.append((seq, float(beam_scores[b, w])))
            results.append(row)
        return results
