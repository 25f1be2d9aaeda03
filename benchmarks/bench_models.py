#!/usr/bin/env python3
"""Per-model training-step benchmarks (BASELINE.json configs 1-3, 5).

Measures train samples/sec for SASRec / HSTU / RQ-VAE (reference shipped
configs, synthetic data, random init) and a scaled LCRec SFT step. The
flagship TIGER benchmark lives in bench.py (the driver contract); this
harness provides the per-model evidence table.

Usage: python benchmarks/bench_models.py [--models sasrec,hstu,rqvae,lcrec]
       [--steps K] [--warmup W] [--out results.jsonl]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timeit(step, steps, warmup, device):
    for i in range(warmup):
        step(i)
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    if device.type == "cuda":
        torch.cuda.synchronize()
    return time.perf_counter() - t0


def _graph_step(model, batch, loss_getter, device, betas=(0.9, 0.999),
                use_graph=True):
    """hipGraph-captured full step on CUDA (the trainers' production
    path); eager AdamW fallback elsewhere. use_graph=False keeps the fused
    flat AdamW but launches the step eagerly."""
    if device.type == "cuda":
        from genrec_amd.parallel.graph_runner import GraphedTrainStep

        runner = GraphedTrainStep(model, batch, loss_getter, lr=1e-3,
                                  betas=betas, weight_decay=0.0,
                                  clip_norm=None, world=1,
                                  use_graph=use_graph)
        return lambda i: runner.step(batch)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, betas=betas)

    def step(i):
        opt.zero_grad(set_to_none=False)
        loss_getter(model(**batch)).backward()
        opt.step()

    return step


def bench_sasrec(device, steps, warmup):
    """SASRec: B=128, L=50, D=64, H=2, 2 blocks, V=12101 (sasrec/amazon.gin),
    graph-captured step on GPU."""
    from genrec_amd.models.sasrec import SASRec

    torch.manual_seed(0)
    B, L, V = 128, 50, 12101
    model = SASRec(num_items=V - 1, max_seq_len=L, embed_dim=64, num_heads=2,
                   num_blocks=2, ffn_dim=256, dropout=0.2).to(device)
    ids = torch.randint(1, V, (B, L), device=device)
    ids[::4, :20] = 0
    model.train()
    step = _graph_step(model, {"input_ids": ids, "targets": ids},
                       lambda out: out[1], device, betas=(0.9, 0.98))

    el = _timeit(step, steps, warmup, device)
    return dict(model="sasrec-amazon-beauty", batch=B,
                samples_per_s=B * steps / el,
                ms_per_step=el / steps * 1e3, hip_graph=device.type == "cuda")


def bench_hstu(device, steps, warmup):
    """HSTU bf16: B=128, L=50, D=64, H=2 + temporal bias (hstu/amazon.gin)."""
    from genrec_amd.models.hstu import HSTU

    torch.manual_seed(0)
    B, L, V = 128, 50, 12101
    model = HSTU(num_items=V - 1, max_seq_len=L, embed_dim=64, num_heads=2,
                 num_blocks=2, dropout=0.2, use_temporal_bias=True).to(device)
    ids = torch.randint(1, V, (B, L), device=device)
    ts = (torch.arange(L, device=device) * 86400 + 10 ** 9).unsqueeze(0) \
        .expand(B, -1).contiguous()
    model.train()
    step = _graph_step(
        model, {"input_ids": ids, "timestamps": ts, "targets": ids},
        lambda out: out[1], device, betas=(0.9, 0.98))

    el = _timeit(step, steps, warmup, device)
    return dict(model="hstu-amazon-beauty-bf16", batch=B,
                samples_per_s=B * steps / el,
                ms_per_step=el / steps * 1e3, hip_graph=device.type == "cuda")


def bench_rqvae(device, steps, warmup):
    """RQ-VAE: B=1024, 768->[512,256,128,64]->32, 3x256 codebooks,
    STE + Sinkhorn-last (tiger/amazon/rqvae.gin)."""
    from genrec_amd.models.rqvae import QuantizeForwardMode, RqVae

    torch.manual_seed(0)
    B = 1024
    model = RqVae(input_dim=768, embed_dim=32,
                  hidden_dims=[512, 256, 128, 64], codebook_size=256,
                  codebook_mode=QuantizeForwardMode.STE,
                  codebook_last_layer_mode=QuantizeForwardMode.SINKHORN,
                  n_layers=3, n_cat_features=0).to(device)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    x = torch.nn.functional.normalize(torch.randn(B, 768, device=device),
                                      dim=-1)
    model.train()
    model(x, gumbel_t=0.2)  # kmeans init outside the timed region

    def step(i):
        opt.zero_grad(set_to_none=False)
        out = model(x, gumbel_t=0.2)
        out.loss.backward()
        opt.step()

    el = _timeit(step, steps, warmup, device)
    return dict(model="rqvae-amazon-beauty", batch=B,
                samples_per_s=B * steps / el,
                ms_per_step=el / steps * 1e3)


def bench_lcrec(device, steps, warmup, full_size=False, attn_impl="sdpa",
                loss_impl="hf", vocab=None, response_tokens=None,
                eager_step=False, layer_impl="hf", lora="none"):
    """LCRec SFT step: Qwen2-1.5B-shaped backbone (lcrec/amazon/lcrec.gin:
    B=32, L=512, bf16, grad ckpt) — full size only on GPU. attn_impl selects
    the backbone attention ("sdpa" | "genrec_gqa") and loss_impl the loss
    ("hf" = the backbone's own | "genrec_lce") and layer_impl the decoder
    layer ("hf" = transformers' | "genrec_fused") for same-box A/Bs. `vocab`
    widens the head to a real tokenizer's size (the offline tokenizer is
    tiny); `response_tokens` supervises only the last K positions of each
    sample, as sft_collate does (default: every position, as before).
    `eager_step` launches the step without hipGraph capture, as
    lcrec_trainer does; only then can "genrec_lce" drop the unsupervised
    rows (the compaction needs one host sync). `lora` adapts the seven
    projections of every layer with the reference's defaults (r=16,
    alpha=32, dropout=0.05) and trains the adapters only: "genrec" through
    ops.lora_linear, "compose" through the stock op composition (dropout,
    two F.linear, scale, add); the step is then launched eagerly (the
    adapter dropout draws a host seed per call)."""
    from genrec_amd.models.lcrec import LCRec, default_qwen_config

    torch.manual_seed(0)
    if lora != "none":
        eager_step = True
    B, L = (32, 512) if full_size else (2, 64)
    cfg = default_qwen_config() if full_size else default_qwen_config(
        vocab_size=2048, hidden_size=256, num_layers=4, num_heads=8,
        num_kv_heads=2, intermediate_size=512)
    if vocab is not None:
        cfg.vocab_size = vocab
    model = LCRec(config=cfg, attn_implementation=attn_impl,
                  loss_implementation=None if loss_impl == "hf"
                  else loss_impl,
                  layer_implementation=None if layer_impl == "hf"
                  else layer_impl)
    model.add_codebook_tokens(5, 256)
    if vocab is not None:
        # add_codebook_tokens resized to the offline tokenizer's length
        model.model.resize_token_embeddings(vocab + 5 * 256)
        model.model.config.vocab_size = vocab + 5 * 256
    if lora != "none":
        model.apply_lora()
        if lora == "compose":
            from genrec_amd.modules.lora import LoRALinear

            composed = _composed_lora_class()
            for m in model.modules():
                if isinstance(m, LoRALinear):
                    m.__class__ = composed
    if full_size:
        model.gradient_checkpointing_enable()
    model = model.to(device)
    if device.type == "cuda":
        model = model.to(torch.bfloat16)
    V = model.model.config.vocab_size
    ids = torch.randint(0, V, (B, L), device=device)
    attn = torch.ones_like(ids)
    labels = ids
    if response_tokens is not None:
        labels = ids.clone()
        labels[:, :L - response_tokens] = -100
    model.train()
    # GraphedTrainStep: fused flat AdamW + steal-grads even when hipGraph
    # capture falls back to eager (HF checkpointing is not capture-safe)
    step = _graph_step(model,
                       {"input_ids": ids, "attention_mask": attn,
                        "labels": labels},
                       lambda out: out.loss, device,
                       use_graph=not eager_step)

    if device.type == "cuda":
        torch.cuda.reset_peak_memory_stats(device)
    el = _timeit(step, steps, warmup, device)
    peak = torch.cuda.max_memory_allocated(device) / 2**30 \
        if device.type == "cuda" else None
    return dict(model="lcrec-qwen2-1.5b" if full_size else "lcrec-tiny",
                attn=attn_impl, loss=loss_impl, layers=layer_impl, vocab=V,
                lora=lora,
                trainable_params=sum(p.numel() for p in model.parameters()
                                     if p.requires_grad),
                step="eager" if eager_step else "graph",
                supervised_per_sample=response_tokens or L,
                batch=B, seq_len=L, samples_per_s=B * steps / el,
                tokens_per_s=B * L * steps / el,
                ms_per_step=el / steps * 1e3, peak_hbm_gib=peak)


def _composed_lora_forward(self, x):
    """peft's op order: base(x) + lora_B(lora_A(dropout(x))) * scaling"""
    F = torch.nn.functional
    xd = F.dropout(x, self.lora_dropout, self.training)
    return self.base_layer(x) + self.lora_B(self.lora_A(xd)) * self.scaling


def _composed_lora_class():
    from genrec_amd.modules.lora import LoRALinear

    return type("_ComposedLoRALinear", (LoRALinear,),
                {"forward": _composed_lora_forward})


class _PackedStep(torch.nn.Module):
    """Binds the packed batch's host-side max_length, so that the step
    runner sees a batch of tensors only."""

    def __init__(self, model, max_length):
        super().__init__()
        self.model, self.max_length = model, max_length

    def forward(self, **batch):
        return self.model(max_length=self.max_length, **batch)


def bench_lcrec_packing(device, steps, warmup, full_size=False,
                        loss_impl="hf", vocab=None, layer_impl="hf",
                        rounds=3, **_):
    """Padded vs packed LCRec SFT step on the same 32 samples, whose
    lengths follow an SFT batch's mix (bench_gqa_attention.sft_length_mix)
    instead of fixed 512-token rows. Both run "genrec_gqa", eagerly (no
    hipGraph), on identically initialised models; the variants alternate
    for `rounds` rounds of `steps` steps and the median round is reported.
    The last 8 tokens of every sample are supervised."""
    import statistics

    from bench_gqa_attention import sft_length_mix
    from genrec_amd.models.lcrec import LCRec, default_qwen_config

    lens = sft_length_mix() if full_size else [5, 70, 33, 64]
    n, lmax, real = len(lens), max(lens), sum(lens)
    T = -(-real // 64) * 64

    def make():
        torch.manual_seed(0)
        cfg = default_qwen_config() if full_size else default_qwen_config(
            vocab_size=2048, hidden_size=256, num_layers=4, num_heads=4,
            num_kv_heads=2, intermediate_size=512)
        if vocab is not None:
            cfg.vocab_size = vocab
        m = LCRec(config=cfg, attn_implementation="genrec_gqa",
                  loss_implementation=None if loss_impl == "hf"
                  else loss_impl,
                  layer_implementation=None if layer_impl == "hf"
                  else layer_impl)
        m.add_codebook_tokens(5, 256)
        if vocab is not None:
            m.model.resize_token_embeddings(vocab + 5 * 256)
            m.model.config.vocab_size = vocab + 5 * 256
        if full_size:
            m.gradient_checkpointing_enable()
        m = m.to(device)
        if device.type == "cuda":
            m = m.to(torch.bfloat16)
        return m.train()

    m_pad, m_pack = make(), make()
    V = m_pad.model.config.vocab_size
    lt = torch.tensor(lens, device=device)
    valid = torch.arange(lmax, device=device)[None, :] < lt[:, None]
    ids = torch.randint(0, V, (n, lmax), device=device) * valid
    pos = torch.arange(lmax, device=device).expand(n, lmax)
    labels = ids.masked_fill(~(valid & (pos >= (lt[:, None] - 8))
                               & (pos > 0)), -100)
    p_ids = ids.new_zeros(1, T)
    p_lab = ids.new_full((1, T), -100)
    p_pos = ids.new_zeros(1, T)
    p_ids[0, :real], p_lab[0, :real], p_pos[0, :real] = \
        ids[valid], labels[valid], pos[valid]
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(),
                      dtype=torch.int32, device=device)
    run = {
        "padded": _graph_step(
            m_pad, {"input_ids": ids, "attention_mask": valid.long(),
                    "labels": labels},
            lambda out: out.loss, device, use_graph=False),
        "packed": _graph_step(
            _PackedStep(m_pack, lmax),
            {"input_ids": p_ids, "labels": p_lab, "position_ids": p_pos,
             "cu_seq_lens": cu},
            lambda out: out.loss, device, use_graph=False),
    }
    for name in run:
        _timeit(run[name], 0, warmup, device)
    ms = {name: [] for name in run}
    for _ in range(rounds):
        for name in run:
            ms[name].append(_timeit(run[name], steps, 0, device)
                            / steps * 1e3)
    med = {name: statistics.median(v) for name, v in ms.items()}
    return dict(model="lcrec-qwen2-1.5b" if full_size else "lcrec-tiny",
                attn="genrec_gqa", loss=loss_impl, layers=layer_impl,
                vocab=V, step="eager", samples=n, real_tokens=real,
                padded_tokens=n * lmax, packed_tokens=T, max_len=lmax,
                padded_ms_per_step=med["padded"],
                packed_ms_per_step=med["packed"],
                padded_ms_rounds=ms["padded"], packed_ms_rounds=ms["packed"],
                packed_speedup=med["padded"] / med["packed"],
                samples_per_s=n / med["packed"] * 1e3,
                ms_per_step=med["packed"], rounds=rounds)


def bench_cobra(device, steps, warmup):
    """COBRA train step (config/cobra/amazon.gin: B=32, C=3, d_model=384,
    6 heads, 4 layers, T=20 items -> interleaved L=80 on the flash
    attention path), bf16 autocast."""
    from genrec_amd.models.cobra import Cobra

    torch.manual_seed(0)
    B, T, Ltxt = 32, 20, 64
    model = Cobra(encoder_n_layers=2, encoder_hidden_dim=384,
                  encoder_num_heads=6, encoder_vocab_size=32128,
                  id_vocab_size=256, n_codebooks=3, d_model=384,
                  decoder_n_layers=4, decoder_num_heads=6,
                  decoder_dropout=0.1).to(device)
    ids = torch.randint(0, 256, (B, T * 3), device=device)
    enc = torch.randint(1, 32128, (B, T, Ltxt), device=device)
    model.train()
    model.static_infonce = device.type == "cuda"  # capture-safe variant
    step = _graph_step(
        model, {"input_ids": ids, "encoder_input_ids": enc},
        lambda out: out.loss_sparse + out.loss_dense, device)

    el = _timeit(step, steps, warmup, device)
    return dict(model="cobra-amazon-beauty", batch=B,
                samples_per_s=B * steps / el,
                ms_per_step=el / steps * 1e3, hip_graph=device.type == "cuda")


BENCHES = {"sasrec": bench_sasrec, "hstu": bench_hstu, "rqvae": bench_rqvae,
           "lcrec": bench_lcrec, "cobra": bench_cobra}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="sasrec,hstu,rqvae")
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--lcrec-full", action="store_true")
    p.add_argument("--lcrec-attn", choices=["sdpa", "genrec_gqa"],
                   default="sdpa")
    p.add_argument("--lcrec-loss", choices=["hf", "genrec_lce"],
                   default="hf")
    p.add_argument("--lcrec-layers", choices=["hf", "genrec_fused"],
                   default="hf")
    p.add_argument("--lcrec-vocab", type=int, default=None,
                   help="backbone vocabulary before the codebook tokens "
                        "(Qwen2.5: 151936)")
    p.add_argument("--lcrec-response-tokens", type=int, default=None,
                   help="supervise only the last K positions per sample")
    p.add_argument("--lcrec-lora", choices=["none", "compose", "genrec"],
                   default="none",
                   help="LoRA adapters on the LCRec step (forces eager)")
    p.add_argument("--lcrec-eager", action="store_true",
                   help="no hipGraph capture of the LCRec step")
    p.add_argument("--lcrec-packing", action="store_true",
                   help="padded vs packed SFT step on one batch of mixed "
                        "lengths (genrec_gqa, eager step)")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    device = torch.device("cuda:0") if torch.cuda.is_available() \
        else torch.device("cpu")
    results = []
    for name in args.models.split(","):
        name = name.strip()
        kw = {}
        if name == "lcrec":
            kw["full_size"] = args.lcrec_full
            kw["attn_impl"] = args.lcrec_attn
            kw["loss_impl"] = args.lcrec_loss
            kw["layer_impl"] = args.lcrec_layers
            kw["vocab"] = args.lcrec_vocab
            kw["response_tokens"] = args.lcrec_response_tokens
            kw["eager_step"] = args.lcrec_eager
            kw["lora"] = args.lcrec_lora
        bench = BENCHES[name]
        if name == "lcrec" and args.lcrec_packing:
            bench = bench_lcrec_packing
        try:
            r = bench(device, args.steps, args.warmup, **kw)
        except Exception as e:  # keep other models running
            print(json.dumps({"model": name, "error": str(e)}), flush=True)
            continue
        r.update(device=str(device), steps=args.steps, warmup=args.warmup,
                 dtype="bf16" if device.type == "cuda" else "fp32",
                 data="synthetic")
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
