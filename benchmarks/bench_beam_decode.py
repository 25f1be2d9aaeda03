"""A/B benchmark of the two beam-search KV caches of LCRec.generate_topk.

  default        the prefill cache expanded W times; every decode step runs
                 gqa_flash_attention on [B*W, Hkv, Lp+t, D] and then gathers
                 all of K and V along the batch (reorder_cache)
  shared_prefix  one prompt copy + per-beam suffix slots + a lineage table;
                 every decode step runs ops.beam_decode_attention

Part 1 (kernel level, one layer): per-step attention time of both paths,
the default path's per-step K/V reorder, and a sweep of the prefix split
count of beam_attn_fwd. Median over repeats of the mean over iters (device
events, variants alternating inside each repeat), min and max alongside.

Part 2 (model level): generate_topk wall time and peak allocation above the
resident model, both paths, on a random-init Qwen2.5-1.5B-shaped backbone.

Mixed-length case (both parts): the prompt lengths come from a fixed seeded
mix and are left-padded to Lp. Kernel pair: beam_decode_attention with the
pad mask against beam_decode_varlen_attention on the packed real tokens;
generate_topk: shared_prefix against shared_prefix + prefill="packed". Rows
carry the real-token share of the mix.

Shapes: the LCRec evaluation recipe (B=32, W=10, Lp=512, Hq/Hkv=12/2,
D=128) and serving batch 1.

Usage: python benchmarks/bench_beam_decode.py [--iters N] [--repeats R]
       [--layers N] [--skip-model] [--cases full,mixed]
       [--out results.jsonl]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from genrec_amd import ops  # noqa: E402

W, LP, HQ, HKV, D, T_SLOTS, T_LIVE = 10, 512, 12, 2, 128, 4, 3
BATCHES = {"recipe": 32, "batch1": 1}
SPLITS = (1, 2, 4, 8)


def _time(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms


def _stats(xs):
    return dict(ms=statistics.median(xs), ms_min=min(xs), ms_max=max(xs))


def bench_attention(name, B, dev, iters, repeats):
    g = torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)

    scale = D ** -0.5
    q = rnd(B * W, 1, HQ, D).transpose(1, 2)
    k_pre, v_pre = rnd(B, HKV, LP, D), rnd(B, HKV, LP, D)
    k_suf, v_suf = rnd(B, T_SLOTS, W, HKV, D), rnd(B, T_SLOTS, W, HKV, D)
    anc = torch.randint(0, W, (B, W, T_SLOTS), generator=g,
                        dtype=torch.int32).to(dev)
    assert ops.beam_decode_supported(q, k_pre, v_pre, k_suf, v_suf, anc)
    # what the default path holds at the same step
    k_exp, v_exp, _ = ops.eager.beam_kv_expand(k_pre, v_pre, k_suf, v_suf,
                                               anc, T_LIVE)
    k_exp, v_exp = k_exp.contiguous(), v_exp.contiguous()
    parent = (torch.arange(B, device=dev)[:, None] * W
              + torch.randint(0, W, (B, W), generator=g).to(dev)).reshape(-1)

    def beam(splits):
        return lambda: ops.beam_decode_attention(
            q, k_pre, v_pre, k_suf, v_suf, anc, T_LIVE, scale=scale,
            _splits=splits)

    variants = {
        "default: gqa_flash_attention": lambda: ops.gqa_flash_attention(
            q, k_exp, v_exp, scale=scale, causal=True),
        "default: reorder K and V": lambda: (k_exp.index_select(0, parent),
                                             v_exp.index_select(0, parent)),
        "shared_prefix: beam_decode_attention": beam(0),
    }
    for s in SPLITS:
        variants[f"shared_prefix: _splits={s}"] = beam(s)
    times = {n: [] for n in variants}
    with torch.no_grad():
        for fn in variants.values():
            for _ in range(10):
                fn()
        for _ in range(repeats):
            for n, fn in variants.items():
                times[n].append(_time(fn, iters))
    picked = ops.ext().beam_attn_pick_splits(B, HKV, W * (HQ // HKV), LP)
    rows = []
    for n in variants:
        rows.append(dict(part="attention_step", shape=name, variant=n, B=B,
                         W=W, Lp=LP, Hq=HQ, Hkv=HKV, D=D, t=T_LIVE,
                         picked_splits=picked, iters=iters, repeats=repeats,
                         **_stats(times[n])))
    return rows


def mixed_lengths(B):
    """Prompt lengths of the mixed case: 70 % short (32..256), 30 % long
    (257..Lp), fixed seed."""
    g = torch.Generator(device="cpu").manual_seed(1234)
    short = torch.randint(32, 257, (B,), generator=g)
    long_ = torch.randint(257, LP + 1, (B,), generator=g)
    return torch.where(torch.rand(B, generator=g) < 0.7, short, long_)


def bench_attention_mixed(name, B, dev, iters, repeats):
    g = torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)

    scale = D ** -0.5
    lens = mixed_lengths(B)
    share = float(lens.sum()) / (B * LP)
    q = rnd(B * W, 1, HQ, D).transpose(1, 2)
    k_pre, v_pre = rnd(B, HKV, LP, D), rnd(B, HKV, LP, D)
    k_suf, v_suf = rnd(B, T_SLOTS, W, HKV, D), rnd(B, T_SLOTS, W, HKV, D)
    anc = torch.randint(0, W, (B, W, T_SLOTS), generator=g,
                        dtype=torch.int32).to(dev)
    real = (torch.arange(LP)[None, :] >= (LP - lens)[:, None]).to(dev)
    pad = ~real                                          # left padding
    # the same real tokens, token-major as a packed prefill leaves them:
    # [1,Hkv,T,D] storage seen as [T,Hkv,D]
    k_pk = k_pre.transpose(1, 2)[real].transpose(0, 1).contiguous() \
        .transpose(0, 1)
    v_pk = v_pre.transpose(1, 2)[real].transpose(0, 1).contiguous() \
        .transpose(0, 1)
    cu = torch.nn.functional.pad(lens.cumsum(0), (1, 0)).to(torch.int32) \
        .to(dev)
    assert ops.beam_decode_supported(q, k_pre, v_pre, k_suf, v_suf, anc)
    assert ops.beam_decode_varlen_supported(q, k_pk, v_pk, cu, k_suf, v_suf,
                                            anc)
    variants = {
        "shared_prefix: beam_decode_attention + pre_pad":
            lambda: ops.beam_decode_attention(
                q, k_pre, v_pre, k_suf, v_suf, anc, T_LIVE, pre_pad=pad,
                scale=scale),
        "packed: beam_decode_varlen_attention":
            lambda: ops.beam_decode_varlen_attention(
                q, k_pk, v_pk, cu, LP, k_suf, v_suf, anc, T_LIVE,
                scale=scale),
    }
    times = {n: [] for n in variants}
    with torch.no_grad():
        for fn in variants.values():
            for _ in range(10):
                fn()
        for _ in range(repeats):
            for n, fn in variants.items():
                times[n].append(_time(fn, iters))
    return [dict(part="attention_step_mixed", shape=name, variant=n, B=B,
                 W=W, Lp=LP, Hq=HQ, Hkv=HKV, D=D, t=T_LIVE,
                 real_token_share=share, iters=iters, repeats=repeats,
                 **_stats(times[n])) for n in variants]


def bench_model_mixed(name, B, model, dev, repeats):
    ids = torch.randint(0, 256, (B, LP),
                        generator=torch.Generator().manual_seed(1)).to(dev)
    lens = mixed_lengths(B)
    attn = (torch.arange(LP)[None, :] >= (LP - lens)[:, None]).long().to(dev)
    cb = model.codebook_token_ids(4, 256)
    allowed = [cb[i] for i in range(4)]
    wall = {None: [], "packed": []}
    peak = {}

    def run(prefill):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.generate_topk(ids, attention_mask=attn, max_new_tokens=4,
                            beam_width=W, allowed_token_ids=allowed,
                            beam_cache="shared_prefix", prefill=prefill)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for prefill in wall:                    # warm-up, and the peak
        run(prefill)
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        run(prefill)
        peak[prefill] = torch.cuda.max_memory_allocated() - before
    for _ in range(repeats):
        for prefill in wall:
            wall[prefill].append(run(prefill))
    return [dict(part="generate_topk_mixed", shape=name,
                 variant="shared_prefix" + (" + packed" if prefill else ""),
                 B=B, W=W, Lp=LP, max_new_tokens=4,
                 layers=model.model.config.num_hidden_layers,
                 real_token_share=float(lens.sum()) / (B * LP),
                 peak_mib=peak[prefill] / 2**20, repeats=repeats,
                 **_stats(wall[prefill])) for prefill in wall]


def bench_model(name, B, model, dev, repeats):
    ids = torch.randint(0, 256, (B, LP),
                        generator=torch.Generator().manual_seed(1)).to(dev)
    cb = model.codebook_token_ids(4, 256)
    allowed = [cb[i] for i in range(4)]
    rows = []
    wall = {None: [], "shared_prefix": []}
    peak = {}

    def run(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.generate_topk(ids, max_new_tokens=4, beam_width=W,
                            allowed_token_ids=allowed, beam_cache=mode)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for mode in wall:                       # warm-up, and the peak
        run(mode)
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        run(mode)
        peak[mode] = torch.cuda.max_memory_allocated() - before
    for _ in range(repeats):
        for mode in wall:
            wall[mode].append(run(mode))
    for mode in wall:
        rows.append(dict(part="generate_topk", shape=name,
                         variant=mode or "default", B=B, W=W, Lp=LP,
                         max_new_tokens=4,
                         layers=model.model.config.num_hidden_layers,
                         peak_mib=peak[mode] / 2**20, repeats=repeats,
                         **_stats(wall[mode])))
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--layers", type=int, default=28)
    p.add_argument("--skip-model", action="store_true")
    p.add_argument("--cases", default="full,mixed",
                   help="comma list of: full (every prompt Lp long), mixed")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    cases = set(args.cases.split(","))
    assert cases and cases <= {"full", "mixed"}, args.cases
    att = [f for c, f in (("full", bench_attention),
                          ("mixed", bench_attention_mixed)) if c in cases]
    mod = [f for c, f in (("full", bench_model),
                          ("mixed", bench_model_mixed)) if c in cases]
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    rows = []
    for name, B in BATCHES.items():
        for fn in att:
            for row in fn(name, B, dev, args.iters, args.repeats):
                print(json.dumps(row), flush=True)
                rows.append(row)
    if not args.skip_model:
        from genrec_amd.models.lcrec import LCRec, default_qwen_config

        torch.manual_seed(0)
        model = LCRec(config=default_qwen_config(num_layers=args.layers),
                      attn_implementation="genrec_gqa")
        model.add_codebook_tokens(4, 256)
        model = model.to(torch.bfloat16).to(dev).eval()
        for name, B in BATCHES.items():
            for fn in mod:
                for row in fn(name, B, model, dev, args.repeats):
                    print(json.dumps(row), flush=True)
                    rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
