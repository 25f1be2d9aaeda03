"""A/B microbenchmark: gqa_flash_attention vs PyTorch bf16 SDPA with
expanded K/V (what the stock transformers `sdpa` path runs for Qwen2).

Shapes: the LCRec SFT prefill (B=8, Hq=12, Hkv=2, L=512, D=128) and the
beam-decode step (B=40, Lq=1, Lk=515). Reports, per variant, the median
over repeats of the mean forward and forward+backward time (device
events, alternating variants inside each repeat) and the bytes the
forward keeps alive for backward (output + saved tensors).

Packed rows ("sft_mix"): 32 samples with the length mix of an LCRec SFT
batch (sft_length_mix), once right-padded to the longest as
gqa_flash_attention takes them ([B,H,L,D] + key-pad mask) and once packed
into one [T,H,D] row for gqa_varlen_attention, same samples, same timing
scheme.

Usage: python benchmarks/bench_gqa_attention.py [--iters N] [--repeats R]
       [--out results.jsonl]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from genrec_amd import ops  # noqa: E402

SHAPES = {
    "prefill": dict(B=8, Hq=12, Hkv=2, Lq=512, Lk=512, D=128),
    "decode": dict(B=40, Hq=12, Hkv=2, Lq=1, Lk=515, D=128),
}


# quantiles of the sample length of an LCRec SFT batch (synthetic dataset
# defaults, offline tokenizer, max_len 512): min, median, p90, max
SFT_LENGTH_QUANTILES = ((0.0, 25), (0.5, 77), (0.9, 127), (1.0, 356))


def sft_length_mix(n=32, seed=0):
    """n sample lengths with the quantiles above (piecewise-linear inverse
    CDF at the n mid-points, the longest pinned to the maximum), shuffled."""
    lens = []
    for i in range(n):
        u = (i + 0.5) / n
        for (u0, l0), (u1, l1) in zip(SFT_LENGTH_QUANTILES,
                                      SFT_LENGTH_QUANTILES[1:]):
            if u <= u1:
                lens.append(round(l0 + (u - u0) / (u1 - u0) * (l1 - l0)))
                break
    lens[-1] = SFT_LENGTH_QUANTILES[-1][1]
    g = torch.Generator().manual_seed(seed)
    return [lens[i] for i in torch.randperm(n, generator=g).tolist()]


def _inputs(s, dev):
    g = torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)

    # q from a projection ([B,L,H,D] storage); k/v as a contiguous cache
    q = rnd(s["B"], s["Lq"], s["Hq"], s["D"]).transpose(1, 2)
    k = rnd(s["B"], s["Hkv"], s["Lk"], s["D"])
    v = rnd(s["B"], s["Hkv"], s["Lk"], s["D"])
    dout = rnd(s["B"], s["Lq"], s["Hq"], s["D"])
    return q, k, v, dout


def _gqa(q, k, v, scale):
    return ops.gqa_flash_attention(q, k, v, scale=scale, causal=True)


def _sdpa(q, k, v, scale):
    rep = q.size(1) // k.size(1)
    b, hkv, lk, d = k.shape
    ke = k[:, :, None].expand(b, hkv, rep, lk, d).reshape(b, hkv * rep, lk, d)
    ve = v[:, :, None].expand(b, hkv, rep, lk, d).reshape(b, hkv * rep, lk, d)
    out = F.scaled_dot_product_attention(q, ke, ve, scale=scale,
                                         is_causal=q.size(2) > 1)
    return out.transpose(1, 2).contiguous()


def _bench_sft_mix(dev, iters, repeats, hq=12, hkv=2, d=128):
    """Padded vs packed attention on the same 32 samples -> result rows."""
    lens = sft_length_mix()
    n, lmax, real = len(lens), max(lens), sum(lens)
    t = -(-real // 64) * 64
    scale = d ** -0.5
    g = torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)

    pq, pk, pv, pdo = (rnd(t, hq, d), rnd(t, hkv, d), rnd(t, hkv, d),
                       rnd(t, hq, d))
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(),
                      dtype=torch.int32, device=dev)
    # the same tokens, right-padded to the longest sample
    lt = torch.tensor(lens, device=dev)
    valid = torch.arange(lmax, device=dev)[None, :] < lt[:, None]

    def pad(x):
        out = x.new_zeros(n, lmax, *x.shape[1:])
        out[valid] = x[:real]
        return out

    bq, bk, bv, bdo = (pad(x) for x in (pq, pk, pv, pdo))
    key_pad = ~valid
    pg = [x.detach().requires_grad_() for x in (pq, pk, pv)]
    bg = [x.transpose(1, 2).detach().requires_grad_() for x in (bq, bk, bv)]

    def packed(q, k, v):
        return ops.gqa_varlen_attention(q, k, v, cu, lmax, scale=scale)

    def padded(q, k, v):
        return ops.gqa_flash_attention(q, k, v, key_pad_mask=key_pad,
                                       scale=scale, causal=True)

    variants = {"genrec_gqa_padded": (padded, bg, bdo),
                "genrec_gqa_varlen": (packed, pg, pdo)}

    def fwd(name):
        fn, xs, _ = variants[name]
        with torch.no_grad():
            fn(*xs)

    def fwd_bwd(name):
        fn, xs, dout = variants[name]
        fn(*xs).backward(dout)
        for x in xs:
            x.grad = None

    for name in variants:
        for _ in range(10):
            fwd(name)
            fwd_bwd(name)
    times = {name: {"fwd": [], "fwd_bwd": []} for name in variants}
    for _ in range(repeats):
        for name in variants:
            times[name]["fwd"].append(_time(lambda: fwd(name), iters))
            times[name]["fwd_bwd"].append(_time(lambda: fwd_bwd(name), iters))
    rows = []
    for name in variants:
        rows.append(dict(
            shape="sft_mix", variant=name, samples=n, Hq=hq, Hkv=hkv, D=d,
            real_tokens=real, padded_tokens=n * lmax, packed_tokens=t,
            max_len=lmax,
            fwd_ms=statistics.median(times[name]["fwd"]),
            fwd_bwd_ms=statistics.median(times[name]["fwd_bwd"]),
            fwd_ms_min=min(times[name]["fwd"]),
            fwd_ms_max=max(times[name]["fwd"]),
            fwd_bwd_ms_min=min(times[name]["fwd_bwd"]),
            fwd_bwd_ms_max=max(times[name]["fwd_bwd"]),
            iters=iters, repeats=repeats))
    return rows


def _time(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms


def _retained_bytes(fn, q, k, v, scale):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = fn(q, k, v, scale)
    torch.cuda.synchronize()
    kept = torch.cuda.memory_allocated() - before
    del out
    return kept


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    variants = {"genrec_gqa": _gqa, "sdpa_expanded": _sdpa}
    rows = []
    for sname, s in SHAPES.items():
        q, k, v, dout = _inputs(s, dev)
        scale = s["D"] ** -0.5
        qg, kg, vg = (t.detach().requires_grad_() for t in (q, k, v))

        def fwd(fn):
            with torch.no_grad():
                fn(q, k, v, scale)

        def fwd_bwd(fn):
            out = fn(qg, kg, vg, scale)
            out.backward(dout)
            qg.grad = kg.grad = vg.grad = None

        times = {n: {"fwd": [], "fwd_bwd": []} for n in variants}
        for n, fn in variants.items():      # warm-up every timed path
            for _ in range(10):
                fwd(fn)
                fwd_bwd(fn)
        for _ in range(args.repeats):
            for n, fn in variants.items():
                times[n]["fwd"].append(_time(lambda: fwd(fn), args.iters))
                times[n]["fwd_bwd"].append(
                    _time(lambda: fwd_bwd(fn), args.iters))
        for n, fn in variants.items():
            row = dict(shape=sname, variant=n, **s,
                       fwd_ms=statistics.median(times[n]["fwd"]),
                       fwd_bwd_ms=statistics.median(times[n]["fwd_bwd"]),
                       fwd_ms_min=min(times[n]["fwd"]),
                       fwd_ms_max=max(times[n]["fwd"]),
                       fwd_bwd_ms_min=min(times[n]["fwd_bwd"]),
                       fwd_bwd_ms_max=max(times[n]["fwd_bwd"]),
                       retained_mib=_retained_bytes(fn, qg, kg, vg, scale)
                       / 2**20,
                       iters=args.iters, repeats=args.repeats)
            print(json.dumps(row), flush=True)
            rows.append(row)
    for row in _bench_sft_mix(dev, args.iters, args.repeats):
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
