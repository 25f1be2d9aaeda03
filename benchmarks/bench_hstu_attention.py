"""A/B microbenchmark: ops.hstu_attention (tiled kernel, L > 64) against the
path an HSTU layer took for such lengths before it existed: position and
temporal bias tensors materialised from the tables ([H,L,L], [B,H,L,L]) and
hstu_pointwise_attention on them.

Shapes: L in {128, 256, 512, 1024, 2048} at B=32, H=2, D=32, bf16, one
left-padded quarter of the batch, timestamps one day apart. q/k/v are the
chunk views of one [B,L,4*H*D] projection, as the layer makes them. Per L
and variant: the median over repeats of the mean forward and
forward+backward time (device events, the two variants alternating inside
each repeat, every timed path warmed up first), the peak of allocated
memory over one forward+backward above what the inputs hold, and the
largest difference between the two variants' outputs.

Usage: python benchmarks/bench_hstu_attention.py [--iters N] [--repeats R]
       [--lengths 128,256,...] [--out results.jsonl]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from genrec_amd import ops  # noqa: E402
from genrec_amd.models.hstu import RelativePositionBias  # noqa: E402

B, H, D = 32, 2, 32
N_POS, N_TIME = 32, 64
LENGTHS = (128, 256, 512, 1024, 2048)


def _inputs(L, dev):
    g = torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape, scale=0.5):
        return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16) \
            .to(dev)

    proj = rnd(B, L, 4 * H * D).requires_grad_()
    pos_w = rnd(N_POS, H).requires_grad_()
    time_w = rnd(N_TIME, H).requires_grad_()
    ts = (torch.arange(L) * 86400 + 1_400_000_000).unsqueeze(0) \
        .expand(B, -1).contiguous().to(dev)
    pad = torch.zeros(B, L, dtype=torch.bool)
    pad[: B // 4, : L // 2] = True
    dout = rnd(B, L, H * D, scale=0.1)
    pos = RelativePositionBias(N_POS, 128, H)
    return dict(proj=proj, pos_w=pos_w, time_w=time_w, ts=ts,
                pad=pad.to(dev), dout=dout,
                rel=pos.rel_bucket_table(L, dev),
                bucket=pos.bucket_table(L, dev))


def _qkv(x):
    b, l, _ = x["proj"].shape
    _, v, q, k = (t.view(b, l, H, D).transpose(1, 2)
                  for t in x["proj"].chunk(4, dim=-1))
    return q, k, v


def _tiled(x):
    q, k, v = _qkv(x)
    out = ops.hstu_attention(q, k, v, x["rel"], x["pos_w"], x["time_w"],
                             x["ts"], x["pad"])
    return out.transpose(1, 2).reshape(out.size(0), out.size(2), H * D)


def _composed(x):
    """RelativePositionBias.forward + TemporalBias.forward +
    hstu_pointwise_attention, as HSTULayer composes them"""
    q, k, v = _qkv(x)
    pos_bias = ops.embedding(x["pos_w"], x["bucket"]).permute(2, 0, 1)
    ts = x["ts"]
    diff = ts.unsqueeze(2) - ts.unsqueeze(1)
    tb = (torch.log(torch.clamp(diff.abs(), min=1).float()) / 0.693).long() \
        .clamp(min=0, max=N_TIME - 1)
    time_bias = ops.embedding(x["time_w"], tb).permute(0, 3, 1, 2)
    out = ops.hstu_pointwise_attention(q, k, v, pos_bias, time_bias,
                                       x["pad"])
    return out.transpose(1, 2).reshape(out.size(0), out.size(2), H * D)


VARIANTS = {"hstu_attention_tiled": _tiled, "composed_bias_tensors": _composed}


def _time(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms


def _fwd(fn, x):
    with torch.no_grad():
        fn(x)


def _fwd_bwd(fn, x):
    fn(x).backward(x["dout"])
    x["proj"].grad = x["pos_w"].grad = x["time_w"].grad = None


def _peak_bytes(fn, x):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    _fwd_bwd(fn, x)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--lengths", default=",".join(str(n) for n in LENGTHS))
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    rows = []
    for L in (int(n) for n in args.lengths.split(",")):
        x = _inputs(L, dev)
        assert ops.hstu_flash_supported(*_qkv(x), x["pos_w"], x["time_w"]), \
            "the tiled kernel must take this shape"
        with torch.no_grad():
            outs = {n: fn(x).float() for n, fn in VARIANTS.items()}
        diff = (outs["hstu_attention_tiled"]
                - outs["composed_bias_tensors"]).abs().max().item()
        del outs
        for fn in VARIANTS.values():      # warm-up every timed path
            for _ in range(5):
                _fwd(fn, x)
                _fwd_bwd(fn, x)
        times = {n: {"fwd": [], "fwd_bwd": []} for n in VARIANTS}
        for _ in range(args.repeats):
            for n, fn in VARIANTS.items():
                times[n]["fwd"].append(_time(lambda: _fwd(fn, x), args.iters))
                times[n]["fwd_bwd"].append(
                    _time(lambda: _fwd_bwd(fn, x), args.iters))
        for n, fn in VARIANTS.items():
            row = dict(L=L, variant=n, B=B, H=H, D=D,
                       fwd_ms=statistics.median(times[n]["fwd"]),
                       fwd_bwd_ms=statistics.median(times[n]["fwd_bwd"]),
                       fwd_ms_min=min(times[n]["fwd"]),
                       fwd_ms_max=max(times[n]["fwd"]),
                       fwd_bwd_ms_min=min(times[n]["fwd_bwd"]),
                       fwd_bwd_ms_max=max(times[n]["fwd_bwd"]),
                       peak_mib=_peak_bytes(fn, x) / 2**20,
                       max_abs_diff_between_variants=diff,
                       iters=args.iters, repeats=args.repeats)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del x
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
