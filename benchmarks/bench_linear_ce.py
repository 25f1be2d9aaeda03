"""A/B microbenchmark: ops.linear_cross_entropy vs the stock LLM-head loss
(F.linear -> .float() -> F.cross_entropy, what transformers runs for
Qwen2ForCausalLM with labels), forward + backward, bf16.

Shapes: the LCRec SFT head, H=1536, V=153,216 (151,936 + 5x256 codebook
tokens), N=16,384 rows (B=32, L=512) with ~3 % of the rows supervised (a
handful of response tokens per sample) and with every row supervised.
Reports, per variant, the median over repeats of the mean forward+backward
time (device events, alternating variants inside each repeat) and the peak
allocation above the pre-call level. `--chunk-rows` sweeps the op's chunk
size (0 = its default). The last rows time the lce_stats + lce_grad kernel
pair alone on one chunk and give its share of the HBM peak from the bytes
it must move (read, read, write of the chunk).

Usage: python benchmarks/bench_linear_ce.py [--iters N] [--repeats R]
       [--chunk-rows 0,256,1752] [--rows 16384] [--out results.jsonl]
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
from genrec_amd.ops import eager  # noqa: E402

H, V = 1536, 151936 + 5 * 256
HBM_PEAK_BYTES_PER_S = 8.0e12      # MI355X HBM3E


def _inputs(n, frac, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    h = torch.randn(n, H, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(V, H, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    t = torch.randint(0, V, (n,), generator=g)
    if frac < 1.0:
        t[torch.rand(n, generator=g) >= frac] = -100
    return h.requires_grad_(), w.requires_grad_(), t.to(dev)


def _stock(h, w, t):
    return F.cross_entropy(F.linear(h, w).float(), t, ignore_index=-100)


def _time(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms


def _peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2**20


def _kernel_rows(dev, iters, repeats):
    """lce_stats + lce_grad alone on one default-sized chunk."""
    rows = []
    r = eager.lce_default_chunk_rows(1 << 20, V)
    g = torch.Generator(device="cpu").manual_seed(1)
    src = torch.randn(r, V, generator=g).to(torch.bfloat16).to(dev)
    work = torch.empty_like(src)
    t = torch.randint(0, V, (r,), generator=g).to(dev)
    inv_n = torch.full((1,), 1.0 / r, device=dev)
    for slices in (0, 1):
        def fn():
            work.copy_(src)
            ops.ext().lce_inplace(work, t, inv_n, -100, slices)

        def copy_only():
            work.copy_(src)

        for _ in range(3):
            fn()
        both = [_time(fn, iters) for _ in range(repeats)]
        copy = [_time(copy_only, iters) for _ in range(repeats)]
        ms = statistics.median(both) - statistics.median(copy)
        moved = 3 * r * V * 2
        rows.append(dict(
            case="kernel_pair", rows=r, vocab=V,
            slices=ops.ext().lce_pick_slices(r, V) if slices == 0 else slices,
            kernel_pair_ms=ms, bytes_moved=moved,
            gbytes_per_s=moved / ms / 1e6,
            share_of_hbm_peak=moved / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S))
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--rows", type=int, default=16384)
    p.add_argument("--chunk-rows", default="0")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    chunk_rows = [int(c) for c in args.chunk_rows.split(",")]
    rows = []
    for case, frac in (("sft_3pct", 0.03), ("all_rows", 1.0)):
        h, w, t = _inputs(args.rows, frac, dev)
        n_valid = int((t != -100).sum())

        def run(loss_fn):
            loss_fn().backward()
            h.grad = w.grad = None

        variants = {"stock": lambda: _stock(h, w, t)}
        for cr in chunk_rows:
            variants[f"genrec_lce[{cr or 'default'}]"] = (
                lambda cr=cr: ops.linear_cross_entropy(
                    h, w, t, chunk_rows=cr or None))
        if frac < 1.0:
            variants["genrec_lce[no compaction]"] = (
                lambda: ops.linear_cross_entropy(h, w, t, compact=False))
        losses = {n: fn().item() for n, fn in variants.items()}
        for fn in variants.values():            # warm-up every timed path
            for _ in range(2):
                run(fn)
        times = {n: [] for n in variants}
        for _ in range(args.repeats):
            for n, fn in variants.items():
                times[n].append(_time(lambda: run(fn), args.iters))
        for n, fn in variants.items():
            row = dict(case=case, variant=n, rows=args.rows,
                       supervised_rows=n_valid, hidden=H, vocab=V,
                       fwd_bwd_ms=statistics.median(times[n]),
                       fwd_bwd_ms_min=min(times[n]),
                       fwd_bwd_ms_max=max(times[n]),
                       peak_mib=_peak_mib(lambda: run(fn)),
                       loss=losses[n], iters=args.iters,
                       repeats=args.repeats)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del h, w, t, variants
        torch.cuda.empty_cache()
    for row in _kernel_rows(dev, 20, args.repeats):
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
