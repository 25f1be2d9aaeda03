#!/usr/bin/env python3
"""LoRA-adapted linear: ops.lora_linear (csrc/kernels/lora.hip) against the
stock op composition (dropout, two F.linear, scale, add; autograd for the
gradients), forward + backward, on the seven Qwen2.5-1.5B projections at
M = B * L = 16,384 rows, r = 16, p = 0.05, bf16, base weight frozen.

Both run in the same process, alternated inside each repeat (composition,
kernels, composition: the two composition runs give the run's own spread).
Times are device events around `--launches` launches; the table shows the
median and min-max over `--repeats` repeats after a warm-up. Each kernel is
also timed alone and reported with the bytes its contract has to move
(computed from the shapes below) and the rate that gives. Before timing,
every output of the kernel route is checked against a float64 reference
with the test suite's bound (2 x the composition's own error).

Usage: python benchmarks/bench_lora.py [--rows 16384] [--repeats 7]
       [--launches 50] [--out results.jsonl]
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

# (name, K, N) of the Qwen2.5-1.5B projections
SHAPES = (("q_proj", 1536, 1536), ("k_proj", 1536, 256),
          ("v_proj", 1536, 256), ("o_proj", 1536, 1536),
          ("gate_proj", 1536, 8960), ("up_proj", 1536, 8960),
          ("down_proj", 8960, 1536))
R, ALPHA, P, SEED = 16, 32.0, 0.05, 1234
S = ALPHA / R


def floor_bytes(M, K, N, r=R):
    """bytes each kernel call of one fwd+bwd has to move: its wide operand
    once (twice for the in-place update), the rank-side matrices once"""
    b = 2
    return {
        "down_fwd": (M * K + r * K + M * r) * b,          # x, A -> t
        "up_add_fwd": (2 * M * N + M * r + N * r) * b,    # y rw, t, B
        "down_bwd": (M * N + r * N + M * r) * b,          # dy, B^T -> dt
        "grad_dB": (M * N + M * r + r * N) * b,           # dy, t -> dB^T
        "grad_dA": (M * K + M * r + r * K) * b,           # x, dt -> dA
        "up_add_bwd": (2 * M * K + M * r + K * r) * b,    # dx rw, dt, A^T
    }


def _timed(fn, launches):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / launches * 1e3          # us


def _stats(xs):
    return dict(median_us=statistics.median(xs), min_us=min(xs),
                max_us=max(xs))


def _compose(x, w, a, b):
    xd = F.dropout(x, P, True)
    return F.linear(x, w) + F.linear(F.linear(xd, a), b) * S


def _check(x, w, a, b, dy):
    """the test suite's bound on (y, dx, dA, dB) at this shape"""
    from genrec_amd import ops
    from genrec_amd.ops import eager

    M, K = x.shape
    mask = eager.lora_dropout_mask(M, K, P, SEED, x.device)

    def run(fn, dtype):
        leaves = [t.detach().to(dtype).requires_grad_(True)
                  for t in (x, a, b)]
        y = fn(leaves[0], w.to(dtype), leaves[1], leaves[2])
        return (y,) + torch.autograd.grad(y, leaves, dy.to(dtype))

    ref = run(lambda x, w, a, b: F.linear(x, w) + S * F.linear(
        F.linear(x * mask / (1 - P), a), b), torch.float64)
    stock = run(lambda x, w, a, b: F.linear(x, w) + F.linear(F.linear(
        (x.float() * mask * (1 / (1 - P))).to(x.dtype), a), b) * S,
        torch.bfloat16)
    got = run(lambda x, w, a, b: ops.lora_linear(
        x, w, None, a, b, S, p=P, training=True, seed=SEED), torch.bfloat16)
    out = {}
    for name, g, s, r in zip(("y", "dx", "dA", "dB"), got, stock, ref):
        ek = (g.double() - r).abs().max().item()
        eb = (s.double() - r).abs().max().item()
        out[name] = dict(kernel_err=ek, stock_err=eb,
                         ratio=ek / eb if eb else float("inf"),
                         held=ek <= 2 * eb)
    return out


def bench_shape(name, M, K, N, repeats, launches, check=True):
    from genrec_amd import ops

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    mk = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale) \
        .to(torch.bfloat16).to(dev)
    x = mk(M, K).requires_grad_(True)
    w = mk(N, K, scale=K ** -0.5)
    a = mk(R, K, scale=K ** -0.5).requires_grad_(True)
    b = mk(N, R, scale=R ** -0.5).requires_grad_(True)
    dy = mk(M, N)
    res = dict(shape=name, M=M, K=K, N=N, r=R, p=P)
    if check:
        res["check"] = _check(x, w, a, b, dy)

    def kernel():
        y = ops.lora_linear(x, w, None, a, b, S, p=P, training=True,
                            seed=SEED)
        torch.autograd.grad(y, (x, a, b), dy)

    def compose():
        torch.autograd.grad(_compose(x, w, a, b), (x, a, b), dy)

    for fn in (kernel, compose):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    tk, tc1, tc2 = [], [], []
    for _ in range(repeats):
        tc1.append(_timed(compose, launches))
        tk.append(_timed(kernel, launches))
        tc2.append(_timed(compose, launches))
    res["kernel"] = _stats(tk)
    res["compose"] = _stats(tc1 + tc2)
    res["compose_spread"] = statistics.median(
        abs(u - v) / min(u, v) for u, v in zip(tc1, tc2))
    res["speedup"] = res["compose"]["median_us"] / res["kernel"]["median_us"]

    # each kernel alone, with its floor bytes
    ext = ops.ext()
    xd, dyd = x.detach(), dy
    t = ext.lora_down(xd, a.detach(), 1 / (1 - P), P, SEED)
    bt = b.detach().t().contiguous()
    at = a.detach().t().contiguous()
    dt = ext.lora_down(dyd, bt, S, 0.0, 0)
    ybuf, dxbuf = torch.zeros(M, N, dtype=torch.bfloat16, device=dev), \
        torch.zeros(M, K, dtype=torch.bfloat16, device=dev)
    calls = {
        "down_fwd": lambda: ext.lora_down(xd, a.detach(), 1 / (1 - P), P,
                                          SEED),
        "up_add_fwd": lambda: ext.lora_up_add_(ybuf, t, b.detach(), S, 0.0,
                                               0),
        "down_bwd": lambda: ext.lora_down(dyd, bt, S, 0.0, 0),
        "grad_dB": lambda: ext.lora_grad(t, dyd, S, 0.0, 0),
        "grad_dA": lambda: ext.lora_grad(dt, xd, 1 / (1 - P), P, SEED),
        "up_add_bwd": lambda: ext.lora_up_add_(dxbuf, dt, at, 1 / (1 - P),
                                               P, SEED),
    }
    floors = floor_bytes(M, K, N)
    res["kernels"] = {}
    for kname, fn in calls.items():
        for _ in range(3):
            fn()
        us = statistics.median(_timed(fn, launches) for _ in range(repeats))
        res["kernels"][kname] = dict(
            us=us, floor_mb=floors[kname] / 1e6,
            tb_per_s=floors[kname] / (us * 1e-6) / 1e12)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=16384)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--launches", type=int, default=50)
    p.add_argument("--shapes", default=None,
                   help="comma-separated projection names (default: all)")
    p.add_argument("--no-check", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora.py measures on the GPU; none found")
    want = set(args.shapes.split(",")) if args.shapes else None
    seen = set()
    for name, K, N in SHAPES:
        if want is not None and name not in want:
            continue
        if (K, N) in seen:      # k/v and gate/up share a shape
            continue
        seen.add((K, N))
        r = bench_shape(name, args.rows, K, N, args.repeats, args.launches,
                        check=not args.no_check)
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
