"""A/B microbenchmark: ops.add_rms_norm / ops.rope_qk / ops.swiglu
(csrc/kernels/llm_layer.hip) against the stock transformers op compositions
they replace inside a Qwen2 decoder layer, forward and forward+backward.

Shapes: the LCRec recipe, B=32, L=512, hidden 1536, intermediate 8960,
12/2 heads, D=128, bf16. Per op and direction the script prints the median
over repeats of the mean call time (device events, the two variants
alternating inside each repeat), the bytes the op has to move at the least
(counted from the tensor sizes in `_cases`), the resulting GB/s and
that rate as a fraction of a reference rate (default 5.05 TB/s, what the
project's lce kernel pair reaches; see profiles/BENCHMARKS.md). The
forward+backward rows go through autograd and are bounded by the host's
launch rate for the smaller ops, so the last rows (variant "kernel") time
each extension call alone, with no autograd around it.

Usage: python benchmarks/bench_llm_layer_ops.py [--iters N] [--repeats R]
       [--batch 32] [--seq 512] [--out results.jsonl]
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
from genrec_amd.ops import eager  # noqa: E402

HIDDEN, INTER, HQ, HKV, D = 1536, 8960, 12, 2, 128
EPS = 1e-6


def _time(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def _cases(B, L, dev):
    """name -> (fused fn, stock fn, inputs, grad outputs, floor bytes fwd,
    floor bytes fwd+bwd). Each fn maps the inputs to a tuple of outputs."""
    g = torch.Generator(device="cpu").manual_seed(0)
    rows = B * L

    def rnd(*shape, grad=True):
        t = torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)
        return t.requires_grad_() if grad else t

    blk = rows * HIDDEN * 2                         # one [rows, hidden] block
    x, res, w = rnd(rows, HIDDEN), rnd(rows, HIDDEN), rnd(HIDDEN)
    dh, dn = rnd(rows, HIDDEN, grad=False), rnd(rows, HIDDEN, grad=False)
    q = rnd(B, L, HQ * D).view(B, L, HQ, D).transpose(1, 2)
    k = rnd(B, L, HKV * D).view(B, L, HKV, D).transpose(1, 2)
    cos = rnd(1, L, D, grad=False)
    sin = rnd(1, L, D, grad=False)
    dq = rnd(B, L, HQ, D, grad=False).transpose(1, 2)
    dk = rnd(B, L, HKV, D, grad=False).transpose(1, 2)
    qk = rows * (HQ + HKV) * D * 2
    gate, up = rnd(rows, INTER), rnd(rows, INTER)
    dy = rnd(rows, INTER, grad=False)
    act = rows * INTER * 2
    return {
        # first norm of a layer: read x, write n | read dn, h, write dx
        "rms_norm": (
            lambda x, w: (ops.add_rms_norm(x, None, w, EPS)[1],),
            lambda x, w: (eager.add_rms_norm(x, None, w, EPS)[1],),
            (x, w), (dn,), 2 * blk, 5 * blk),
        # second norm: read x, res, write h, n | read dn, dh, h, write dx
        "add_rms_norm": (
            lambda x, r, w: ops.add_rms_norm(x, r, w, EPS),
            lambda x, r, w: eager.add_rms_norm(x, r, w, EPS),
            (x, res, w), (dh, dn), 4 * blk, 8 * blk),
        "rope_qk": (
            lambda q, k: ops.rope_qk(q, k, cos, sin),
            lambda q, k: eager.rope_qk(q, k, cos, sin),
            (q, k), (dq, dk), 2 * qk, 4 * qk),
        # read gate, up, write y | read gate, up, dy, write dgate, dup
        "swiglu": (
            lambda a, b: (ops.swiglu(a, b),),
            lambda a, b: (eager.swiglu(a, b),),
            (gate, up), (dy,), 3 * act, 8 * act),
    }


def _kernel_cases(B, L, dev):
    """name -> (callable running one extension call, floor bytes)."""
    e = ops.ext()
    g = torch.Generator(device="cpu").manual_seed(1)
    rows = B * L

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)

    blk, qk, act = rows * HIDDEN * 2, rows * (HQ + HKV) * D * 2, \
        rows * INTER * 2
    x, res, w = rnd(rows, HIDDEN), rnd(rows, HIDDEN), rnd(HIDDEN)
    dh, dn = rnd(rows, HIDDEN), rnd(rows, HIDDEN)
    h, _, inv = e.add_rms_norm_fwd(x, res, w, EPS)
    q = rnd(B, L, HQ * D).view(B, L, HQ, D).transpose(1, 2)
    k = rnd(B, L, HKV * D).view(B, L, HKV, D).transpose(1, 2)
    cos, sin = rnd(1, L, D), rnd(1, L, D)
    gu, dy = rnd(rows, 2 * INTER), rnd(rows, INTER)
    gate, up = gu[:, :INTER], gu[:, INTER:]
    return {
        "add_rms_norm_fwd (no residual)":
            (lambda: e.add_rms_norm_fwd(x, None, w, EPS), 2 * blk),
        "add_rms_norm_fwd (residual)":
            (lambda: e.add_rms_norm_fwd(x, res, w, EPS), 4 * blk),
        "add_rms_norm_bwd (no dh) + dw reduce":
            (lambda: e.add_rms_norm_bwd(dn, None, h, w, inv), 3 * blk),
        "add_rms_norm_bwd (dh) + dw reduce":
            (lambda: e.add_rms_norm_bwd(dn, dh, h, w, inv), 4 * blk),
        "rope_qk_fwd": (lambda: e.rope_qk_fwd(q, k, cos, sin, False), 2 * qk),
        "rope_qk_fwd (inverse)":
            (lambda: e.rope_qk_fwd(q, k, cos, sin, True), 2 * qk),
        "swiglu_fwd (halves of one buffer)":
            (lambda: e.swiglu_fwd(gate, up), 3 * act),
        "swiglu_bwd": (lambda: e.swiglu_bwd(dy, gate, up), 5 * act),
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--seq", type=int, default=512)
    p.add_argument("--reference-tbps", type=float, default=5.05)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_llm_layer_ops needs a GPU"
    dev = torch.device("cuda:0")
    results = []
    for name, (fused, stock, ins, douts, b_fwd, b_all) in _cases(
            args.batch, args.seq, dev).items():

        def fwd(fn):
            with torch.no_grad():
                fn(*ins)

        def fwd_bwd(fn):
            torch.autograd.grad(fn(*ins), ins, douts)

        for direction, run, nbytes in (("fwd", fwd, b_fwd),
                                       ("fwd+bwd", fwd_bwd, b_all)):
            for fn in (fused, stock):                 # warm-up, both variants
                run(fn)
            torch.cuda.synchronize()
            t = {"fused": [], "stock": []}
            for _ in range(args.repeats):
                t["fused"].append(_time(lambda: run(fused), args.iters))
                t["stock"].append(_time(lambda: run(stock), args.iters))
            for variant in ("fused", "stock"):
                ms = statistics.median(t[variant])
                rate = nbytes / (ms * 1e-3)
                r = dict(op=name, direction=direction, variant=variant,
                         ms=round(ms, 4), floor_mb=round(nbytes / 1e6, 1),
                         gb_per_s=round(rate / 1e9, 1),
                         frac_of_reference=round(
                             rate / (args.reference_tbps * 1e12), 3),
                         speedup_vs_stock=round(
                             statistics.median(t["stock"]) / ms, 2),
                         batch=args.batch, seq=args.seq)
                print(json.dumps(r), flush=True)
                results.append(r)
    for name, (fn, nbytes) in _kernel_cases(args.batch, args.seq,
                                            dev).items():
        fn()
        torch.cuda.synchronize()
        ms = statistics.median(_time(fn, args.iters * 5)
                               for _ in range(args.repeats))
        rate = nbytes / (ms * 1e-3)
        r = dict(op=name, variant="kernel", ms=round(ms, 4),
                 floor_mb=round(nbytes / 1e6, 1),
                 gb_per_s=round(rate / 1e9, 1),
                 frac_of_reference=round(
                     rate / (args.reference_tbps * 1e12), 3),
                 batch=args.batch, seq=args.seq)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
