"""Per-shape timing of the T5 MFMA attention (ops.t5_attention).

The TIGER train step runs three attention shapes at B=256, H=6, D=64 and
every one of them launches B*H = 1536 blocks, so a kernel trace of the step
cannot tell them apart. This tool times each alone:

  enc_self   Lq=61 Lk=61  rel-bias [H,61,61] (with grad) + key padding
  dec_self   Lq=4  Lk=4   causal additive mask
  cross      Lq=4  Lk=61  key padding

q/k/v are the strided views the model passes: chunks of a fused
[B,L,3*H*D] projection output, viewed [B,L,H,D] and transposed. Dropout
p=0.1 is on, as in training. Reports, per shape, the median over repeats
of the mean forward and forward+backward time (device events). Eager
forward+backward at these sizes runs at the host's launch rate, not the
kernels'; for kernel times run one shape under a kernel trace:

    rocprofv3 --kernel-trace --stats -- \
        python benchmarks/bench_t5_attention.py --shapes enc_self

Usage: python benchmarks/bench_t5_attention.py [--iters N] [--repeats R]
       [--shapes NAME ...] [--out results.jsonl]
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

B, H, D, P_DROP = 256, 6, 64, 0.1
SHAPES = {
    "enc_self": dict(Lq=61, Lk=61, bias=True, key_pad=True, causal_mask=False),
    "dec_self": dict(Lq=4, Lk=4, bias=False, key_pad=False, causal_mask=True),
    "cross": dict(Lq=4, Lk=61, bias=False, key_pad=True, causal_mask=False),
}


def _inputs(s, dev):
    g = torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    def split(x, l):
        return x.view(B, l, H, D).transpose(1, 2)

    lq, lk = s["Lq"], s["Lk"]
    qkv_q = rnd(B, lq, 3 * H * D).to(torch.bfloat16).requires_grad_()
    if lq == lk:
        qkv_k = qkv_q               # self attention: one fused projection
    else:
        qkv_k = rnd(B, lk, 3 * H * D).to(torch.bfloat16).requires_grad_()
    leaves = [qkv_q] if qkv_k is qkv_q else [qkv_q, qkv_k]
    q = split(qkv_q.chunk(3, dim=-1)[0], lq)
    k = split(qkv_k.chunk(3, dim=-1)[1], lk)
    v = split(qkv_k.chunk(3, dim=-1)[2], lk)
    bias = key_pad = add_mask = None
    if s["bias"]:
        bias = rnd(H, lq, lk).requires_grad_()
        leaves.append(bias)
    if s["key_pad"]:
        key_pad = torch.zeros(B, lk, dtype=torch.bool, device=dev)
        key_pad[::2, lk - 7:] = True
    if s["causal_mask"]:
        add_mask = torch.triu(
            torch.full((lq, lk), float("-inf"), device=dev), 1)
    dout = rnd(B, lq, H, D).to(torch.bfloat16).transpose(1, 2)
    return q, k, v, bias, key_pad, add_mask, dout, leaves


def _time(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=300)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--shapes", nargs="+", default=list(SHAPES),
                   choices=list(SHAPES),
                   help="time only these (one shape per kernel-trace run "
                        "tells the shapes' kernels apart)")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    scale = D ** -0.5
    rows = []
    for sname in args.shapes:
        s = SHAPES[sname]
        q, k, v, bias, key_pad, add_mask, dout, leaves = _inputs(s, dev)

        def attn():
            return ops.t5_attention(q, k, v, bias, key_pad, add_mask, scale,
                                    P_DROP, True)

        def fwd():
            with torch.no_grad():
                attn()

        def fwd_bwd():
            attn().backward(dout)
            for t in leaves:
                t.grad = None

        for _ in range(10):             # warm-up every timed path
            fwd()
            fwd_bwd()
        t_fwd, t_fb = [], []
        for _ in range(args.repeats):
            t_fwd.append(_time(fwd, args.iters))
            t_fb.append(_time(fwd_bwd, args.iters))
        row = dict(shape=sname, B=B, H=H, D=D, Lq=s["Lq"], Lk=s["Lk"],
                   dropout_p=P_DROP,
                   fwd_us=1e3 * statistics.median(t_fwd),
                   fwd_bwd_us=1e3 * statistics.median(t_fb),
                   fwd_us_min=1e3 * min(t_fwd), fwd_us_max=1e3 * max(t_fwd),
                   fwd_bwd_us_min=1e3 * min(t_fb),
                   fwd_bwd_us_max=1e3 * max(t_fb),
                   iters=args.iters, repeats=args.repeats)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
