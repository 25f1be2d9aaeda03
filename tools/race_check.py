#!/usr/bin/env python3
"""Kernel race / nondeterminism checker (SURVEY.md §5.2 sanitizers).

LDS races and missing barriers in HIP kernels typically surface as
run-to-run nondeterminism (wave scheduling varies between launches). This
harness runs every genrec kernel N times on identical inputs — optionally
with a concurrent "scheduling perturber" stream issuing dummy memory
traffic to shake up wave interleaving — and asserts bitwise-identical
outputs. Deterministic-by-construction kernels (no atomics in the output
path) must produce exactly equal bits; the dQ-atomic flash backward is
checked against an fp32 tolerance instead.

Usage (on a GPU box):
    python tools/race_check.py [--iters 20] [--perturb]

Exit code 0 = all kernels deterministic; 1 = mismatch (prints kernel+op).
Also runnable as `pytest tests/test_gpu_sanitize.py` (same checks, fewer
iters).
"""

from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _perturber(stream, n=1 << 20):
    """Issue dummy traffic on a side stream to perturb wave scheduling."""
    with torch.cuda.stream(stream):
        a = torch.randn(n, device="cuda")
        for _ in range(4):
            a = a * 1.0001 + 0.1


def run_case(name, fn, iters=10, perturb=False, atol=0.0):
    torch.manual_seed(0)
    side = torch.cuda.Stream() if perturb else None
    ref = None
    for it in range(iters):
        if side is not None:
            _perturber(side)
        out = fn()
        torch.cuda.synchronize()
        outs = [o.detach().clone() for o in
                (out if isinstance(out, (list, tuple)) else [out])]
        if ref is None:
            ref = outs
            continue
        for i, (a, b) in enumerate(zip(ref, outs)):
            if atol == 0.0:
                if not torch.equal(a, b):
                    print(f"RACE? {name}[out{i}] iter {it}: "
                          f"{(a.float() - b.float()).abs().max().item():.3e}")
                    return False
            else:
                if not torch.allclose(a.float(), b.float(), atol=atol):
                    print(f"RACE? {name}[out{i}] iter {it} (atol {atol})")
                    return False
    print(f"ok   {name} ({iters} iters{', perturbed' if perturb else ''})")
    return True


def build_cases():
    from genrec_amd import ops

    dev = "cuda:0"
    B, H, L, D = 4, 6, 61, 64
    q = torch.randn(B, H, L, D, device=dev, dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    bias = torch.randn(H, L, L, device=dev)
    dout = torch.randn_like(q)

    def attn_fwd():
        return ops.ext().attn_fwd_mfma(q, k, v, bias, None, None, None,
                                       0.125, False, 0, 0.0, 0, None)[:2]

    fwd = ops.ext().attn_fwd_mfma(q, k, v, bias, None, None, None,
                                  0.125, False, 0, 0.0, 0, None)
    p_saved, dmask = fwd[1], fwd[2]

    def attn_bwd():
        return ops.ext().attn_bwd_mfma(dout, q, k, v, p_saved, dmask, None,
                                       0.125, 0, 0.0, 0, True, 3)

    Lq2, Lk2 = 80, 128
    qf = torch.randn(B, H, Lq2, D, device=dev, dtype=torch.bfloat16)
    kf = torch.randn(B, H, Lk2, D, device=dev, dtype=torch.bfloat16)
    vf = torch.randn_like(kf)
    doutf = torch.randn_like(qf)

    def flash_fwd():
        return ops.ext().attn_fwd_flash(qf, kf, vf, None, None, None, None,
                                        0.125, False, 0.0, 0, None)[:3]

    ffwd = ops.ext().attn_fwd_flash(qf, kf, vf, None, None, None, None,
                                    0.125, False, 0.0, 0, None)
    fo, fs, fml, fdm = ffwd

    def flash_bwd():
        return ops.ext().attn_bwd_flash(doutf, qf, kf, vf, fo, fs, fml, fdm,
                                        None, 0.125, 0.0, False, 0)[:3]

    # grouped-query flash attention: 6 query heads on 1 KV head, D=128,
    # three tiles with a ragged tail, left padding; [B,L,H,D] views in
    Lg, Dg = 130, 128
    qg = torch.randn(B, Lg, 6, Dg, device=dev,
                     dtype=torch.bfloat16).transpose(1, 2)
    kg = torch.randn(B, Lg, 1, Dg, device=dev,
                     dtype=torch.bfloat16).transpose(1, 2)
    vg = torch.randn_like(kg)
    doutg = torch.randn(B, Lg, 6, Dg, device=dev, dtype=torch.bfloat16)
    padg = torch.arange(Lg, device=dev)[None, :] < torch.tensor(
        [70, 0, 3, 0], device=dev)[:, None]
    sg = Dg ** -0.5

    def gqa_fwd():
        return ops.ext().gqa_attn_fwd(qg, kg, vg, padg, sg, True)

    go, glse = ops.ext().gqa_attn_fwd(qg, kg, vg, padg, sg, True)

    def gqa_bwd():
        return ops.ext().gqa_attn_bwd(doutg, qg, kg, vg, go, glse, padg,
                                      sg, True)

    # the same kernels in variable-length mode: the B rows above packed
    # into one [T,H,D] row whose sequence starts sit off the tile grid,
    # with an empty sequence and a tail that belongs to no sequence
    Tv = B * Lg
    qv, kv_, vv, doutv = (t.transpose(1, 2).reshape(Tv, -1, Dg)
                          for t in (qg, kg, vg, doutg.transpose(1, 2)))
    cuv = torch.tensor([0, 1, 70, 70, 200, Tv - 50], dtype=torch.int32,
                       device=dev)

    def gqa_varlen_fwd():
        return ops.ext().gqa_varlen_fwd(qv, kv_, vv, cuv, Tv, sg)

    vo, vlse = ops.ext().gqa_varlen_fwd(qv, kv_, vv, cuv, Tv, sg)

    def gqa_varlen_bwd():
        return ops.ext().gqa_varlen_bwd(doutv, qv, kv_, vv, vo, vlse, cuv,
                                        Tv, sg)

    # shared-prefix beam decode: 14 query heads on 2 KV heads x 10 beams =
    # 70 packed rows (two Q tiles), three K tiles over 2 splits, left
    # padding, 3 live suffix slots with a shared ancestor
    Bb, Wb = 2, 10
    qb = torch.randn(Bb * Wb, 1, 14, Dg, device=dev,
                     dtype=torch.bfloat16).transpose(1, 2)
    kb = torch.randn(Bb, Lg, 2, Dg, device=dev,
                     dtype=torch.bfloat16).transpose(1, 2)
    vb = torch.randn_like(kb)
    ksb = torch.randn(Bb, 4, Wb, 2, Dg, device=dev, dtype=torch.bfloat16)
    vsb = torch.randn_like(ksb)
    ancb = torch.randint(0, Wb, (Bb, Wb, 4), device=dev, dtype=torch.int32)
    ancb[:, 1] = ancb[:, 0]
    padb = padg[:Bb]

    def beam_fwd():
        return ops.ext().beam_attn_fwd(qb, kb, vb, padb, ksb, vsb, ancb, 3,
                                       sg, 2)

    # the same step over a packed prefill: the prompts' K/V as one
    # token-major row, starts off the tile grid, lengths 130 and 67 (the
    # second prompt has fewer tiles than there are splits: 3)
    kbv, vbv = (t.transpose(1, 2).reshape(Bb * Lg, 2, Dg) for t in (kb, vb))
    cub = torch.tensor([3, 133, 200], dtype=torch.int32, device=dev)

    def beam_varlen_fwd():
        return ops.ext().beam_attn_varlen_fwd(qb, kbv, vbv, cub, Lg, ksb, vsb,
                                              ancb, 3, sg, 3)

    # HSTU pointwise attention: one ragged 64-tile, D=32, both bias tables,
    # a key-pad tail on one batch item
    Lh, Dh, n_pos, n_time = 50, 32, 32, 64
    qh, kh, vh, douth = (torch.randn(B, 2, Lh, Dh, device=dev,
                                     dtype=torch.bfloat16) for _ in range(4))
    pbh = torch.randint(0, n_pos, (Lh, Lh), device=dev, dtype=torch.int32)
    posw = torch.randn(n_pos, 2, device=dev, dtype=torch.bfloat16)
    timew = torch.randn(n_time, 2, device=dev, dtype=torch.bfloat16)
    tsh = (torch.arange(Lh, device=dev) * 3600 + 10 ** 9).unsqueeze(0) \
        .expand(B, -1).contiguous()
    padh = torch.zeros(B, Lh, dtype=torch.bool, device=dev)
    padh[1, 40:] = True

    def hstu_fwd():
        return ops.ext().hstu_attn_fwd(qh, kh, vh, pbh, posw, timew, tsh,
                                       padh)

    hs = ops.ext().hstu_attn_fwd(qh, kh, vh, pbh, posw, timew, tsh, padh)[1]

    def hstu_bwd():
        return ops.ext().hstu_attn_bwd(douth, qh, kh, vh, hs, pbh, tsh,
                                       n_pos, n_time)[:3]

    x = torch.randn(4096, 384, device=dev, dtype=torch.bfloat16)
    w = torch.randn(384, device=dev, dtype=torch.bfloat16)

    def rms():
        return ops.ext().rms_norm_fwd(x, w, 1e-6, True)[0]

    logits = torch.randn(4096, 769, device=dev, dtype=torch.bfloat16)
    targets = torch.randint(0, 769, (4096,), device=dev)

    def ce():
        return ops.ext().softmax_ce_fwd(logits, targets, -100)[:2]

    # linear + CE on the LLM head: 3 row chunks (fp32 dW accumulation),
    # 3 column slices per row with a vector tail, some rows ignored
    lh = torch.randn(130, 64, device=dev, dtype=torch.bfloat16)
    lw = torch.randn(4099, 64, device=dev, dtype=torch.bfloat16) * 0.25
    lt = torch.randint(0, 4099, (130,), device=dev)
    lt[::3] = -100

    def lce():
        h, wt = lh.clone().requires_grad_(), lw.clone().requires_grad_()
        loss = ops.linear_cross_entropy(h, wt, lt, chunk_rows=64, _slices=3)
        loss.backward()
        return loss.detach(), h.grad, wt.grad

    b = torch.randn(384, device=dev, dtype=torch.bfloat16)

    def ln_fwd():
        return ops.ext().layer_norm_fwd(x, w, b, 1e-5)

    lf = ops.ext().layer_norm_fwd(x, w, b, 1e-5)
    dy_ln = torch.randn_like(x)

    def ln_bwd():
        return ops.ext().layer_norm_bwd(dy_ln, x, w, lf[1], lf[2])

    def csum():
        return ops.ext().colsum(x)

    # Qwen2 layer kernels: 300 rows of d = 1536 (3 chunks per lane, 75
    # blocks of dw partials, a residual and an incoming dh), RoPE over
    # 12 + 2 heads read through [B,L,H*D] transpose views, SwiGLU on the
    # two halves of one [rows, 2*I] buffer
    e = ops.ext()
    nx = torch.randn(300, 1536, device=dev, dtype=torch.bfloat16)
    nres, ndn, ndh = (torch.randn_like(nx) for _ in range(3))
    nw = torch.randn(1536, device=dev, dtype=torch.bfloat16)

    def addnorm_fwd():
        return e.add_rms_norm_fwd(nx, nres, nw, 1e-6)

    nh, _, ninv = e.add_rms_norm_fwd(nx, nres, nw, 1e-6)

    def addnorm_bwd():
        return e.add_rms_norm_bwd(ndn, ndh, nh, nw, ninv)

    rq = torch.randn(2, 70, 12 * Dg, device=dev, dtype=torch.bfloat16) \
        .view(2, 70, 12, Dg).transpose(1, 2)
    rk = torch.randn(2, 70, 2 * Dg, device=dev, dtype=torch.bfloat16) \
        .view(2, 70, 2, Dg).transpose(1, 2)
    rcos = torch.randn(2, 70, Dg, device=dev, dtype=torch.bfloat16)
    rsin = torch.randn_like(rcos)

    def rope_fwd():
        return e.rope_qk_fwd(rq, rk, rcos, rsin, False)

    def rope_bwd():
        return e.rope_qk_fwd(rq, rk, rcos, rsin, True)

    sgu = torch.randn(37, 2 * 8960, device=dev, dtype=torch.bfloat16)
    sdy = torch.randn(37, 8960, device=dev, dtype=torch.bfloat16)

    def swiglu_fwd():
        return e.swiglu_fwd(sgu[:, :8960], sgu[:, 8960:])

    def swiglu_bwd():
        return e.swiglu_bwd(sdy, sgu[:, :8960], sgu[:, 8960:])

    return [
        ("add_rms_norm_fwd(h,n,inv_rms)", addnorm_fwd, 0.0),
        ("add_rms_norm_bwd(dx,dw)", addnorm_bwd, 0.0),
        ("rope_qk_fwd", rope_fwd, 0.0),
        ("rope_qk_fwd(inverse)", rope_bwd, 0.0),
        ("swiglu_fwd", swiglu_fwd, 0.0),
        ("swiglu_bwd(dgate,dup)", swiglu_bwd, 0.0),
        ("attn_fwd_mfma", attn_fwd, 0.0),
        ("attn_bwd_ds(8-wave)", attn_bwd, 0.0),
        ("attn_fwd_flash", flash_fwd, 0.0),
        # flash bwd accumulates dQ with fp32 global atomics -> order-
        # dependent rounding; tolerance instead of bitwise
        ("attn_bwd_flash", flash_bwd, 2e-3),
        # no atomics anywhere: bitwise
        ("gqa_attn_fwd", gqa_fwd, 0.0),
        ("gqa_attn_bwd", gqa_bwd, 0.0),
        ("gqa_varlen_fwd", gqa_varlen_fwd, 0.0),
        ("gqa_varlen_bwd", gqa_varlen_bwd, 0.0),
        ("beam_attn_fwd", beam_fwd, 0.0),
        ("beam_attn_varlen_fwd", beam_varlen_fwd, 0.0),
        ("hstu_attn_fwd(out,s)", hstu_fwd, 0.0),
        # dpos / dtime come from float LDS atomics (order-dependent
        # rounding) and are left out; dq, dk, dv have none
        ("hstu_attn_bwd(dq,dk,dv)", hstu_bwd, 0.0),
        ("rms_norm", rms, 0.0),
        ("layer_norm_fwd", ln_fwd, 0.0),
        ("layer_norm_bwd", ln_bwd, 0.0),
        ("colsum(vec4)", csum, 0.0),
        ("softmax_ce", ce, 0.0),
        ("linear_cross_entropy(loss,dhidden,dweight)", lce, 0.0),
    ]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--perturb", action="store_true")
    args = p.parse_args()
    assert torch.cuda.is_available(), "race_check needs a GPU"
    ok = True
    for name, fn, atol in build_cases():
        ok &= run_case(name, fn, iters=args.iters, perturb=args.perturb,
                       atol=atol)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
