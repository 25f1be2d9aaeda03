"""T5 MFMA attention (attention_mfma.hip) with transposed-read operands.

The kernels read K, Q, dO, V, P^T and dS^T by columns through
frag_load_tr (ds_read_b64_tr_b16). A wrong block address there gives wrong
MFMA operands without a fault, so these tests compare EVERY element:

(a) direct extension calls with dropout on (the path the TIGER benchmark
    runs), against an fp32 torch reference built with the kernel's own
    dropout mask, over the tile-edge shapes and both input layouts;
(b) exact-integer operands with closed-form results;
(c) bitwise run-to-run determinism.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H = 3, 2
SHAPES = [(61, 61, 64), (64, 64, 64), (4, 4, 64), (4, 61, 64), (33, 17, 64),
          (61, 61, 32), (1, 1, 32)]
# the tolerances of test_mfma_attention_vs_eager
TOL = dict(atol=5e-2, rtol=5e-2)
TOL_SILU = dict(atol=1.0, rtol=5e-2)
TOL_DBIAS = dict(atol=8e-2, rtol=8e-2)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


def _ext():
    from genrec_amd import ops

    return ops.ext()


def _qkv(lq, lk, d, layout):
    """bf16 q/k/v/dout as [B,H,L,D]: contiguous, or transpose views of the
    chunks of a fused [B,L,3*H*D] projection output."""
    if layout == "contig":
        q = torch.randn(B, H, lq, d, device=DEV).bfloat16()
        k = torch.randn(B, H, lk, d, device=DEV).bfloat16()
        v = torch.randn(B, H, lk, d, device=DEV).bfloat16()
        dout = torch.randn(B, H, lq, d, device=DEV).bfloat16()
        return q, k, v, dout
    qkv_q = torch.randn(B, lq, 3 * H * d, device=DEV).bfloat16()
    qkv_k = torch.randn(B, lk, 3 * H * d, device=DEV).bfloat16()
    q = qkv_q.chunk(3, dim=-1)[0].view(B, lq, H, d).transpose(1, 2)
    k = qkv_k.chunk(3, dim=-1)[1].view(B, lk, H, d).transpose(1, 2)
    v = qkv_k.chunk(3, dim=-1)[2].view(B, lk, H, d).transpose(1, 2)
    dout = torch.randn(B, lq, H, d, device=DEV).bfloat16().transpose(1, 2)
    assert not q.is_contiguous() and q.stride(3) == 1
    return q, k, v, dout


def _reference(q, k, v, bias, pad, am, scale, causal, silu, keep, p):
    """fp32 torch composition with the kernel's masking order and its own
    dropout mask `keep`."""
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias
    lq, lk = s.shape[-2:]
    if causal:
        above = torch.triu(torch.ones(lq, lk, dtype=torch.bool, device=DEV), 1)
        s = s.masked_fill(above, -1e9)
    if pad is not None:
        s = s.masked_fill(pad[:, None, None, :], -1e9)
    if am is not None:
        s = s + am
    pr = s * torch.sigmoid(s) if silu else torch.softmax(s, dim=-1)
    if p > 0:
        pr = pr * keep.float() / (1.0 - p)
    return torch.matmul(pr, v)


def _run_case(lq, lk, d, layout, kind, seed=1234):
    """fwd + bwd through the extension; returns (got, ref) dicts."""
    q, k, v, dout = _qkv(lq, lk, d, layout)
    bias = pad = am = None
    causal, silu, p, scale = False, False, 0.3, 0.125
    if kind == "bias_pad":
        bias = torch.randn(H, lq, lk, device=DEV)
        if lk > 1:
            pad = torch.zeros(B, lk, dtype=torch.bool, device=DEV)
            pad[1, (3 * lk) // 4:] = True
    elif kind == "causal_addmask":
        am = torch.triu(torch.full((lq, lk), float("-inf"), device=DEV), 1)
    elif kind == "silu":
        # the SiLU backward takes no dropout mask (HSTU runs without
        # dropout), so this case runs with p = 0
        bias = torch.randn(B, H, lq, lk, device=DEV)
        causal, silu, p, scale = True, True, 0.0, 1.0
    act = 1 if silu else 0
    ext = _ext()
    out, p_saved, keep = ext.attn_fwd_mfma(q, k, v, bias, pad, am, None,
                                           scale, causal, act, p, seed, None)
    dq, dk, dv, dbias = ext.attn_bwd_mfma(
        dout, q, k, v, p_saved, keep, None, scale, act, p, seed,
        bias is not None, bias.dim() if bias is not None else 0)
    got = dict(out=out, dq=dq, dk=dk, dv=dv)
    if bias is not None:
        got["dbias"] = dbias

    q2, k2, v2 = (t.float().detach().requires_grad_() for t in (q, k, v))
    b2 = bias.detach().clone().requires_grad_() if bias is not None else None
    r = _reference(q2, k2, v2, b2, pad, am, scale, causal, silu, keep, p)
    r.backward(dout.float())
    ref = dict(out=r.detach(), dq=q2.grad, dk=k2.grad, dv=v2.grad)
    if bias is not None:
        ref["dbias"] = b2.grad
    if p > 0:
        frac = keep.float().mean().item()
        assert keep.shape == (B, H, lq, lk) and (lq * lk < 64 or
                                                 0.4 < frac < 0.95), frac
    return got, ref


def _compare(got, ref, silu=False):
    for name in ref:
        tol = TOL_DBIAS if name == "dbias" else (TOL_SILU if silu else TOL)
        g, r = got[name].float(), ref[name]
        assert g.shape == r.shape, (name, g.shape, r.shape)
        err = (g - r).abs().max().item()
        print(f"{name}: max abs err {err:.4g}")
        assert torch.allclose(g, r, **tol), (name, err)


@pytest.mark.parametrize("kind", ["bias_pad", "causal_addmask"])
@pytest.mark.parametrize("layout", ["contig", "chunk"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dropout_vs_reference(shape, layout, kind):
    got, ref = _run_case(*shape, layout, kind)
    _compare(got, ref)


@pytest.mark.parametrize("layout", ["contig", "chunk"])
def test_silu_vs_reference(layout):
    got, ref = _run_case(61, 61, 64, layout, "silu")
    _compare(got, ref, silu=True)


def _int_tile(rows, cols, a, b_, mod):
    """small integers (|x| <= mod//2, exact in bf16) that differ along both
    axes"""
    r = torch.arange(rows, device=DEV)[:, None]
    c = torch.arange(cols, device=DEV)[None, :]
    return ((a * r + b_ * c) % mod - mod // 2).float()


@pytest.mark.parametrize("masked", [False, True], ids=["uniform", "masked"])
def test_exact_integer_operands(masked):
    """q = 0 makes S = 0 and P uniform over the allowed keys, a power of two
    (1/64, or 1/32 under an additive mask that lets row i see the 32 keys
    whose bit i%6 equals (i//6)&1). With integer v and dout every sum is
    exact in fp32, so out = bf16(P v), dV = bf16(P^T dO) and dK = 0 hold on
    every element; a mis-addressed operand block moves them by whole
    units."""
    lq = lk = d = 64
    q = torch.zeros(B, H, lq, d, device=DEV, dtype=torch.bfloat16)
    k = torch.randn(B, H, lk, d, device=DEV).bfloat16()
    bh = torch.arange(B * H, device=DEV).view(B, H, 1, 1).float()
    v32 = _int_tile(lk, d, 5, 11, 61).expand(B, H, lk, d) + bh
    do32 = _int_tile(lq, d, 7, 3, 53).expand(B, H, lq, d) - bh
    v, dout = v32.bfloat16(), do32.bfloat16()
    assert torch.equal(v.float(), v32) and torch.equal(dout.float(), do32)
    am = None
    allow = torch.ones(lq, lk, device=DEV)
    if masked:
        i = torch.arange(lq, device=DEV)[:, None]
        j = torch.arange(lk, device=DEV)[None, :]
        allow = (((j >> (i % 6)) & 1) == ((i // 6) & 1)).float()
        assert (allow.sum(1) == 32).all()
        am = torch.zeros(lq, lk, device=DEV).masked_fill(allow == 0,
                                                         float("-inf"))
        # transpose views, as the models pass them
        v = v.transpose(1, 2).contiguous().transpose(1, 2)
        dout = dout.transpose(1, 2).contiguous().transpose(1, 2)
    pr = allow / allow.sum(1, keepdim=True)          # exact powers of two
    ext = _ext()
    out, p_saved, keep = ext.attn_fwd_mfma(q, k, v, None, None, am, None,
                                           0.125, False, 0, 0.0, 0, None)
    dq, dk, dv, _ = ext.attn_bwd_mfma(dout, q, k, v, p_saved, keep, None,
                                      0.125, 0, 0.0, 0, False, 0)
    assert torch.equal(p_saved, pr.expand(B, H, lq, lk))
    want_out = torch.matmul(pr, v32).bfloat16()
    want_dv = torch.matmul(pr.t(), do32).bfloat16()
    assert torch.equal(out, want_out), (out.float() - want_out.float()) \
        .abs().max()
    assert torch.equal(dv, want_dv), (dv.float() - want_dv.float()) \
        .abs().max()
    assert torch.equal(dk, torch.zeros_like(dk))
    assert torch.isfinite(dq.float()).all()


def test_bitwise_deterministic():
    """two runs of the encoder shape (bias, key padding, dropout) agree on
    every bit of every output"""
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        got, _ = _run_case(61, 61, 64, "chunk", "bias_pad")
        runs.append(got)
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
