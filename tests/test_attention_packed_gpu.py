"""Packed qkv gradient of T5 self-attention.

attn_bwd_mfma can write dq, dk, dv into the three column blocks of one
[B, L, 3*H*D] buffer (the layout the fused qkv projection's backward
reads), on the 64-row and on the small-query kernels. The buffer must hold
exactly the concatenation of the unpacked gradients, and a T5Attention
layer must compute the same output and gradients on the packed route as on
the chunk route (GENREC_DISABLE_PACKED_QKV=1).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H = 3, 2


def _ext():
    from genrec_amd import ops

    return ops.ext()


# encoder shape (64-row kernels), decoder shape (small-query kernels), and
# a size that is no multiple of a fragment with the narrow head
@pytest.mark.parametrize("shape", [(61, 61, 64), (4, 4, 64), (33, 33, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_dqkv_out_is_the_concatenation(shape):
    lq, lk, d = shape
    torch.manual_seed(0)
    ext = _ext()
    qkv = torch.randn(B, lq, 3 * H * d, device=DEV).bfloat16()
    q, k, v = (c.view(B, lq, H, d).transpose(1, 2)
               for c in qkv.chunk(3, dim=-1))
    dout = torch.randn(B, lq, H, d, device=DEV).bfloat16().transpose(1, 2)
    bias = torch.randn(H, lq, lk, device=DEV)
    pad = torch.zeros(B, lk, dtype=torch.bool, device=DEV)
    pad[1, (3 * lk) // 4:] = True
    p, seed, scale = 0.3, 1234, 0.125
    out, p_saved, keep = ext.attn_fwd_mfma(q, k, v, bias, pad, None, None,
                                           scale, False, 0, p, seed, None)
    dq, dk, dv, dbias = ext.attn_bwd_mfma(
        dout, q, k, v, p_saved, keep, None, scale, 0, p, seed, True, 3)
    # poison: every element of the buffer must be written
    dqkv = torch.full((B, lq, 3 * H * d), float("nan"), device=DEV,
                      dtype=torch.bfloat16)
    dq2, dk2, dv2, dbias2 = ext.attn_bwd_mfma(
        dout, q, k, v, p_saved, keep, None, scale, 0, p, seed, True, 3,
        None, 0, dqkv)
    want = torch.cat([g.transpose(1, 2).reshape(B, lq, H * d)
                      for g in (dq, dk, dv)], dim=-1)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(dqkv, want)
    assert torch.equal(dbias2, dbias)
    # the returned gradients are views of the buffer
    for got, ref in ((dq2, dq), (dk2, dk), (dv2, dv)):
        assert got.shape == ref.shape and torch.equal(got, ref)
        assert got.untyped_storage().data_ptr() == \
            dqkv.untyped_storage().data_ptr()


def test_dqkv_out_is_checked():
    ext = _ext()
    q = torch.randn(B, H, 4, 64, device=DEV).bfloat16()
    k = torch.randn(B, H, 8, 64, device=DEV).bfloat16()
    out, p_saved, keep = ext.attn_fwd_mfma(q, k, k, None, None, None, None,
                                           0.125, False, 0, 0.0, 0, None)
    buf = torch.empty(B, 4, 3 * H * 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="Lq == Lk"):
        ext.attn_bwd_mfma(out, q, k, k, p_saved, keep, None, 0.125, 0, 0.0,
                          0, False, 0, None, 0, buf)
    with pytest.raises(RuntimeError, match="dqkv_out"):
        ext.attn_bwd_mfma(out, q, q, q, p_saved[..., :4].contiguous(), keep,
                          None, 0.125, 0, 0.0, 0, False, 0, None, 0,
                          buf.float())


def _layer_run(layer, x0, pad):
    torch.manual_seed(7)
    layer.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_()
    out = layer(x, key_padding_mask=pad)
    out.backward(torch.ones_like(out) * 0.5 + out.detach() * 0.25)
    torch.cuda.synchronize()
    return dict(out=out.detach(), dx=x.grad, dqkv_w=layer.qkv.weight.grad,
                dbias_w=layer.rel_bias.weight.grad)


# L = 61 runs the 64-row kernels, L = 4 the small-query ones
@pytest.mark.parametrize("seq", [61, 4])
def test_layer_packed_equals_chunk_route(monkeypatch, seq):
    """One bf16 T5Attention self-attention layer (as the graphed TIGER step
    runs it), train mode, dropout 0.1, the RNG reset before each run: the
    packed route and the chunk route agree on every bit of the output, the
    input gradient and the two weight gradients."""
    from genrec_amd import ops
    from genrec_amd.modules.transformer import T5Attention

    torch.manual_seed(0)
    layer = T5Attention(128, H, dropout=0.1).to(DEV).bfloat16().train()
    x0 = torch.randn(B, seq, 128, device=DEV).bfloat16()
    pad = torch.zeros(B, seq, dtype=torch.bool, device=DEV)
    pad[1, (3 * seq) // 4:] = True

    monkeypatch.delenv("GENREC_DISABLE_PACKED_QKV", raising=False)
    qkv = layer.qkv(x0)
    assert ops.packed_qkv_eligible(qkv, H, None, None, False)
    packed = _layer_run(layer, x0, pad)
    monkeypatch.setenv("GENREC_DISABLE_PACKED_QKV", "1")
    assert not ops.packed_qkv_eligible(qkv, H, None, None, False)
    chunk = _layer_run(layer, x0, pad)
    for name in packed:
        assert packed[name] is not None and chunk[name] is not None, name
        assert torch.isfinite(packed[name].float()).all(), name
        assert torch.equal(packed[name], chunk[name]), (
            name,
            (packed[name].float() - chunk[name].float()).abs().max().item())
    assert packed["dqkv_w"].abs().max() > 0
