"""ops.dropout_add_rms_norm on CPU is the composed eager pair, and the
transformer wiring built on it leaves the blocks' results unchanged."""

import pytest
import torch
import torch.nn.functional as F

from genrec_amd import ops
from genrec_amd.modules.norms import RMSNorm, T5RMSNorm
from genrec_amd.modules.transformer import (
    TransformerBlock, TransformerEncoderDecoder,
)
from genrec_amd.ops import eager


def _inputs(dtype):
    g = torch.Generator().manual_seed(0)
    y = torch.randn(3, 5, 32, generator=g).to(dtype).requires_grad_()
    res = torch.randn(3, 5, 32, generator=g).to(dtype).requires_grad_()
    w = (1.0 + 0.1 * torch.randn(32, generator=g)).requires_grad_()
    return y, res, w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("t5", [True, False])
def test_eval_equals_composed_eager(dtype, t5):
    y, res, w = _inputs(dtype)
    h, n = ops.dropout_add_rms_norm(y, res, w, 0.1, 1e-6, t5, False)
    h_ref = res + y
    assert torch.equal(h, h_ref)
    assert torch.equal(n, eager.rms_norm(h_ref, w, 1e-6, t5))


@pytest.mark.parametrize("t5", [True, False])
def test_training_equals_composed_eager_with_same_seed(t5):
    y, res, w = _inputs(torch.float32)
    torch.manual_seed(3)
    h, n = ops.dropout_add_rms_norm(y, res, w, 0.3, 1e-6, t5, True)
    grads = torch.autograd.grad((h.sum() + (n * n).sum()), (y, res, w))
    torch.manual_seed(3)
    h_ref = res + F.dropout(y, p=0.3, training=True)
    n_ref = eager.rms_norm(h_ref, w, 1e-6, t5)
    ref = torch.autograd.grad((h_ref.sum() + (n_ref * n_ref).sum()),
                              (y, res, w))
    assert torch.equal(h, h_ref) and torch.equal(n, n_ref)
    assert not torch.equal(h, res + y)
    for a, b in zip(grads, ref):
        assert torch.equal(a, b)


def _reference_block(blk, x, context=None):
    """The block as written before the fused wiring."""
    x = x + blk.self_attn(blk.norm1(x))
    if blk.cross_attn_enabled and context is not None:
        x = x + blk.cross_attn(blk.norm_cross(x), key=context, value=context)
    return x + blk.ff(blk.norm2(x))


@pytest.mark.parametrize("norm_cls", [RMSNorm, T5RMSNorm, torch.nn.LayerNorm])
@pytest.mark.parametrize("cross", [False, True])
def test_block_alone_returns_tensor(norm_cls, cross):
    torch.manual_seed(0)
    blk = TransformerBlock(32, 2, dropout=0.1, norm_cls=norm_cls,
                           ff_hidden_dim=64, cross_attn=cross).eval()
    x = torch.randn(2, 5, 32)
    ctx = torch.randn(2, 3, 32) if cross else None
    out = blk(x, context=ctx)
    assert isinstance(out, torch.Tensor)
    assert torch.equal(out, _reference_block(blk, x, ctx))
    # handing over to a following norm returns that norm's output too
    nxt = norm_cls(32)
    out2, normed = blk(x, context=ctx, next_norm=nxt)
    assert torch.equal(out2, out) and torch.equal(normed, nxt(out))
    assert torch.equal(blk(x, context=ctx, normed=blk.norm1(x)), out)


@pytest.mark.parametrize("norm_cls", [T5RMSNorm, torch.nn.LayerNorm])
def test_stack_equals_blocks_one_by_one(norm_cls):
    torch.manual_seed(0)
    m = TransformerEncoderDecoder(32, 2, 2, 2, dim_feedforward=64,
                                  dropout=0.1, norm_cls=norm_cls).eval()
    src, tgt = torch.randn(2, 5, 32), torch.randn(2, 3, 32)
    tgt_mask = torch.triu(torch.full((3, 3), float("-inf")), diagonal=1)
    mem = src
    for blk in m.encoder.layers:
        mem = blk(mem)
    ref = tgt
    for blk in m.decoder.layers:
        ref = blk(ref, context=mem, attn_mask=tgt_mask)
    assert torch.equal(m(src, tgt), ref)
