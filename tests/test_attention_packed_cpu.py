"""Packed qkv route of T5Attention: eligibility, and the CPU route it must
leave alone."""

import torch

from genrec_amd import ops
from genrec_amd.modules.transformer import T5Attention
from genrec_amd.ops.attention import _packed_qkv_fits

H, D = 2, 64


def _qkv(l=8, dtype=torch.bfloat16):
    return torch.zeros(2, l, 3 * H * D, dtype=dtype)


def test_not_eligible_on_cpu():
    """a CPU tensor that meets every other condition stays on the chunk
    route"""
    assert _packed_qkv_fits(_qkv(), H, None, None, False)
    assert _packed_qkv_fits(_qkv(), H, torch.zeros(8, 8), None, False)
    assert not ops.packed_qkv_eligible(_qkv(), H)
    assert not ops.packed_qkv_eligible(_qkv(), H, torch.zeros(8, 8), None,
                                       False)


def test_conditions():
    """a kv_cache, fp32, L > 64, table-bias mode, a head width the MFMA
    kernels do not take and a batched additive mask each rule the packed
    route out, before the device is looked at"""
    cases = [
        (_qkv(), H, None, {}, False),
        (_qkv(dtype=torch.float32), H, None, None, False),
        (_qkv(l=65), H, None, None, False),
        (_qkv(), H, None, None, True),
        (_qkv(), 8, None, None, False),                      # D = 16
        (_qkv(), 1, None, None, False),                      # D = 128
        (_qkv(), H, torch.zeros(2, 8, 8), None, False),
    ]
    for case in cases:
        assert not _packed_qkv_fits(*case)
        assert not ops.packed_qkv_eligible(*case)
    assert _packed_qkv_fits(_qkv(l=64), H, None, None, False)


def test_cpu_layer_forward_backward():
    torch.manual_seed(0)
    layer = T5Attention(128, H, dropout=0.0)
    x = torch.randn(2, 5, 128, requires_grad=True)
    pad = torch.zeros(2, 5, dtype=torch.bool)
    pad[1, 3:] = True
    out = layer(x, key_padding_mask=pad)
    assert out.shape == (2, 5, 128)
    out.sum().backward()
    for g in (x.grad, layer.qkv.weight.grad, layer.rel_bias.weight.grad):
        assert g is not None and torch.isfinite(g).all()
    assert layer.qkv.weight.grad.abs().max() > 0
    # incremental decode with a kv_cache keeps the chunk route
    layer.eval()
    cache = {}
    with torch.no_grad():
        step0 = layer(x[:, :3], kv_cache=cache)
        step1 = layer(x[:, 3:4], kv_cache=cache)
    assert step0.shape == (2, 3, 128) and step1.shape == (2, 1, 128)
    assert cache["k"].shape == (2, H, 4, 64)
