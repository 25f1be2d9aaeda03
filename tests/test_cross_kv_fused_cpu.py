"""Fused cross-attention K/V projection: the autograd plumbing, without a GPU.

ops.project_cross_kv projects the encoder memory to every decoder layer's
K/V in one GEMM and ops.cross_attention_kv attends on two column blocks of
the result; the layers' backward nodes share one gradient buffer that
exactly one of them hands to autograd. impl="torch" runs the same two
autograd nodes in plain PyTorch, here in fp64, where the fused and the
per-layer route differ only in summation order.
"""

import pytest
import torch

from genrec_amd import ops
from genrec_amd.ops import cross_kv as ckv_mod
from genrec_amd.ops import eager
from genrec_amd.modules.transformer import TransformerDecoder

D_MODEL, H, B, LQ, LK = 128, 2, 2, 4, 5
RTOL = 1e-9


def _inputs():
    g = torch.Generator().manual_seed(3)
    tgt = torch.randn(B, LQ, D_MODEL, generator=g, dtype=torch.float64)
    memory = torch.randn(B, LK, D_MODEL, generator=g, dtype=torch.float64)
    pad = torch.zeros(B, LK, dtype=torch.bool)
    pad[1, LK - 2:] = True          # one row with a padded tail
    return tgt, memory, pad


def _decoder(n_layers):
    torch.manual_seed(11)
    return TransformerDecoder(D_MODEL, n_layers, H, dropout=0.0,
                              ff_hidden_dim=64).double().train()


def _run(dec, impl, no_grad=False):
    tgt0, mem0, pad = _inputs()
    dec.zero_grad(set_to_none=True)
    tgt, mem = tgt0.clone().requires_grad_(), mem0.clone().requires_grad_()
    if no_grad:
        with torch.no_grad():
            return dict(out=dec(tgt, memory=mem,
                                memory_key_padding_mask=pad,
                                cross_kv_impl=impl))
    out = dec(tgt, memory=mem, memory_key_padding_mask=pad,
              cross_kv_impl=impl)
    w = torch.linspace(-1.0, 1.0, out.numel(), dtype=out.dtype).view_as(out)
    (out * w).sum().backward()
    res = dict(out=out.detach(), d_memory=mem.grad, d_tgt=tgt.grad)
    for name, p in dec.named_parameters():
        res["d_" + name] = p.grad
    return res


@pytest.fixture(scope="module", params=[2, 3], ids=["2layers", "3layers"])
def routes(request):
    dec = _decoder(request.param)
    per_layer = _run(dec, None)
    fused = _run(dec, "torch")
    return request.param, dec, per_layer, fused


def test_fused_route_matches_per_layer_route(routes):
    n, dec, per_layer, fused = routes
    kv_names = [f"d_layers.{i}.cross_attn.{w}.weight"
                for i in range(n) for w in ("k", "v")]
    assert set(kv_names) <= set(fused) and len(kv_names) == 2 * n
    assert set(fused) == set(per_layer)
    for name in fused:
        assert fused[name] is not None, name
        assert fused[name].abs().max() > 0, name
        torch.testing.assert_close(fused[name], per_layer[name], rtol=RTOL,
                                   atol=0, msg=lambda m: f"{name}: {m}")


def test_kv_weight_grads_are_slices_of_one_tensor(routes):
    """the per-parameter gradients are taken as they come: row slices of
    the one stacked weight gradient, no copy per parameter"""
    n, dec, _, _ = routes
    _run(dec, "torch")
    ptrs = {getattr(layer.cross_attn, w).weight.grad.untyped_storage()
            .data_ptr() for layer in dec.layers for w in ("k", "v")}
    assert len(ptrs) == 1
    for layer in dec.layers:
        assert layer.cross_attn.k.weight.grad.is_contiguous()


def test_repeat_and_no_grad(routes):
    n, dec, _, fused = routes
    again = _run(dec, "torch")
    for name in fused:
        assert torch.equal(again[name], fused[name]), name
    quiet = _run(dec, "torch", no_grad=True)
    assert not quiet["out"].requires_grad
    assert torch.equal(quiet["out"], fused["out"])


def test_cpu_modules_take_the_per_layer_route(monkeypatch):
    calls = []
    real = ops.project_cross_kv

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "project_cross_kv", spy)
    dec = _decoder(2)
    res = _run(dec, None)
    assert not calls
    _run(dec, "torch")
    assert calls == [1]
    # and the graph of the default route has none of the new nodes
    tgt, mem, pad = _inputs()
    out = dec(tgt, memory=mem.requires_grad_(), memory_key_padding_mask=pad)
    seen, todo = set(), [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(f for f, _ in fn.next_functions)
    names = {type(fn).__name__ for fn in seen}
    assert not any("ProjectKV" in s or "CrossAttnKV" in s for s in names)
    assert res["out"] is not None


@pytest.mark.parametrize("n_layers", [2, 3])
def test_subset_of_layers(monkeypatch, n_layers):
    """Only the last layer's cross attention enters the loss. The gradient
    buffer starts as NaN here, so a block that nobody wrote and nobody
    zeroed would show."""
    monkeypatch.setattr(
        ckv_mod, "_new_grad_buffer",
        lambda shape, dtype, device: torch.full(
            shape, float("nan"), dtype=dtype, device=device))
    g = torch.Generator().manual_seed(5)
    _, mem0, pad = _inputs()
    d_head = D_MODEL // H
    q0 = torch.randn(B, H, LQ, d_head, generator=g, dtype=torch.float64)
    kws = [torch.randn(D_MODEL, D_MODEL, generator=g, dtype=torch.float64)
           .requires_grad_() for _ in range(n_layers)]
    vws = [torch.randn(D_MODEL, D_MODEL, generator=g, dtype=torch.float64)
           .requires_grad_() for _ in range(n_layers)]
    last = n_layers - 1
    scale = d_head ** -0.5

    mem, q = mem0.clone().requires_grad_(), q0.clone().requires_grad_()
    ckv = ops.project_cross_kv(mem, kws, vws, impl="torch")
    assert ckv.kv_all.shape == (B, LK, n_layers * 2 * D_MODEL)
    out = ops.cross_attention_kv(q, ckv, last, pad, scale, 0.0, True)
    w = torch.linspace(-1.0, 1.0, out.numel(), dtype=out.dtype).view_as(out)
    (out * w).sum().backward()

    mem_r, q_r = mem0.clone().requires_grad_(), q0.clone().requires_grad_()
    kw_r = kws[last].detach().clone().requires_grad_()
    vw_r = vws[last].detach().clone().requires_grad_()

    def split(x):
        return x.view(B, LK, H, d_head).transpose(1, 2)

    ref = eager.fused_attention(q_r, split(mem_r @ kw_r.t()),
                                split(mem_r @ vw_r.t()), scale=scale,
                                key_pad_mask=pad)
    (ref * w).sum().backward()

    torch.testing.assert_close(out, ref, rtol=RTOL, atol=0)
    torch.testing.assert_close(q.grad, q_r.grad, rtol=RTOL, atol=0)
    torch.testing.assert_close(mem.grad, mem_r.grad, rtol=RTOL, atol=0)
    torch.testing.assert_close(kws[last].grad, kw_r.grad, rtol=RTOL, atol=0)
    torch.testing.assert_close(vws[last].grad, vw_r.grad, rtol=RTOL, atol=0)
    for i in range(last):
        for p in (kws[i], vws[i]):
            assert p.grad is not None and torch.equal(
                p.grad, torch.zeros_like(p))


def test_a_layer_reads_its_blocks_once():
    _, mem, pad = _inputs()
    w = [torch.eye(D_MODEL, dtype=torch.float64) for _ in range(2)]
    ckv = ops.project_cross_kv(mem, w, w, impl="torch")
    q = torch.zeros(B, H, LQ, D_MODEL // H, dtype=torch.float64)
    ops.cross_attention_kv(q, ckv, 0, pad, 1.0, 0.0, False)
    with pytest.raises(RuntimeError, match="twice"):
        ops.cross_attention_kv(q, ckv, 0, pad, 1.0, 0.0, False)
    with pytest.raises(IndexError):
        ops.cross_attention_kv(q, ckv, 2, pad, 1.0, 0.0, False)


def test_another_consumer_of_kv_all_is_an_error():
    _, mem0, pad = _inputs()
    mem = mem0.clone().requires_grad_()
    w = [torch.eye(D_MODEL, dtype=torch.float64) for _ in range(2)]
    ckv = ops.project_cross_kv(mem, w, w, impl="torch")
    q = torch.ones(B, H, LQ, D_MODEL // H, dtype=torch.float64)
    out = ops.cross_attention_kv(q, ckv, 0, pad, 1.0, 0.0, False)
    with pytest.raises(RuntimeError, match="no other consumer"):
        (out.sum() + ckv.kv_all.sum()).backward()


def _fits_args(dtype=torch.bfloat16, n=2, bias=False, lq=LQ, lk=LK):
    mem = torch.zeros(B, lk, D_MODEL, dtype=dtype)
    tgt = torch.zeros(B, lq, D_MODEL, dtype=dtype)
    kws = [torch.zeros(D_MODEL, D_MODEL, dtype=dtype) for _ in range(n)]
    vws = [torch.zeros(D_MODEL, D_MODEL, dtype=dtype) for _ in range(n)]
    biases = [None] * (2 * n)
    if bias:
        biases[1] = torch.zeros(D_MODEL, dtype=dtype)
    return [mem, tgt, kws, vws, biases, H, None]


def test_gates(monkeypatch):
    for knob in ckv_mod._ROUTING_KNOBS:
        monkeypatch.delenv(knob, raising=False)
    fits = ckv_mod._cross_kv_fits
    assert fits(*_fits_args())
    args = _fits_args()
    args[6] = [{}, {}]
    assert not fits(*args)                          # kv_caches
    assert not fits(*_fits_args(dtype=torch.float32))
    assert not fits(*_fits_args(bias=True))
    args = _fits_args()
    args[3][1] = torch.zeros(2 * D_MODEL, D_MODEL, dtype=torch.bfloat16)
    assert not fits(*args)                          # mismatched layers
    assert not fits(*_fits_args(lq=65))
    assert not fits(*_fits_args(lk=65))
    # CPU tensors that fit are still not eligible
    assert not ops.cross_kv_eligible(*_fits_args())
    assert ckv_mod._route_enabled()
    assert set(ckv_mod._ROUTING_KNOBS) == {
        "GENREC_DISABLE_CROSS_KV_FUSE", "GENREC_DISABLE_ATTN",
        "GENREC_DISABLE_MFMA", "GENREC_FORCE_FLASH"}
    for knob in ckv_mod._ROUTING_KNOBS:
        monkeypatch.setenv(knob, "1")
        assert not ckv_mod._route_enabled(), knob
        monkeypatch.delenv(knob)
    assert ckv_mod._route_enabled()
