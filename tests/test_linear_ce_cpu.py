"""ops.linear_cross_entropy on the plain-PyTorch path (ops/eager.py): the
compaction + chunk loop against F.cross_entropy(F.linear(h, w), t), and the
LCRec `loss_implementation="genrec_lce"` switch against the backbone's own
loss. Everything here runs without a GPU."""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from genrec_amd import ops

N, H, V = 37, 16, 101
IGNORE = -100


@functools.lru_cache(maxsize=None)
def _inputs(dtype, ignored):
    g = torch.Generator().manual_seed(7)
    h = torch.randn(N, H, generator=g, dtype=dtype)
    w = torch.randn(V, H, generator=g, dtype=dtype) * 0.5
    t = torch.randint(0, V, (N,), generator=g)
    t[0], t[1] = 0, V - 1
    if ignored == "some":
        t[torch.rand(N, generator=g) < 0.6] = IGNORE
        t[2], t[3] = IGNORE, 5          # both kinds are present
    elif ignored == "all":
        t[:] = IGNORE
    return h, w, t


def _reference(h, w, t, reduction):
    h, w = h.clone().requires_grad_(), w.clone().requires_grad_()
    if (t != IGNORE).any():
        loss = F.cross_entropy(F.linear(h, w), t, ignore_index=IGNORE,
                               reduction=reduction)
    else:       # F.cross_entropy's mean is 0/0 here; the op defines it as 0
        loss = (F.linear(h, w) * 0).sum()
    loss.backward()
    return loss.detach(), h.grad, w.grad


def _run(h, w, t, scale=1.0, **kw):
    h, w = h.clone().requires_grad_(), w.clone().requires_grad_()
    loss = ops.linear_cross_entropy(h, w, t, ignore_index=IGNORE, **kw)
    assert type(loss.grad_fn).__name__ == "_LinearCEEagerFnBackward"
    (loss * scale).backward()
    return loss.detach(), h.grad, w.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("ignored", ["some", "none", "all"])
@pytest.mark.parametrize("chunk_rows", [N, 8, 1])
@pytest.mark.parametrize("compact", [True, False])
def test_matches_composition(dtype, reduction, ignored, chunk_rows, compact):
    h, w, t = _inputs(dtype, ignored)
    ref = _reference(h, w, t, reduction)
    got = _run(h, w, t, reduction=reduction, chunk_rows=chunk_rows,
               compact=compact)
    for name, a, b in zip(("loss", "dhidden", "dweight"), got, ref):
        assert a.dtype == dtype and a.shape == b.shape, name
        torch.testing.assert_close(a, b, msg=lambda m: f"{name}: {m}")
    if ignored == "all":
        assert got[0].item() == 0.0
        assert not got[1].any() and not got[2].any()
    if ignored == "some":          # ignored rows get exactly zero gradient
        assert not got[1][t == IGNORE].any()


def test_default_chunk_rows_and_nd_inputs():
    h, w, t = _inputs(torch.float32, "some")
    ref = _reference(h, w, t, "mean")
    got = _run(h, w, t)
    torch.testing.assert_close(got[0], ref[0])
    # [B, L, H] hidden with [B, L] targets
    h3 = torch.cat([h, h[:3]]).reshape(4, 10, H)
    t3 = torch.cat([t, t[:3]]).reshape(4, 10)
    a = ops.linear_cross_entropy(h3, w, t3)
    b = F.cross_entropy(F.linear(h3, w).reshape(-1, V), t3.reshape(-1),
                        ignore_index=IGNORE)
    torch.testing.assert_close(a, b)


@pytest.mark.parametrize("chunk_rows", [N, 8])
def test_scaled_loss_scales_gradients(chunk_rows):
    h, w, t = _inputs(torch.float32, "some")
    _, dh1, dw1 = _run(h, w, t, chunk_rows=chunk_rows)
    _, dh4, dw4 = _run(h, w, t, scale=0.25, chunk_rows=chunk_rows)
    torch.testing.assert_close(dh4, dh1 * 0.25)
    torch.testing.assert_close(dw4, dw1 * 0.25)


def test_no_grad_and_partial_requires_grad():
    h, w, t = _inputs(torch.float32, "some")
    ref = _reference(h, w, t, "mean")
    with torch.no_grad():
        loss = ops.linear_cross_entropy(h.clone().requires_grad_(), w, t)
    assert not loss.requires_grad
    torch.testing.assert_close(loss, ref[0])
    # only the weight needs a gradient
    w2 = w.clone().requires_grad_()
    ops.linear_cross_entropy(h, w2, t, chunk_rows=8).backward()
    torch.testing.assert_close(w2.grad, ref[2])


def test_autocast_returns_parameter_dtype_grads():
    h, w, t = _inputs(torch.float32, "some")
    h, w = h.clone().requires_grad_(), w.clone().requires_grad_()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        loss = ops.linear_cross_entropy(h, w, t)
    loss.backward()
    assert loss.dtype == torch.float32
    assert h.grad.dtype == torch.float32 and w.grad.dtype == torch.float32
    ref = _reference(h.detach(), w.detach(), t, "mean")
    # bf16 operands: 2^-8 relative on O(1) logits
    torch.testing.assert_close(loss.detach(), ref[0], atol=0.05, rtol=0.05)


def test_bf16_chunks_accumulate_dweight_in_fp32():
    h, w, t = _inputs(torch.float32, "some")
    hb, wb = h.to(torch.bfloat16), w.to(torch.bfloat16)
    ref = _reference(hb.float(), wb.float(), t, "mean")
    one = _run(hb, wb, t, chunk_rows=N)
    many = _run(hb, wb, t, chunk_rows=1)
    # bf16 logits are off by e <= 2^-9 max|logit|, which moves the loss by
    # at most 2e and every probability by a factor within exp(+-2e); dlogits
    # and the results are then rounded to bf16 (2^-9 relative each)
    e = 2 ** -9 * F.linear(hb.float(), wb.float()).abs().max().item()
    for a, b, r in zip(one, many, ref):
        assert a.dtype == b.dtype
        bound = (2 * e + 2 ** -7) * max(r.abs().max().item(), 1.0)
        assert (a.float() - r).abs().max().item() <= bound
        assert (b.float() - r).abs().max().item() <= bound
        # the two arms round the same fp32-accumulated values to bf16 once
        # each (2^-9 relative), up to summation order
        assert (a.float() - b.float()).abs().max().item() \
            <= 2 ** -7 * a.float().abs().max().item()
    assert one[2].dtype == torch.bfloat16


def test_rejects_unknown_reduction():
    h, w, t = _inputs(torch.float32, "none")
    with pytest.raises(ValueError, match="reduction"):
        ops.linear_cross_entropy(h, w, t, reduction="none")


# --------------------------------------------------------------- model level

QWEN = dict(vocab_size=512, hidden_size=64, num_layers=2, num_heads=4,
            num_kv_heads=2, intermediate_size=256)


@functools.lru_cache(maxsize=None)
def _models():
    from genrec_amd.models.lcrec import LCRec, default_qwen_config

    torch.manual_seed(0)
    stock = LCRec(config=default_qwen_config(**QWEN),
                  attn_implementation="sdpa")
    stock.add_codebook_tokens(3, 8)
    stock.eval()
    lce = copy.deepcopy(stock)
    lce.loss_implementation = "genrec_lce"
    torch.manual_seed(1)
    ids = torch.randint(0, 256, (3, 19))
    attn = torch.ones_like(ids)
    attn[1, 12:] = 0
    labels = ids.masked_fill(attn == 0, -100)
    labels[:, :7] = -100                      # the prompt carries no loss
    return stock, lce, ids, attn, labels


def test_model_loss_and_grads_match_stock_path():
    stock, lce, ids, attn, labels = _models()
    outs = {}
    for name, m in (("stock", stock), ("lce", lce)):
        m.zero_grad()
        out = m(ids, attn, labels=labels)
        out.loss.backward()
        outs[name] = (out, {k: p.grad.clone()
                            for k, p in m.named_parameters()
                            if p.grad is not None})
        m.zero_grad()
    assert outs["lce"][0].logits is None
    assert outs["stock"][0].logits is not None
    torch.testing.assert_close(outs["lce"][0].loss, outs["stock"][0].loss)
    assert outs["lce"][1].keys() == outs["stock"][1].keys()
    for k, g in outs["stock"][1].items():
        torch.testing.assert_close(outs["lce"][1][k], g,
                                   msg=lambda m: f"{k}: {m}")


def test_model_without_labels_is_identical():
    stock, lce, ids, attn, _ = _models()
    with torch.no_grad():
        a = stock(ids, attn)
        b = lce(ids, attn)
    assert a.loss is None and b.loss is None
    assert torch.equal(a.logits, b.logits)


def test_model_constructor_and_fallback(caplog):
    from genrec_amd.models.lcrec import LCRec, default_qwen_config

    with pytest.raises(ValueError, match="loss_implementation"):
        LCRec(config=default_qwen_config(**QWEN), loss_implementation="nope")
    _, lce, ids, attn, labels = _models()
    wrapped = copy.copy(lce)                   # shares the parameters

    class Opaque(torch.nn.Module):             # hides .model / .lm_head
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, **kw):
            return self.inner(**kw)

    class PeftLike(Opaque):        # forwards .model to the causal LM itself
        def __init__(self, inner):
            super().__init__(inner)
            self.model = inner
            self.lm_head = inner.lm_head

    for wrapper in (Opaque, PeftLike):
        wrapped._modules = dict(lce._modules)
        wrapped.model = wrapper(lce.model)
        wrapped._lce_fallback_logged = False
        caplog.clear()
        with caplog.at_level("WARNING", logger="genrec_amd"):
            with torch.no_grad():
                out = wrapped(ids, attn, labels=labels)
                wrapped(ids, attn, labels=labels)
        assert out.logits is not None and torch.isfinite(out.loss)
        assert sum("genrec_lce" in r.getMessage()
                   for r in caplog.records) == 1
