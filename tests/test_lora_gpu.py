"""LoRA adapter kernels (csrc/kernels/lora.hip) and ops.lora_linear on the
GPU, bf16.

Yardstick: kernel and stock bf16 composition (peft's order: dropout, two
F.linear, scale, add; autograd for the gradients) are both diffed against a
float64 reference computed from the same bf16 inputs and the same mask, and
for every output tensor

    max|kernel - ref| <= 2 * max|stock_bf16 - ref|

Every comparison prints its two errors and their ratio. Shapes: M in
{1, 17, 130} (below a fragment, ragged, more than one 64-row tile with a
ragged tail), (K, N) in {(64, 8), (72, 40), (200, 136)} (multiples of 8,
not of 64), r in {16, 32, 64}, p in {0, 0.25}.
"""

import copy
import math

import pytest
import torch
import torch.nn.functional as F

from genrec_amd import ops
from genrec_amd.ops import eager
from genrec_amd.ops import lora as lora_ops

pytestmark = pytest.mark.gpu

MS = (1, 17, 130)
KNS = ((64, 8), (72, 40), (200, 136))
RANKS = (16, 32, 64)
PS = (0.0, 0.25)
SEED = 4321
S = 2.0                                   # alpha / r of the default config


def _dev():
    return torch.device("cuda:0")


def _ext():
    return ops.ext()


def _rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16) \
        .to(_dev())


def _held(label, got, stock, ref):
    ref = ref.double()
    assert got.shape == ref.shape, label
    assert torch.isfinite(got.float()).all(), f"{label} not finite"
    err_k = (got.double() - ref).abs().max().item()
    err_b = (stock.double() - ref).abs().max().item()
    ratio = err_k / err_b if err_b > 0 else (0.0 if err_k == 0 else math.inf)
    print(f"{label}: kernel {err_k:.3e} stock_bf16 {err_b:.3e} "
          f"ratio {ratio:.2f}")
    assert err_k <= 2 * err_b, (label, err_k, err_b)


def _mask(M, Kw, p):
    """float64 keep mask on the device (ones for p = 0)"""
    if p == 0.0:
        return torch.ones(M, Kw, dtype=torch.float64, device=_dev())
    return eager.lora_dropout_mask(M, Kw, p, SEED, _dev()).double()


def _stock_dropout(x, mask, p):
    """what torch's dropout kernel computes for this mask: one rounding"""
    if p == 0.0:
        return x
    return (x.float() * mask.float() * (1.0 / (1.0 - p))).to(x.dtype)


class _StockDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, p):
        ctx.mask, ctx.p = mask, p
        return _stock_dropout(x, mask, p)

    @staticmethod
    def backward(ctx, dy):
        return _stock_dropout(dy, ctx.mask, ctx.p), None, None


def _ulp_bf16(t):
    a = t.float().abs().clamp_min(2.0 ** -120)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


# ----------------------------------------------------------------- mask

@pytest.mark.parametrize("p", [0.05, 0.25])
def test_mask_equals_eager(p):
    for M, Kw in ((1, 8), (17, 72), (130, 200), (64, 1000)):
        got = _ext().lora_dropout_mask(M, Kw, p, SEED)
        assert got.dtype == torch.uint8 and got.is_cuda
        assert torch.equal(got.cpu(), eager.lora_dropout_mask(M, Kw, p, SEED))
    big = 2**31 - 5                                   # seed near the top
    assert torch.equal(_ext().lora_dropout_mask(9, 40, p, big).cpu(),
                       eager.lora_dropout_mask(9, 40, p, big))


# ------------------------------------------------------ each kernel alone

@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("r", RANKS)
def test_lora_down(r, p):
    g = torch.Generator().manual_seed(r)
    for M in MS:
        for Kw in (64, 72, 200):
            x, pm = _rnd(g, M, Kw), _rnd(g, r, Kw, scale=Kw ** -0.5)
            mask = _mask(M, Kw, p)
            c = 1.0 / (1.0 - p) if p else S
            got = _ext().lora_down(x, pm, c, p, SEED)
            ref = c * ((x.double() * mask) @ pm.double().t())
            if p:   # forward use: t = dropout(x) A^T
                stock = F.linear(_stock_dropout(x, mask, p), pm)
            else:   # backward use: dt = s * dy B
                stock = F.linear(x, pm) * c
                f32 = (c * (x.float() @ pm.float().t())).to(torch.bfloat16)
                assert ((got.float() - f32.float()).abs()
                        <= _ulp_bf16(f32)).all(), (M, Kw, r)
            _held(f"down M{M} Kw{Kw} r{r} p{p}", got, stock, ref)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("r", RANKS)
def test_lora_up_add(r, p):
    g = torch.Generator().manual_seed(100 + r)
    for M in MS:
        for Kw in (8, 40, 136, 200):
            y, t = _rnd(g, M, Kw), _rnd(g, M, r)
            q = _rnd(g, Kw, r, scale=r ** -0.5)
            mask = _mask(M, Kw, p)
            c = 1.0 / (1.0 - p) if p else S
            ref = y.double() + c * mask * (t.double() @ q.double().t())
            if p:   # backward use: dx += dropout'(dt A)
                stock = y + _stock_dropout(F.linear(t, q), mask, p)
            else:   # forward use: y += s * t B^T
                stock = y + F.linear(t, q) * c
            got = y.clone()
            out = _ext().lora_up_add_(got, t, q, c, p, SEED)
            assert out.data_ptr() == got.data_ptr()
            _held(f"up_add M{M} Kw{Kw} r{r} p{p}", got, stock, ref)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("r", RANKS)
def test_lora_grad(r, p):
    g = torch.Generator().manual_seed(200 + r)
    for M in MS:
        for Kw in (8, 72, 200):
            t, x = _rnd(g, M, r), _rnd(g, M, Kw)
            mask = _mask(M, Kw, p)
            c = 1.0 / (1.0 - p) if p else S
            got = _ext().lora_grad(t, x, c, p, SEED)
            ref = c * (t.double().t() @ (x.double() * mask))
            if p:   # dA = dt^T dropout(x)
                stock = t.t() @ _stock_dropout(x, mask, p)
            else:   # dB^T = s * t^T dy
                stock = (t.t() @ x) * c
            _held(f"grad M{M} Kw{Kw} r{r} p{p}", got, stock, ref)


def test_lora_grad_many_row_chunks():
    """more rows than one chunk of 64-row tiles: the fixed-order second
    stage sums several partials (8 strips -> 64 chunks of one tile)"""
    g = torch.Generator().manual_seed(7)
    M, Kw, r, p = 64 * 70 + 5, 72, 16, 0.25
    t, x = _rnd(g, M, r), _rnd(g, M, Kw)
    mask = _mask(M, Kw, p)
    c = 1.0 / (1.0 - p)
    got = _ext().lora_grad(t, x, c, p, SEED)
    ref = c * (t.double().t() @ (x.double() * mask))
    stock = t.t() @ _stock_dropout(x, mask, p)
    _held("grad chunks", got, stock, ref)
    assert torch.equal(got, _ext().lora_grad(t, x, c, p, SEED))


# ------------------------------------------------------------ end to end

def _layouts(g, M, K):
    """x as a contiguous tensor, as [B, L, K], as a column slice"""
    flat = _rnd(g, M, K)
    yield "contiguous", flat
    if M % 2 == 0:
        yield "3d", flat.view(2, M // 2, K)
    else:
        yield "3d", flat.view(1, M, K)
    wide = _rnd(g, M, K + 24)
    wide[:, :K] = flat
    yield "slice", wide[:, :K]


def _end_to_end(x, w, b, a, bb, p, fn):
    """(y, dx, dA, dB, dweight, dbias) of fn on fresh leaves"""
    leaves = [t.detach().clone().requires_grad_(True)
              for t in (x, w, b, a, bb)]
    y = fn(*leaves)
    g = torch.Generator().manual_seed(5)
    dy = _rnd(g, *y.shape).to(y.dtype)        # the same bf16 values
    grads = torch.autograd.grad(y, leaves, dy)
    return (y,) + tuple(grads)


def _reference(x, w, b, a, bb, p):
    M = x.numel() // x.size(-1)
    mask = _mask(M, x.size(-1), p).view(x.shape)
    keep = 1.0 - p

    def ref_fn(x, w, b, a, bb):
        xd = x * mask / keep
        return F.linear(x, w, b) + S * F.linear(F.linear(xd, a), bb)

    def stock_fn(x, w, b, a, bb):
        xd = _StockDropout.apply(x, mask, p)
        return F.linear(x, w, b) + F.linear(F.linear(xd, a), bb) * S

    ref = _end_to_end(*(t.double() for t in (x, w, b, a, bb)), p, ref_fn)
    # the float64 run draws dy as bf16 and autograd upcasts it: same dy
    stock = _end_to_end(x, w, b, a, bb, p, stock_fn)
    return ref, stock


NAMES = ("y", "dx", "dA", "dB", "dweight", "dbias")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("r", RANKS)
def test_lora_linear_end_to_end(r, p):
    g = torch.Generator().manual_seed(300 + r)
    for M in MS:
        for K, N in KNS:
            w, b = _rnd(g, N, K, scale=K ** -0.5), _rnd(g, N)
            a = _rnd(g, r, K, scale=K ** -0.5)
            bb = _rnd(g, N, r, scale=r ** -0.5)
            for layout, x in _layouts(g, M, K):
                assert lora_ops.lora_eligible(x, w, b, a, bb), layout
                ref, stock = _reference(x, w, b, a, bb, p)
                got = _end_to_end(
                    x, w, b, a, bb, p,
                    lambda *t: ops.lora_linear(*t, S, p=p, training=True,
                                               seed=SEED))
                for name, k_, s_, r_ in zip(NAMES, got, stock, ref):
                    _held(f"{name} M{M} K{K} N{N} r{r} p{p} {layout}",
                          k_, s_, r_)


def test_determinism_and_seed():
    g = torch.Generator().manual_seed(11)
    M, K, N, r, p = 130, 200, 136, 16, 0.25
    x, w, b = _rnd(g, M, K), _rnd(g, N, K, scale=K ** -0.5), _rnd(g, N)
    a, bb = _rnd(g, r, K, scale=K ** -0.5), _rnd(g, N, r, scale=0.25)
    run = lambda seed: _end_to_end(
        x, w, b, a, bb, p,
        lambda *t: ops.lora_linear(*t, S, p=p, training=True, seed=seed))
    one, two, other = run(SEED), run(SEED), run(SEED + 1)
    for name, u, v in zip(NAMES, one, two):
        assert torch.equal(u, v), name
    assert not torch.equal(one[0], other[0])
    assert not torch.equal(_ext().lora_dropout_mask(M, K, p, SEED),
                           _ext().lora_dropout_mask(M, K, p, SEED + 1))


def test_up_add_in_place_semantics():
    g = torch.Generator().manual_seed(12)
    M, Kw, r = 17, 72, 16
    buf = torch.full((M + 3, Kw + 16), 777.0, dtype=torch.bfloat16,
                     device=_dev())
    y = buf[:M, :Kw]
    y.copy_(_rnd(g, M, Kw))
    before = buf.clone()
    t, q = _rnd(g, M, r), _rnd(g, Kw, r)
    _ext().lora_up_add_(y, t, q, S, 0.0, 0)
    assert not torch.equal(buf[:M, :Kw], before[:M, :Kw])
    assert torch.equal(buf[M:], before[M:])
    assert torch.equal(buf[:, Kw:], before[:, Kw:])
    # B = 0: bit-unchanged
    y2 = before[:M, :Kw].clone()
    _ext().lora_up_add_(y2, t, torch.zeros_like(q), S, 0.0, 0)
    assert torch.equal(y2.view(torch.int16),
                       before[:M, :Kw].contiguous().view(torch.int16))


def test_kill_switch_takes_eager(monkeypatch):
    g = torch.Generator().manual_seed(13)
    M, K, N, r, p = 17, 72, 40, 16, 0.25
    x, w, b = _rnd(g, M, K), _rnd(g, N, K, scale=K ** -0.5), _rnd(g, N)
    a, bb = _rnd(g, r, K, scale=K ** -0.5), _rnd(g, N, r, scale=0.25)
    ref, stock = _reference(x, w, b, a, bb, p)
    monkeypatch.setenv("GENREC_DISABLE_LORA", "1")
    assert not lora_ops.lora_eligible(x, w, b, a, bb)

    def boom(*a, **k):
        raise AssertionError("kernel route taken with the kill switch on")

    monkeypatch.setattr(lora_ops._KernelImpl, "lora_down", boom)
    got = _end_to_end(
        x, w, b, a, bb, p,
        lambda *t: ops.lora_linear(*t, S, p=p, training=True, seed=SEED))
    for name, k_, s_, r_ in zip(NAMES, got, stock, ref):
        _held(f"kill switch {name}", k_, s_, r_)


def test_host_checks_raise_and_op_falls_back():
    g = torch.Generator().manual_seed(14)
    M, K, N = 17, 72, 40
    x, w, b = _rnd(g, M, K), _rnd(g, N, K, scale=K ** -0.5), _rnd(g, N)
    ext = _ext()

    def falls_back(x, w, b, a, bb):
        assert not lora_ops.lora_eligible(x, w, b, a, bb)
        y = ops.lora_linear(x, w, b, a, bb, S)
        want = F.linear(x.double(), w.double(), b.double()) + S * F.linear(
            F.linear(x.double(), a.double()), bb.double())
        torch.testing.assert_close(y.double(), want, rtol=2e-2, atol=2e-2)

    # r = 8
    a8, b8 = _rnd(g, 8, K, scale=0.1), _rnd(g, N, 8, scale=0.1)
    with pytest.raises(RuntimeError, match="rank"):
        ext.lora_down(x, a8, 1.0, 0.0, 0)
    with pytest.raises(RuntimeError, match="rank"):
        ext.lora_up_add_(torch.zeros(M, N, dtype=torch.bfloat16,
                                     device=_dev()),
                         _rnd(g, M, 8), b8, 1.0, 0.0, 0)
    with pytest.raises(RuntimeError, match="rank"):
        ext.lora_grad(_rnd(g, M, 8), x, 1.0, 0.0, 0)
    falls_back(x, w, b, a8, b8)
    # K % 8 != 0
    a, bb = _rnd(g, 16, K, scale=0.1), _rnd(g, N, 16, scale=0.1)
    x4, w4, a4 = _rnd(g, M, K + 4), _rnd(g, N, K + 4, scale=0.1), \
        _rnd(g, 16, K + 4, scale=0.1)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.lora_down(x4, a4, 1.0, 0.0, 0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.lora_grad(_rnd(g, M, 16), x4, 1.0, 0.0, 0)
    falls_back(x4, w4, b, a4, bb)
    # fp16
    with pytest.raises(RuntimeError, match="bf16"):
        ext.lora_down(x.half(), a.half(), 1.0, 0.0, 0)
    with pytest.raises(RuntimeError, match="bf16"):
        ext.lora_down(x, a.half(), 1.0, 0.0, 0)
    falls_back(x.half(), w.half(), b.half(), a.half(), bb.half())
    # non-contiguous last dimension
    xt = _rnd(g, K, M).t()
    assert xt.shape == (M, K) and xt.stride(1) != 1
    with pytest.raises(RuntimeError, match="contiguous last"):
        ext.lora_down(xt, a, 1.0, 0.0, 0)
    with pytest.raises(RuntimeError, match="contiguous last"):
        ext.lora_up_add_(xt, _rnd(g, M, 16), _rnd(g, K, 16), 1.0, 0.0, 0)
    falls_back(xt, w, b, a, bb)
    # a row stride that is no multiple of 8
    odd = _rnd(g, M, K + 4)[:, :K]
    with pytest.raises(RuntimeError, match="row stride"):
        ext.lora_down(odd, a, 1.0, 0.0, 0)
    falls_back(odd, w, b, a, bb)


# ---------------------------------------------------- small-backbone SFT

QWEN = dict(vocab_size=512, hidden_size=256, num_layers=2, num_heads=4,
            num_kv_heads=2, intermediate_size=256)   # head_dim 64


def test_small_backbone_sft_steps():
    from genrec_amd.models.lcrec import LCRec, default_qwen_config
    from genrec_amd.modules import lora
    from genrec_amd.trainers.lcrec_trainer import sft_collate

    torch.manual_seed(0)
    plain = LCRec(config=default_qwen_config(**QWEN),
                  attn_implementation="genrec_gqa",
                  layer_implementation="genrec_fused")
    plain.add_codebook_tokens(3, 8)
    plain = plain.to(_dev()).to(torch.bfloat16).train()
    model = copy.deepcopy(plain)
    assert model.apply_lora(r=16, alpha=32, dropout=0.0) == 14
    model.train()
    base = {k: v.clone() for k, v in model.model.state_dict().items()
            if ".lora_" not in k}

    samples = [{"prompt": f"history: <C0_{i}><C1_{i + 1}><C2_{i + 2}> next",
                "response": f"<C0_{i + 3}><C1_{i}>"} for i in range(4)]
    batch = sft_collate(samples, model, 64, packing=True)
    batch = {k: v.to(_dev()) if torch.is_tensor(v) else v
             for k, v in batch.items()}
    assert "cu_seq_lens" in batch

    with torch.no_grad():
        want = plain(**batch).loss
    params = [p for p in model.parameters() if p.requires_grad]
    assert len(params) == 28
    opt = torch.optim.AdamW(params, lr=1e-3)
    losses = []
    for _ in range(2):
        loss = model(**batch).loss
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.detach())
    print("losses", [l.item() for l in losses], "plain", want.item())
    assert all(torch.isfinite(l) for l in losses)
    assert torch.equal(losses[0], want)               # B = 0
    for k, v in model.model.state_dict().items():
        if ".lora_" not in k:
            assert torch.equal(v, base[k]), k
    assert any(m.lora_B.weight.abs().max() > 0 for m in model.model.modules()
               if isinstance(m, lora.LoRALinear))
