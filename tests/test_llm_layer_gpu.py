"""Fused Qwen2 layer kernels (csrc/kernels/llm_layer.hip) and the
`layer_implementation="genrec_fused"` route on the GPU, bf16.

Tolerance rule (the project's yardstick, test_gqa_attention_gpu.py): the
kernel and the stock bf16 op composition are both diffed against an fp32
reference computed from the same bf16 inputs, and

    max|kernel - ref| <= 2 * max|stock_bf16 - ref| + ulp_bf16(max|ref|)

The three numbers are printed per comparison. RoPE is additionally held,
exactly, to the rounding formulas of the issue written with fp32 torch ops.
"""

import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from genrec_amd import ops
from genrec_amd.ops import eager

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _ulp_bf16(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16) \
        .to(_dev())


def _held(label, got, stock, ref):
    """The yardstick for one tensor (None = an absent gradient = zeros)."""
    ref = ref.float()
    got = torch.zeros_like(ref) if got is None else got.float()
    stock = torch.zeros_like(ref) if stock is None else stock.float()
    assert got.shape == ref.shape, label
    assert torch.isfinite(got).all(), f"{label} not finite"
    err_k = (got - ref).abs().max().item()
    err_b = (stock - ref).abs().max().item()
    bound = 2 * err_b + _ulp_bf16(ref.abs().max().item())
    print(f"{label}: kernel {err_k:.3e} stock_bf16 {err_b:.3e} "
          f"bound {bound:.3e}")
    assert err_k <= bound, (label, err_k, err_b, bound)


def _fn_names(*tensors):
    names, seen = [], set()
    stack = [t.grad_fn for t in tensors]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


# ------------------------------------------------------------- add_rms_norm

NORM_KERNEL_D = [8, 896, 1536, 3584, 4096]
NORM_FALLBACK_D = [4104, 1532]
EPS = 1e-6


def _norm_run(fn, x, res, w, douts):
    """(h, n, dx, dres, dw) of fn on fresh leaves; douts = (dh, dn), either
    may be None (that output then takes no part in the backward)."""
    x = x.detach().clone().requires_grad_()
    w = w.detach().clone().requires_grad_()
    res = None if res is None else res.detach().clone().requires_grad_()
    h, n = fn(x, res, w)
    pairs = [(o, g) for o, g in zip((h, n), douts) if g is not None]
    ins = [x, w] + ([] if res is None else [res])
    grads = torch.autograd.grad([o for o, _ in pairs], ins,
                                [g.to(o.dtype) for o, g in pairs],
                                allow_unused=True)
    dx, dw = grads[0], grads[1]
    dres = grads[2] if res is not None else None
    return h.detach(), n.detach(), dx, dres, dw, _fn_names(h, n)


def _norm_ref(x, res, w):          # fp32 from the bf16 inputs, nothing rounded
    h = x if res is None else x + res
    return h, w * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS))


def _norm_stock(x, res, w):        # torch.add + Qwen2RMSNorm.forward in bf16
    return eager.add_rms_norm(x, res, w, EPS)


def _norm_op(x, res, w):
    return ops.add_rms_norm(x, res, w, EPS)


@pytest.mark.parametrize("rows", [1, 3, 300])
@pytest.mark.parametrize("d", NORM_KERNEL_D + NORM_FALLBACK_D)
def test_add_rms_norm(d, rows):
    g = torch.Generator(device="cpu").manual_seed(d * 1009 + rows)
    x, res = _rnd(g, rows, d), _rnd(g, rows, d)
    w = (1.0 + 0.25 * torch.randn(d, generator=g)).to(torch.bfloat16) \
        .to(_dev())
    dh, dn = _rnd(g, rows, d), _rnd(g, rows, d)
    for r in (None, res):
        for douts, mode in (((None, dn), "dn"), ((dh, None), "dh"),
                            ((dh, dn), "dh+dn")):
            label = f"add_rms_norm d{d} rows{rows} res{r is not None} {mode}"
            got = _norm_run(_norm_op, x, r, w, douts)
            stock = _norm_run(_norm_stock, x, r, w, douts)
            ref = _norm_run(_norm_ref, x.float(),
                            None if r is None else r.float(), w.float(),
                            douts)
            in_graph = "_AddRMSNormFnBackward" in got[5]
            assert in_graph == (d in NORM_KERNEL_D), (label, got[5])
            # h = x + residual in one rounding: torch.add's bits
            assert torch.equal(got[0], x if r is None else x + r), label
            for name, k, s, f in zip(("n", "dx", "dres", "dw"), got[1:5],
                                     stock[1:5], ref[1:5]):
                if f is None:
                    assert k is None, (label, name)
                    continue
                _held(f"{label} {name}", k, s, f)
            if r is not None and got[2] is not None:
                # one gradient tensor serves x and the residual
                assert torch.equal(got[2], got[3]), label
            again = _norm_run(_norm_op, x, r, w, douts)
            for name, a, b in zip(("h", "n", "dx", "dres", "dw"), got[:5],
                                  again[:5]):
                assert (a is None and b is None) or torch.equal(a, b), \
                    (label, name)


def test_add_rms_norm_3d_and_noncontiguous_inputs():
    g = torch.Generator(device="cpu").manual_seed(5)
    x = _rnd(g, 2, 7, 2 * 896)[..., :896]          # a strided view
    res = _rnd(g, 2, 7, 896)
    w = _rnd(g, 896)
    h, n = ops.add_rms_norm(x, res, w, EPS)
    h2, n2 = ops.add_rms_norm(x.contiguous(), res, w, EPS)
    assert h.shape == n.shape == (2, 7, 896)
    assert torch.equal(h, h2) and torch.equal(n, n2)


# ------------------------------------------------------------------ rope_qk

def _rbf(x):
    return x.to(torch.bfloat16).float()


def rope_formula(x, cos, sin, inverse):
    """The kernel's rounding sequence written with fp32 torch ops: every
    product rounded to bf16, then the sum rounded to bf16."""
    half = x.size(-1) // 2
    xf, c, s = x.float(), cos.float().unsqueeze(1), sin.float().unsqueeze(1)
    a = _rbf(xf * c)
    if inverse:
        t = _rbf(xf * s)
        b = torch.cat((t[..., half:], -t[..., :half]), dim=-1)
    else:
        b = _rbf(torch.cat((-xf[..., half:], xf[..., :half]), dim=-1) * s)
    return (a + b).to(torch.bfloat16)


def _rope_run(fn, q, k, cos, sin, dq, dk):
    q = q.detach().requires_grad_()
    k = k.detach().requires_grad_()
    qo, ko = fn(q, k, cos, sin)
    gq, gk = torch.autograd.grad([qo, ko], [q, k],
                                 [dq.to(qo.dtype), dk.to(ko.dtype)])
    return qo.detach(), ko.detach(), gq, gk, _fn_names(qo, ko), (qo, ko)


ROPE_B = 2


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", [(4, 2), (12, 2)])
@pytest.mark.parametrize("L", [1, 5, 70])
def test_rope_qk(L, heads, D):
    from transformers.models.qwen2.modeling_qwen2 import apply_rotary_pos_emb

    B, (hq, hkv) = ROPE_B, heads
    g = torch.Generator(device="cpu").manual_seed(L * 131 + hq * 17 + D)
    # separate [B,L,H*D] projections, and q/k/v packed in one wider buffer
    q_sep = _rnd(g, B, L, hq * D).view(B, L, hq, D).transpose(1, 2)
    k_sep = _rnd(g, B, L, hkv * D).view(B, L, hkv, D).transpose(1, 2)
    packed = _rnd(g, B, L, (hq + 2 * hkv) * D)
    q_off = packed[..., hkv * D:(hkv + hq) * D].view(B, L, hq, D) \
        .transpose(1, 2)
    k_off = packed[..., :hkv * D].view(B, L, hkv, D).transpose(1, 2)
    dq = _rnd(g, B, L, hq, D).transpose(1, 2)     # as gqa_attn_bwd returns
    dk = _rnd(g, B, L, hkv, D).transpose(1, 2)
    stock_equals_formula = True
    for q, k, layout in ((q_sep, k_sep, "separate"), (q_off, k_off, "offset")):
        for cb in (B, 1):
            # random tables with unequal halves
            cos, sin = _rnd(g, cb, L, D), _rnd(g, cb, L, D)
            label = f"rope L{L} H{heads} D{D} {layout} cos[{cb}]"
            got = _rope_run(ops.rope_qk, q, k, cos, sin, dq, dk)
            assert "_RopeQKFnBackward" in got[4], (label, got[4])
            for t, h in zip(got[5], (hq, hkv)):
                assert t.shape == (B, h, L, D)
                assert t.transpose(1, 2).is_contiguous(), label
            want = (rope_formula(q, cos, sin, False),
                    rope_formula(k, cos, sin, False),
                    rope_formula(dq, cos, sin, True),
                    rope_formula(dk, cos, sin, True))
            for name, a, b in zip(("q", "k", "dq", "dk"), got[:4], want):
                assert torch.equal(a, b), (label, name)
            stock = _rope_run(apply_rotary_pos_emb, q, k, cos, sin, dq, dk)
            ref = _rope_run(eager.rope_qk, q.float(), k.float(), cos.float(),
                            sin.float(), dq.float(), dk.float())
            for name, a, s, f in zip(("q", "k", "dq", "dk"), got[:4],
                                     stock[:4], ref[:4]):
                _held(f"{label} {name}", a, s, f)
                stock_equals_formula &= torch.equal(a, s)
    print(f"rope L{L} H{heads} D{D}: stock bf16 on this GPU equals the "
          f"rounding formulas bit for bit: {stock_equals_formula}")


def test_rope_qk_fallbacks():
    g = torch.Generator(device="cpu").manual_seed(3)
    q, k = _rnd(g, 2, 4, 5, 96), _rnd(g, 2, 2, 5, 96)
    cos, sin = _rnd(g, 1, 5, 96), _rnd(g, 1, 5, 96)
    got = _rope_run(ops.rope_qk, q, k, cos, sin, q, k)
    assert "_RopeQKFnBackward" not in got[4]
    want = eager.rope_qk(q, k, cos, sin)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # fp32 tables (autocast with an fp32 residual stream): stock promotion
    q, k = _rnd(g, 2, 4, 5, 64), _rnd(g, 2, 2, 5, 64)
    cos, sin = _rnd(g, 1, 5, 64).float(), _rnd(g, 1, 5, 64).float()
    got = _rope_run(ops.rope_qk, q, k, cos, sin, q, k)
    assert "_RopeQKFnBackward" not in got[4]
    assert got[0].dtype == torch.float32


# ------------------------------------------------------------------- swiglu

def _swiglu_run(fn, gate, up, dy):
    gate = gate.detach().requires_grad_()
    up = up.detach().requires_grad_()
    y = fn(gate, up)
    dg, du = torch.autograd.grad([y], [gate, up], [dy.to(y.dtype)])
    return y.detach(), dg, du, _fn_names(y)


def _swiglu_stock(gate, up):
    return F.silu(gate) * up


@pytest.mark.parametrize("I", [8, 256, 8960])
@pytest.mark.parametrize("rows", [1, 37])
def test_swiglu(rows, I):
    g = torch.Generator(device="cpu").manual_seed(rows * 10007 + I)
    both = _rnd(g, rows, 2 * I, scale=2.0)
    dy = _rnd(g, rows, I)
    for gate, up, layout in (
            (both[:, :I].contiguous(), both[:, I:].contiguous(), "contig"),
            (both[:, :I], both[:, I:], "halves")):
        label = f"swiglu rows{rows} I{I} {layout}"
        got = _swiglu_run(ops.swiglu, gate, up, dy)
        assert "_SwiGLUFnBackward" in got[3], (label, got[3])
        stock = _swiglu_run(_swiglu_stock, gate, up, dy)
        ref = _swiglu_run(_swiglu_stock, gate.float(), up.float(), dy.float())
        for name, a, s, f in zip(("y", "dgate", "dup"), got[:3], stock[:3],
                                 ref[:3]):
            assert a.is_contiguous() and a.shape == (rows, I)
            _held(f"{label} {name}", a, s, f)


def test_swiglu_3d_and_fallback():
    g = torch.Generator(device="cpu").manual_seed(11)
    gate, up, dy = _rnd(g, 2, 5, 256), _rnd(g, 2, 5, 256), _rnd(g, 2, 5, 256)
    got = _swiglu_run(ops.swiglu, gate, up, dy)
    flat = _swiglu_run(ops.swiglu, gate.view(10, 256), up.view(10, 256),
                       dy.view(10, 256))
    assert "_SwiGLUFnBackward" in got[3]
    for a, b in zip(got[:3], flat[:3]):
        assert a.shape == (2, 5, 256) and torch.equal(a.view(10, 256), b)
    gate, up, dy = _rnd(g, 3, 100), _rnd(g, 3, 100), _rnd(g, 3, 100)
    got = _swiglu_run(ops.swiglu, gate, up, dy)
    assert "_SwiGLUFnBackward" not in got[3]
    assert torch.equal(got[0], _swiglu_stock(gate, up))


def test_swiglu_saturated_gates():
    g = torch.Generator(device="cpu").manual_seed(13)
    vals = torch.tensor([-100.0, -20.0, 0.0, 20.0, 100.0])
    gate = vals.repeat_interleave(8)[None, :].to(torch.bfloat16).to(_dev())
    up, dy = _rnd(g, 1, 40, scale=3.0), _rnd(g, 1, 40, scale=3.0)
    got = _swiglu_run(ops.swiglu, gate, up, dy)
    assert "_SwiGLUFnBackward" in got[3]
    stock = _swiglu_run(_swiglu_stock, gate, up, dy)
    ref = _swiglu_run(_swiglu_stock, gate.float(), up.float(), dy.float())
    for name, a, s, f in zip(("y", "dgate", "dup"), got[:3], stock[:3],
                             ref[:3]):
        assert torch.isfinite(a).all(), name
        assert (a[s == 0] == 0).all(), name
        _held(f"swiglu saturated {name}", a, s, f)
    # sigmoid is exactly 0 / 1 at the ends: y = 0 / up, dgate = 0 / dy*up
    assert (got[0][:, :8] == 0).all() and (got[1][:, :8] == 0).all()
    assert torch.equal(got[0][:, 32:], (gate * up)[:, 32:])
    assert torch.equal(got[1][:, 32:], (dy.float() * up.float())
                       .to(torch.bfloat16)[:, 32:])


# --------------------------------------------------------------- model level

QWEN = dict(vocab_size=512, hidden_size=512, num_layers=2, num_heads=4,
            num_kv_heads=2, intermediate_size=256)   # head_dim 128
M_L, M_PADS = 70, [66, 0, 3]
NODES = {"_AddRMSNormFnBackward": 2 * QWEN["num_layers"] + 1,
         "_RopeQKFnBackward": QWEN["num_layers"],
         "_SwiGLUFnBackward": QWEN["num_layers"]}


@functools.lru_cache(maxsize=None)
def _models():
    from genrec_amd.models.lcrec import LCRec, default_qwen_config
    from genrec_amd.modules import hf_layers

    torch.manual_seed(0)
    stock = LCRec(config=default_qwen_config(**QWEN),
                  attn_implementation="sdpa")
    stock.add_codebook_tokens(3, 8)
    stock = stock.to(_dev()).to(torch.bfloat16).eval()
    fused = copy.deepcopy(stock)
    fused.layer_implementation = "genrec_fused"
    assert hf_layers.install(fused.model) == QWEN["num_layers"]
    ref = copy.deepcopy(stock).float()      # same (bf16-rounded) weights
    torch.manual_seed(1)
    ids = torch.randint(0, 256, (len(M_PADS), M_L), device=_dev())
    attn = (torch.arange(M_L, device=_dev())[None, :]
            >= torch.tensor(M_PADS, device=_dev())[:, None]).long()
    return stock, fused, ref, ids, attn


def _train_run(m, ids, attn):
    valid = attn.bool()
    m.zero_grad()
    out = m(ids, attn, labels=ids.masked_fill(~valid, -100))
    names = _fn_names(out.loss)
    out.loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    m.zero_grad()
    return out.logits.detach()[valid], out.loss.detach(), grads, names


def test_model_loss_logits_and_grads():
    stock, fused, ref, ids, attn = _models()
    r, s, k = (_train_run(m, ids, attn) for m in (ref, stock, fused))
    for name, want in NODES.items():
        assert k[3].count(name) == want, (name, k[3].count(name))
        assert s[3].count(name) == 0          # the stock copy stays stock
    _held("model logits", k[0], s[0], r[0])
    _held("model loss", k[1], s[1], r[1])
    assert k[2].keys() == r[2].keys()
    for name in r[2]:
        _held(f"model grad {name}", k[2][name], s[2][name], r[2][name])


def test_model_gradient_checkpointing_bitwise():
    _, fused, _, ids, attn = _models()
    plain = _train_run(fused, ids, attn)
    ckpt = copy.deepcopy(fused)
    ckpt.gradient_checkpointing_enable()
    ckpt.train()
    got = _train_run(ckpt, ids, attn)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    for name in plain[2]:
        assert torch.equal(got[2][name], plain[2][name]), name


def _prefill_and_decode(m, ids, attn, steps):
    """Logits of the last prompt position and of `steps` cached single-token
    steps, with left padding and batch-dependent position ids."""
    from transformers import DynamicCache

    cache = DynamicCache()
    outs = []
    with torch.no_grad():
        pos = (attn.cumsum(-1) - 1).clamp(min=0)
        out = m.model(input_ids=ids, attention_mask=attn, position_ids=pos,
                      past_key_values=cache, use_cache=True)
        outs.append(out.logits[:, -1].float())
        for tok in steps:
            attn = torch.cat([attn, torch.ones_like(attn[:, :1])], dim=1)
            pos = pos[:, -1:] + 1
            out = m.model(input_ids=tok, attention_mask=attn,
                          position_ids=pos, past_key_values=cache,
                          use_cache=True)
            outs.append(out.logits[:, -1].float())
    return outs


def test_model_prefill_and_cached_decode():
    stock, fused, ref, ids, attn = _models()
    torch.manual_seed(2)
    steps = [torch.randint(0, 256, (len(M_PADS), 1), device=_dev())
             for _ in range(2)]
    r, s, k = (_prefill_and_decode(m, ids, attn, steps)
               for m in (ref, stock, fused))
    for i, what in enumerate(("prefill", "decode 1", "decode 2")):
        _held(f"model {what} logits", k[i], s[i], r[i])


@pytest.mark.parametrize("beam_cache", [None, "shared_prefix"])
def test_model_generate_topk(beam_cache):
    from genrec_amd.modules import hf_attention  # noqa: F401  (registers)

    _, fused, _, ids, attn = _models()
    m = copy.deepcopy(fused)
    m.model.set_attn_implementation("genrec_gqa")
    m.attn_implementation = "genrec_gqa"
    cb = m.codebook_token_ids(3, 8)
    res = m.generate_topk(ids, attention_mask=attn, max_new_tokens=3,
                          beam_width=4, beam_cache=beam_cache,
                          allowed_token_ids=[cb[0], cb[1], cb[2]])
    assert len(res) == len(M_PADS) and all(len(r) == 4 for r in res)
    for row in res:
        scores = [s for _, s in row]
        assert all(math.isfinite(s) for s in scores)
        assert scores == sorted(scores, reverse=True)
        for seq, _ in row:
            new = seq[M_L:].tolist()
            assert len(new) == 3
            for step in range(3):
                assert new[step] in cb[step].tolist()
