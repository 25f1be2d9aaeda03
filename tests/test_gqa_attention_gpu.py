"""Grouped-query flash attention kernels (csrc/kernels/attention_gqa.hip)
against the fp32 eager reference, on the GPU.

Tolerance rule (per case, for out, dq, dk and dv): both the kernel and
PyTorch's own bf16 SDPA (math backend, expanded K/V) are diffed against
`eager.gqa_attention` in fp32 on the same bf16-rounded inputs, and

    max|kernel - ref| <= 2 * max|sdpa_bf16 - ref| + ulp_bf16(max|ref|)

The 2x margin allows for a different accumulation order and for P being
rounded to bf16 before the PV MFMA. Only query rows with a visible key are
compared; rows with none must be exactly 0 (outputs and dq).
"""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

from genrec_amd import ops
from genrec_amd.ops import eager

pytestmark = pytest.mark.gpu

B = 2
HEADS = [(4, 2), (6, 1), (2, 2)]
DIMS = [64, 128]


def _dev():
    return torch.device("cuda:0")


def _ulp_bf16(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _key_pad(lk, pads, side):
    if pads is None:
        return None
    n = torch.tensor(pads, device=_dev())[:, None]
    j = torch.arange(lk, device=_dev())[None, :]
    return (j < n) if side == "left" else (j >= lk - n)


def _visible(lq, lk, key_pad):
    i = torch.arange(lq, device=_dev())[:, None] + (lk - lq)
    j = torch.arange(lk, device=_dev())[None, :]
    vis = (j <= i)[None].expand(B, lq, lk)
    if key_pad is not None:
        vis = vis & ~key_pad[:, None, :]
    return vis                                              # [B,Lq,Lk]


@functools.lru_cache(maxsize=None)
def _case(D, hq, hkv, lq, lk, pads=None, side="left"):
    """Inputs, fp32 reference and bf16-SDPA baseline of one case, computed
    once and shared (never modified) by the tests that need them."""
    g = torch.Generator(device="cpu").manual_seed(
        D * 1000003 + hq * 10007 + hkv * 101 + lq * 7 + lk)
    dev = _dev()

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)

    # [B,L,H,D] storage: what the q/k/v projections produce
    q_s, k_s, v_s = rnd(B, lq, hq, D), rnd(B, lk, hkv, D), rnd(B, lk, hkv, D)
    dout = rnd(B, lq, hq, D)
    key_pad = _key_pad(lk, pads, side)
    scale = D ** -0.5
    vis = _visible(lq, lk, key_pad)
    row_ok = vis.any(-1)                                    # [B,Lq]

    # fp32 reference on the bf16-rounded inputs
    qf, kf, vf = (t.float().transpose(1, 2).detach().requires_grad_()
                  for t in (q_s, k_s, v_s))
    ref = eager.gqa_attention(qf, kf, vf, key_pad_mask=key_pad, scale=scale,
                              causal=True)
    ref.backward(dout.float())
    ref_t = (ref.detach(), qf.grad, kf.grad, vf.grad)

    # PyTorch bf16 SDPA, math backend, expanded K/V, same mask; rows with
    # no visible key get every key (not compared) and a zero upstream grad
    from torch.nn.attention import SDPBackend, sdpa_kernel

    qb, kb, vb = (t.transpose(1, 2).detach().requires_grad_()
                  for t in (q_s, k_s, v_s))
    rep = hq // hkv
    safe = (vis | ~row_ok[..., None])[:, None]              # [B,1,Lq,Lk]
    with sdpa_kernel(SDPBackend.MATH):
        base = F.scaled_dot_product_attention(
            qb, kb.repeat_interleave(rep, 1), vb.repeat_interleave(rep, 1),
            attn_mask=safe, scale=scale)
    base = base.transpose(1, 2)                             # [B,Lq,Hq,D]
    base.backward(dout * row_ok[:, :, None, None])
    base_t = (base.detach(), qb.grad, kb.grad, vb.grad)
    return dict(q_s=q_s, k_s=k_s, v_s=v_s, dout=dout, key_pad=key_pad,
                scale=scale, row_ok=row_ok, ref=ref_t, base=base_t)


def _run_kernel(c, contiguous=False):
    q, k, v = (t.transpose(1, 2) for t in (c["q_s"], c["k_s"], c["v_s"]))
    if contiguous:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
    out = ops.gqa_flash_attention(q, k, v, key_pad_mask=c["key_pad"],
                                  scale=c["scale"], causal=True)
    assert type(out.grad_fn).__name__ == "_GqaFlashAttnFnBackward"
    out.backward(c["dout"])
    return out.detach(), q.grad, k.grad, v.grad


def _check(c, got, label):
    row_ok = c["row_ok"]
    names = ("out", "dq", "dk", "dv")
    lq, hq = c["q_s"].size(1), c["q_s"].size(2)
    assert got[0].shape == (B, lq, hq, c["q_s"].size(3))
    assert got[0].is_contiguous()
    for name, x, ref, base in zip(names, got, c["ref"], c["base"]):
        assert x.shape == ref.shape, name
        assert torch.isfinite(x).all(), f"{label} {name} not finite"
        xf, bf = x.float(), base.float()
        if name == "out":                # [B,Lq,Hq,D]
            sel = row_ok
            assert (xf[~row_ok] == 0).all(), f"{label} out at empty rows"
            xf, rf, bf = xf[sel], ref[sel], bf[sel]
        elif name == "dq":               # [B,Hq,Lq,D]
            sel = row_ok[:, None, :].expand(-1, hq, -1)
            assert (xf[~sel] == 0).all(), f"{label} dq at empty rows"
            xf, rf, bf = xf[sel], ref[sel], bf[sel]
        else:
            rf = ref
        err_k = (xf - rf).abs().max().item()
        err_b = (bf - rf).abs().max().item()
        bound = 2 * err_b + _ulp_bf16(rf.abs().max().item())
        print(f"{label} {name}: kernel {err_k:.3e} sdpa_bf16 {err_b:.3e} "
              f"bound {bound:.3e}")
        assert err_k <= bound, (label, name, err_k, err_b, bound)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("L", [63, 64, 65, 130])
def test_prefill(D, heads, L):
    c = _case(D, *heads, L, L)
    _check(c, _run_kernel(c), f"prefill D{D} H{heads} L{L}")


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("lq,lk", [(1, 70), (1, 64), (5, 133), (1, 1)])
def test_decode_and_chunk(D, heads, lq, lk):
    c = _case(D, *heads, lq, lk)
    _check(c, _run_kernel(c), f"decode D{D} H{heads} {lq}x{lk}")


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("L,pads,side", [
    (130, (70, 0), "left"),    # a whole leading K tile masked for valid rows
    (65, (3, 64), "left"),
    (65, (0, 5), "right"),
])
def test_padding(D, L, pads, side):
    c = _case(D, 4, 2, L, L, pads, side)
    got = _run_kernel(c)
    _check(c, got, f"pad D{D} L{L} {side}{pads}")
    # padded keys receive exactly zero gradient
    kp = c["key_pad"][:, None, :, None].expand_as(got[2])
    assert (got[2][kp] == 0).all() and (got[3][kp] == 0).all()
    if side == "left":
        assert (~c["row_ok"]).any()


def test_lse_matches_reference_and_is_finite():
    c = _case(128, 4, 2, 130, 130, (70, 0), "left")
    q, k, v = (t.transpose(1, 2) for t in (c["q_s"], c["k_s"], c["v_s"]))
    out, lse = ops.ext().gqa_attn_fwd(q, k, v, c["key_pad"], c["scale"], True)
    assert lse.shape == (B, 4, 130) and lse.dtype == torch.float32
    assert torch.isfinite(lse).all()
    s = torch.einsum("bqhd,bkhd->bhqk", c["q_s"].float(),
                     c["k_s"].float().repeat_interleave(2, 2)) * c["scale"]
    vis = _visible(130, 130, c["key_pad"])[:, None]
    ref = torch.logsumexp(s.masked_fill(~vis, float("-inf")), -1)
    ok = c["row_ok"][:, None, :].expand(-1, 4, -1)
    torch.testing.assert_close(lse[ok], ref[ok], atol=1e-3, rtol=1e-4)
    assert (lse[~ok] == 0).all()


@pytest.mark.parametrize("D", DIMS)
def test_layouts_bitwise_equal(D):
    c = _case(D, 4, 2, 130, 130, (70, 0), "left")
    a = _run_kernel(c, contiguous=False)   # [B,L,H,D].transpose(1,2) views
    b = _run_kernel(c, contiguous=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[0].shape == (B, 130, 4, D) and a[0].is_contiguous()
    # grads come back as transpose views of [B,L,H,D] storage
    for gname, gt in zip(("dq", "dk", "dv"), a[1:]):
        assert gt.transpose(1, 2).is_contiguous(), gname


def test_contiguous_kv_cache_decode_no_copy_layout():
    # decode against a contiguous [B,Hkv,Lk,D] cache, q from a projection
    c = _case(128, 6, 1, 1, 70)
    got = _run_kernel(c, contiguous=True)
    _check(c, got, "decode cache-layout")


def test_determinism():
    c = _case(128, 6, 1, 130, 130)
    q, k, v = (t.transpose(1, 2) for t in (c["q_s"], c["k_s"], c["v_s"]))
    runs = []
    for _ in range(2):
        out, lse = ops.ext().gqa_attn_fwd(q, k, v, None, c["scale"], True)
        dq, dk, dv = ops.ext().gqa_attn_bwd(c["dout"], q, k, v, out, lse,
                                            None, c["scale"], True)
        runs.append((out, lse, dq, dk, dv))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_dispatch_proof(monkeypatch):
    c = _case(64, 4, 2, 65, 65)
    q, k, v = (t.transpose(1, 2).detach().requires_grad_()
               for t in (c["q_s"], c["k_s"], c["v_s"]))
    out = ops.gqa_flash_attention(q, k, v, scale=c["scale"])
    assert type(out.grad_fn).__name__ == "_GqaFlashAttnFnBackward"
    monkeypatch.setenv("GENREC_DISABLE_ATTN_GQA", "1")
    out2 = ops.gqa_flash_attention(q, k, v, scale=c["scale"])
    assert "GqaFlash" not in type(out2.grad_fn).__name__
    assert out2.shape == out.shape
    monkeypatch.delenv("GENREC_DISABLE_ATTN_GQA")
    # unsupported shapes never reach the host wrapper from the op layer...
    q32 = torch.randn(B, 4, 8, 32, device=_dev(), dtype=torch.bfloat16,
                      requires_grad=True)
    k32 = torch.randn(B, 2, 8, 32, device=_dev(), dtype=torch.bfloat16)
    out3 = ops.gqa_flash_attention(q32, k32, k32, scale=1.0)
    assert "GqaFlash" not in type(out3.grad_fn).__name__
    # ...and the wrapper itself rejects them with a message
    with pytest.raises(RuntimeError, match="head dim"):
        ops.ext().gqa_attn_fwd(q32, k32, k32, None, 1.0, True)
    with pytest.raises(RuntimeError, match="multiple of Hkv"):
        ops.ext().gqa_attn_fwd(q[:, :3], k, v, None, 1.0, True)


def test_op_is_capture_safe():
    c = _case(128, 4, 2, 130, 130, (70, 0), "left")
    q, k, v = (t.transpose(1, 2) for t in (c["q_s"], c["k_s"], c["v_s"]))

    def fwd():
        return ops.gqa_flash_attention(q, k, v, key_pad_mask=c["key_pad"],
                                       scale=c["scale"])

    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            eager_out = fwd()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = fwd()
        graph.replay()
        first = static_out.clone()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(first, static_out) and torch.equal(first, eager_out)


# --------------------------------------------------------------- model level

QWEN = dict(vocab_size=512, hidden_size=512, num_layers=2, num_heads=4,
            num_kv_heads=2, intermediate_size=256)   # head_dim 128
M_L, M_PADS = 70, [66, 0, 3]


@functools.lru_cache(maxsize=None)
def _models():
    import copy

    from genrec_amd.models.lcrec import LCRec, default_qwen_config
    from genrec_amd.modules import hf_attention  # noqa: F401  (registers)

    torch.manual_seed(0)
    sdpa = LCRec(config=default_qwen_config(**QWEN),
                 attn_implementation="sdpa")
    sdpa.add_codebook_tokens(3, 8)
    sdpa = sdpa.to(_dev()).to(torch.bfloat16).eval()
    gqa = copy.deepcopy(sdpa)
    gqa.model.set_attn_implementation("genrec_gqa")
    ref = copy.deepcopy(sdpa).float()       # same (bf16-rounded) weights
    torch.manual_seed(1)
    ids = torch.randint(0, 256, (len(M_PADS), M_L), device=_dev())
    attn = (torch.arange(M_L, device=_dev())[None, :]
            >= torch.tensor(M_PADS, device=_dev())[:, None]).long()
    return sdpa, gqa, ref, ids, attn


def test_model_logits_loss_and_grads():
    sdpa, gqa, ref, ids, attn = _models()
    valid = attn.bool()
    labels = ids.masked_fill(~valid, -100)
    res = {}
    for name, m in (("ref", ref), ("sdpa", sdpa), ("gqa", gqa)):
        m.zero_grad()
        out = m(ids, attn, labels=labels)
        out.loss.backward()
        res[name] = (out.logits.detach().float()[valid],
                     out.loss.detach().float())
        if name == "gqa":
            grads = [p.grad for p in m.parameters() if p.grad is not None]
            assert grads and all(torch.isfinite(g).all() for g in grads)
            fns = set()
            stack = [out.loss.grad_fn]
            while stack:                      # the kernel is in the graph
                fn = stack.pop()
                if fn is None or fn in fns:
                    continue
                fns.add(fn)
                stack.extend(f for f, _ in fn.next_functions)
            assert sum(type(f).__name__ == "_GqaFlashAttnFnBackward"
                       for f in fns) == QWEN["num_layers"]
        m.zero_grad()
    for idx, what in ((0, "logits"), (1, "loss")):
        r = res["ref"][idx]
        err_k = (res["gqa"][idx] - r).abs().max().item()
        err_b = (res["sdpa"][idx] - r).abs().max().item()
        bound = 2 * err_b + _ulp_bf16(r.abs().max().item())
        print(f"model {what}: genrec_gqa {err_k:.3e} sdpa_bf16 {err_b:.3e} "
              f"bound {bound:.3e}")
        assert math.isfinite(err_k) and err_k <= bound, (what, err_k, bound)


def test_model_generate_topk_constrained():
    _, gqa, _, ids, attn = _models()
    cb = gqa.codebook_token_ids(3, 8)
    res = gqa.generate_topk(ids, attention_mask=attn, max_new_tokens=3,
                            beam_width=4,
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


def test_model_forward_captured_graph():
    _, gqa, _, ids, _ = _models()
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            eager_logits = gqa.model(input_ids=ids, use_cache=False).logits
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_logits = gqa.model(input_ids=ids, use_cache=False).logits
        graph.replay()
        first = static_logits.clone()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.isfinite(first).all()
    assert torch.equal(first, static_logits)
    torch.testing.assert_close(first.float(), eager_logits.float(),
                               atol=0.05, rtol=0.05)
