"""Grouped-query attention: eager reference, the "genrec_gqa" transformers
hook and the LCRec `attn_implementation` switch (CPU, fp32)."""

import copy

import pytest
import torch
import torch.nn.functional as F

from genrec_amd.models.lcrec import LCRec, default_qwen_config
from genrec_amd.ops import eager

TINY = dict(vocab_size=512, hidden_size=64, num_layers=2, num_heads=4,
            num_kv_heads=2, intermediate_size=128)


def _sdpa_expanded(q, k, v, key_pad, scale):
    """F.scaled_dot_product_attention on repeat_interleave-expanded K/V with
    the explicit causal-offset AND key-valid mask -> ([B,Lq,Hq,D], any_vis)."""
    B, Hq, Lq, D = q.shape
    Hkv, Lk = k.size(1), k.size(2)
    g = Hq // Hkv
    ke, ve = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    i = torch.arange(Lq)[:, None] + (Lk - Lq)
    j = torch.arange(Lk)[None, :]
    vis = (j <= i)[None, None].expand(B, 1, Lq, Lk)
    if key_pad is not None:
        vis = vis & ~key_pad[:, None, None, :]
    # sdpa rows with no visible key are not compared: give them one key
    any_vis = vis.any(-1)                                   # [B,1,Lq]
    safe = vis | ~any_vis[..., None]
    out = F.scaled_dot_product_attention(q, ke, ve, attn_mask=safe,
                                         scale=scale)
    return out.transpose(1, 2), any_vis[:, 0]               # [B,Lq]


@pytest.mark.parametrize("heads", [(4, 2), (6, 1), (2, 2)])
@pytest.mark.parametrize("lq,lk", [(9, 9), (1, 10), (3, 10)])
@pytest.mark.parametrize("pads", [None, (4, 0, 1), (10, 2, 0)])
def test_eager_gqa_matches_sdpa(heads, lq, lk, pads):
    torch.manual_seed(0)
    hq, hkv = heads
    B, D = 3, 16
    q = torch.randn(B, hq, lq, D)
    k = torch.randn(B, hkv, lk, D)
    v = torch.randn(B, hkv, lk, D)
    key_pad = None
    if pads is not None:  # left padding
        key_pad = torch.arange(lk)[None, :] < torch.tensor(pads)[:, None]
    scale = D ** -0.5
    got = eager.gqa_attention(q, k, v, key_pad_mask=key_pad, scale=scale,
                              causal=True)
    assert got.shape == (B, lq, hq, D) and got.is_contiguous()
    ref, any_vis = _sdpa_expanded(q, k, v, key_pad, scale)
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got[any_vis], ref[any_vis], atol=1e-5, rtol=0)
    # rows with no visible key are exactly 0
    assert (got[~any_vis] == 0).all()
    if pads == (10, 2, 0) and lk == 10:
        assert (~any_vis).any()


def test_eager_gqa_empty_rows_have_zero_grad():
    torch.manual_seed(0)
    q = torch.randn(2, 4, 5, 8, requires_grad=True)
    k = torch.randn(2, 2, 5, 8, requires_grad=True)
    v = torch.randn(2, 2, 5, 8, requires_grad=True)
    key_pad = torch.arange(5)[None, :] < torch.tensor([3, 0])[:, None]
    out = eager.gqa_attention(q, k, v, key_pad_mask=key_pad, scale=0.3)
    out.sum().backward()
    for t in (q, k, v):
        assert torch.isfinite(t.grad).all()
    assert (q.grad[0, :, :3] == 0).all()      # fully-masked query rows
    assert (k.grad[0, :, :3] == 0).all() and (v.grad[0, :, :3] == 0).all()


# --------------------------------------------------------------- model level

PADS, L = [4, 0, 1], 9


def _left_padded_batch(vocab):
    torch.manual_seed(1)
    ids = torch.randint(0, vocab, (len(PADS), L))
    attn = (torch.arange(L)[None, :] >= torch.tensor(PADS)[:, None]).long()
    return ids, attn


@pytest.fixture(scope="module")
def model_pair():
    torch.manual_seed(0)
    base = LCRec(config=default_qwen_config(**TINY))
    base.add_codebook_tokens(3, 8)
    from genrec_amd.modules import hf_attention  # noqa: F401  (registers)

    gqa = copy.deepcopy(base)
    gqa.model.set_attn_implementation("genrec_gqa")
    assert base.model.config._attn_implementation != "genrec_gqa"
    return base.eval(), gqa.eval()


def test_lcrec_constructs_with_genrec_gqa():
    m = LCRec(config=default_qwen_config(**TINY),
              attn_implementation="genrec_gqa")
    assert m.model.config._attn_implementation == "genrec_gqa"
    assert m.attn_implementation == "genrec_gqa"
    # None keeps the transformers default
    d = LCRec(config=default_qwen_config(**TINY))
    assert d.model.config._attn_implementation != "genrec_gqa"


def test_load_pretrained_keeps_the_implementation(tmp_path):
    m = LCRec(config=default_qwen_config(**TINY),
              attn_implementation="genrec_gqa")
    m.save_pretrained(str(tmp_path / "ck"))
    m.load_pretrained(str(tmp_path / "ck"))
    assert m.model.config._attn_implementation == "genrec_gqa"
    d = LCRec(config=default_qwen_config(**TINY))
    d.load_pretrained(str(tmp_path / "ck"))
    assert d.model.config._attn_implementation != "genrec_gqa"


def test_notellm_constructs_with_genrec_gqa():
    from genrec_amd.models.notellm import Query2Embedding

    m = Query2Embedding(config=default_qwen_config(**TINY),
                        gradient_checkpointing=False,
                        attn_implementation="genrec_gqa")
    assert m.model.config._attn_implementation == "genrec_gqa"


def test_genrec_gqa_prefill_decode_and_grads_match_default(model_pair):
    from transformers import DynamicCache

    base, gqa = model_pair
    assert gqa.model.config._attn_implementation == "genrec_gqa"
    ids, attn = _left_padded_batch(256)
    valid = attn.bool()

    outs = []
    for m in (base, gqa):
        m.zero_grad()
        labels = ids.masked_fill(~valid, -100)
        out = m(ids, attn, labels=labels)
        out.loss.backward()
        grads = {n: p.grad.clone() for n, p in m.named_parameters()
                 if p.grad is not None}
        with torch.no_grad():
            cache = DynamicCache()
            pre = m.model(input_ids=ids, attention_mask=attn,
                          past_key_values=cache, use_cache=True)
            nxt = pre.logits[:, -1].argmax(-1, keepdim=True)
            attn2 = torch.cat([attn, torch.ones(len(PADS), 1,
                                                dtype=attn.dtype)], 1)
            dec = m.model(input_ids=nxt, attention_mask=attn2,
                          past_key_values=cache, use_cache=True)
        outs.append((out.logits.detach(), out.loss.detach(), grads,
                     pre.logits, nxt, dec.logits))

    (lg0, loss0, g0, pre0, nxt0, dec0), (lg1, loss1, g1, pre1, nxt1, dec1) = outs
    torch.testing.assert_close(lg1[valid], lg0[valid], atol=1e-5, rtol=0)
    torch.testing.assert_close(pre1[valid], pre0[valid], atol=1e-5, rtol=0)
    assert torch.equal(nxt0, nxt1)
    torch.testing.assert_close(dec1, dec0, atol=1e-5, rtol=0)
    torch.testing.assert_close(loss1, loss0, atol=1e-5, rtol=0)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for n in g0:
        assert torch.isfinite(g1[n]).all(), n
        torch.testing.assert_close(g1[n], g0[n], atol=1e-5, rtol=0, msg=n)


def _count_op_calls(monkeypatch):
    from genrec_amd.modules import hf_attention

    calls = []
    real = hf_attention.gqa_flash_attention

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(hf_attention, "gqa_flash_attention", counted)
    return calls


def test_genrec_gqa_routes_through_the_op(model_pair, monkeypatch):
    base, gqa = model_pair
    calls = _count_op_calls(monkeypatch)
    ids, attn = _left_padded_batch(256)
    with torch.no_grad():
        base(ids, attn)
        assert len(calls) == 0
        gqa(ids, attn)
        assert len(calls) == TINY["num_layers"]
        gqa(ids)                                # mask None -> pure causal
        assert len(calls) == 2 * TINY["num_layers"]


def test_generate_topk_same_beams(model_pair):
    base, gqa = model_pair
    cb = base.codebook_token_ids(3, 8)
    torch.manual_seed(0)
    prompt = torch.randint(0, 256, (2, 6))
    res = [m.generate_topk(prompt, max_new_tokens=3, beam_width=4,
                           allowed_token_ids=[cb[0], cb[1], cb[2]])
           for m in (base, gqa)]
    assert len(res[1]) == 2 and len(res[1][0]) == 4
    for b in range(2):
        for (s0, sc0), (s1, sc1) in zip(res[0][b], res[1][b]):
            assert torch.equal(s0, s1)
            assert abs(sc0 - sc1) < 1e-4


def test_adapter_falls_back_without_raising(monkeypatch):
    calls = _count_op_calls(monkeypatch)
    torch.manual_seed(0)
    cfg = default_qwen_config(**TINY)
    cfg.attention_dropout = 0.1
    m = LCRec(config=cfg, attn_implementation="genrec_gqa")
    ids, attn = _left_padded_batch(256)
    m.train()                                  # dropout > 0 while training
    out = m(ids, attn, labels=ids)
    assert torch.isfinite(out.loss)
    out.loss.backward()
    m.eval()
    with torch.no_grad():                      # output_attentions requested
        out = m.model(input_ids=ids, attention_mask=attn,
                      output_attentions=True)
    assert torch.isfinite(out.logits[attn.bool()]).all()
    assert len(calls) == 0                     # both went to stock sdpa


def test_adapter_key_pad_from_float_and_bool_masks():
    from genrec_amd.modules.hf_attention import _key_pad_from_mask

    B, lq, lk = 2, 3, 5
    key_valid = torch.tensor([[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]]).bool()
    i = torch.arange(lq)[:, None] + (lk - lq)
    causal = torch.arange(lk)[None, :] <= i
    mask = (causal[None, None] & key_valid[:, None, None, :])
    want = ~key_valid
    assert torch.equal(_key_pad_from_mask(mask, B, lq, lk), want)
    fmask = torch.zeros(B, 1, lq, lk).masked_fill(
        ~mask, torch.finfo(torch.float32).min)
    assert torch.equal(_key_pad_from_mask(fmask, B, lq, lk), want)
    assert _key_pad_from_mask(mask[:, :, :2], B, lq, lk) is None
