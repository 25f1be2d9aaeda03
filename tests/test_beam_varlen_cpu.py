"""Padding-free generation on the CPU: the packed-prefix eager op against
the padded one, SharedPrefixBeamCache.from_packed_prefill's bookkeeping and
LCRec.generate_topk(prefill="packed") against the left-padded prefill."""

import functools

import pytest
import torch

from genrec_amd.modules.hf_attention import SharedPrefixBeamCache
from genrec_amd.ops import eager

HQ, HKV, D, W, T = 4, 2, 16, 3, 4
LENS = [1, 64, 65, 130, 7]


def _packed_state(lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, Ttot = len(lens), sum(lens)
    q = torch.randn(B * W, HQ, 1, D, generator=g)
    k_pre, v_pre = (torch.randn(Ttot, HKV, D, generator=g) for _ in range(2))
    k_suf, v_suf = (torch.randn(B, T, W, HKV, D, generator=g)
                    for _ in range(2))
    anc = torch.randint(0, W, (B, W, T), generator=g, dtype=torch.int32)
    anc[:, 1] = anc[:, 0]              # two beams inherit the same slots
    cu = torch.tensor([0] + lens).cumsum(0).to(torch.int32)
    return q, k_pre, v_pre, cu, k_suf, v_suf, anc


def _left_padded(k_pre, v_pre, lens):
    """[B,Hkv,Lp,D] K/V with prompt b's tokens at the right end, NaN in the
    pads, and the [B,Lp] pad mask."""
    B, lp = len(lens), max(max(lens), 1)
    k = torch.full((B, HKV, lp, D), float("nan"))
    v = torch.full((B, HKV, lp, D), float("nan"))
    pad = torch.ones(B, lp, dtype=torch.bool)
    s = 0
    for b, n in enumerate(lens):
        if n:
            k[b, :, lp - n:] = k_pre[s:s + n].transpose(0, 1)
            v[b, :, lp - n:] = v_pre[s:s + n].transpose(0, 1)
            pad[b, lp - n:] = False
        s += n
    # the padded eager op multiplies masked probabilities (exact 0) with the
    # pad values: keep those finite
    return k.nan_to_num(0.0), v.nan_to_num(0.0), pad


@pytest.mark.parametrize("t", [1, 4])
def test_eager_varlen_equals_padded(t):
    q, k_pre, v_pre, cu, k_suf, v_suf, anc = _packed_state(LENS, seed=t)
    got = eager.beam_decode_varlen_attention(
        q, k_pre, v_pre, cu, max(LENS), k_suf, v_suf, anc, t, scale=D ** -0.5)
    assert got.shape == (len(LENS) * W, 1, HQ, D)
    k, v, pad = _left_padded(k_pre, v_pre, LENS)
    want = eager.beam_decode_attention(q, k, v, k_suf, v_suf, anc, t,
                                       pre_pad=pad, scale=D ** -0.5)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("t", [1, 4])
def test_eager_varlen_zero_length_prompt_is_suffix_softmax(t):
    lens = [5, 0, 3]
    q, k_pre, v_pre, cu, k_suf, v_suf, anc = _packed_state(lens, seed=7)
    scale = D ** -0.5
    got = eager.beam_decode_varlen_attention(
        q, k_pre, v_pre, cu, 5, k_suf, v_suf, anc, t, scale=scale)
    assert torch.isfinite(got).all()
    g = HQ // HKV
    for w in range(W):
        ks = torch.stack([k_suf[1, s, int(anc[1, w, s])] for s in range(t)])
        vs = torch.stack([v_suf[1, s, int(anc[1, w, s])] for s in range(t)])
        for h in range(HQ):
            p = torch.softmax(ks[:, h // g] @ q[W + w, h, 0] * scale, dim=0)
            want = p @ vs[:, h // g]
            assert torch.allclose(got[W + w, 0, h], want, rtol=1e-5,
                                  atol=1e-5)
    # the other prompts are what they are without the empty one
    keep = [0, 2]
    rows = torch.cat([torch.arange(b * W, (b + 1) * W) for b in keep])
    alone = eager.beam_decode_varlen_attention(
        q[rows], k_pre, v_pre, torch.tensor([0, 5, 8], dtype=torch.int32), 5,
        k_suf[keep], v_suf[keep], anc[keep], t, scale=scale)
    assert torch.allclose(got[rows], alone, rtol=1e-6, atol=1e-6)


def test_eager_varlen_clamps_offsets():
    lens = [4, 6]
    q, k_pre, v_pre, _, k_suf, v_suf, anc = _packed_state(lens, seed=9)
    # prompt 0 runs past the tensor, prompt 1 ends before it starts
    wild = torch.tensor([3, 99, 2], dtype=torch.int32)
    clamped = torch.tensor([3, 10, 10], dtype=torch.int32)
    a = eager.beam_decode_varlen_attention(
        q, k_pre, v_pre, wild, 10, k_suf, v_suf, anc, 2, scale=0.25)
    b = eager.beam_decode_varlen_attention(
        q, k_pre, v_pre, clamped, 10, k_suf, v_suf, anc, 2, scale=0.25)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_from_packed_prefill_bookkeeping_equals_rectangular():
    from transformers import DynamicCache

    g = torch.Generator().manual_seed(3)
    lens, layers, lp = [3, 5], 2, 5
    B, Ttot = len(lens), sum(lens)
    cu = torch.tensor([0, 3, 8], dtype=torch.int32)
    packed_cache = DynamicCache()
    rect_k, rect_v = [], []
    for i in range(layers):
        k = torch.randn(1, HKV, Ttot, D, generator=g)
        v = torch.randn(1, HKV, Ttot, D, generator=g)
        packed_cache.update(k, v, i)
        rect_k.append(torch.zeros(B, HKV, lp, D))
        rect_v.append(torch.zeros(B, HKV, lp, D))
    packed = SharedPrefixBeamCache.from_packed_prefill(packed_cache, cu, lp,
                                                       W, T)
    rect = SharedPrefixBeamCache(rect_k, rect_v, W, T)
    assert packed.packed and not rect.packed
    assert packed.max_prefix == lp and torch.equal(packed.cu_seqlens, cu)
    assert packed.cu_seqlens.dtype == torch.int32
    for i in range(layers):
        # [Ttot,Hkv,D] views of the prefill's tensors, not copies
        assert packed.k_pre[i].shape == (Ttot, HKV, D)
        assert packed.k_pre[i].data_ptr() \
            == packed_cache.layers[i].keys.data_ptr()
        assert torch.equal(packed.v_pre[i],
                           packed_cache.layers[i].values[0].transpose(0, 1))
    assert packed.get_seq_length() == lp
    for step, parents in enumerate([[[0, 0, 1], [2, 1, 0]],
                                    [[1, 2, 2], [0, 0, 1]]]):
        for i in range(layers):
            k = torch.randn(B * W, HKV, 1, D, generator=g)
            v = torch.randn(B * W, HKV, 1, D, generator=g)
            packed.update(k, v, i)
            rect.update(k, v, i)
        parent = torch.tensor(parents)
        packed.advance(parent)
        rect.advance(parent)
        assert packed.t == rect.t == step + 1
        assert packed.get_seq_length() == lp + step + 1
        assert torch.equal(packed.anc, rect.anc)
        for i in range(layers):
            assert torch.equal(packed.k_suf[i], rect.k_suf[i])
            assert torch.equal(packed.v_suf[i], rect.v_suf[i])
    with pytest.raises(ValueError, match="packed prefix"):
        SharedPrefixBeamCache(packed.k_pre, packed.v_pre, W, T,
                              pre_pad=torch.zeros(B, lp, dtype=torch.bool),
                              cu_seqlens=cu, max_prefix=lp)


# ------------------------------------------------------------- model level

N_NEW, M_W = 4, 4
M_L, M_PADS = 70, [66, 0, 3]
SCORE_TOL = 1e-4   # fp32; the two prefills differ by the absolute positions


@functools.lru_cache(maxsize=None)
def _lcrec(attn_implementation="genrec_gqa"):
    from genrec_amd.models.lcrec import LCRec, default_qwen_config

    torch.manual_seed(0)
    m = LCRec(config=default_qwen_config(
        vocab_size=512, hidden_size=256, num_layers=2, num_heads=4,
        num_kv_heads=2, intermediate_size=256),
        attn_implementation=attn_implementation)
    m.add_codebook_tokens(N_NEW, 8)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.normal_(0, 0.25 if "embed_tokens" in name else 0.05)
    ids = torch.randint(0, 256, (len(M_PADS), M_L),
                        generator=torch.Generator().manual_seed(1))
    attn = (torch.arange(M_L)[None, :]
            >= torch.tensor(M_PADS)[:, None]).long()
    return m.float().eval(), ids, attn


def test_generate_topk_packed_matches_padded(monkeypatch):
    m, ids, attn = _lcrec()
    allowed = list(m.codebook_token_ids(N_NEW, 8))
    kw = dict(attention_mask=attn, max_new_tokens=N_NEW, beam_width=M_W,
              allowed_token_ids=allowed, beam_cache="shared_prefix")
    base = m.generate_topk(ids, **kw)

    fed = []
    forward = m.model.forward

    def spy(*args, **kwargs):
        fed.append(tuple(kwargs["input_ids"].shape))
        return forward(*args, **kwargs)

    monkeypatch.setattr(m.model, "forward", spy)
    new = m.generate_topk(ids, prefill="packed", **kw)
    # one packed row of the real tokens, then the decode steps
    assert fed[0] == (1, int(attn.sum()))
    assert fed[1:] == [(len(M_PADS) * M_W, 1)] * (N_NEW - 1)

    assert len(new) == len(base) == len(M_PADS)
    worst = 0.0
    for b, (row_a, row_b) in enumerate(zip(base, new)):
        assert len(row_a) == len(row_b) == M_W
        sc_a = sorted((s for _, s in row_a), reverse=True)
        sc_b = [s for _, s in row_b]
        assert sc_b == sorted(sc_b, reverse=True)
        for (seq_a, _), (seq_b, _) in zip(row_a, row_b):
            assert seq_b.shape == seq_a.shape == (M_L + N_NEW,)
            # the caller's padded row, pads included
            assert torch.equal(seq_b[:M_L], ids[b])
        worst = max(worst, max(abs(a - c) for a, c in zip(sc_a, sc_b)))
    print(f"largest sorted-score difference packed vs padded: {worst:.3e}")
    assert worst <= SCORE_TOL, worst


def test_packed_prefill_errors():
    m, ids, attn = _lcrec()
    kw = dict(attention_mask=attn, max_new_tokens=2, beam_width=2)
    with pytest.raises(ValueError, match="shared_prefix"):
        m.generate_topk(ids, prefill="packed", **kw)
    with pytest.raises(ValueError, match="prefill"):
        m.generate_topk(ids, prefill="ragged", beam_cache="shared_prefix",
                        **kw)
    sdpa, ids, attn = _lcrec("sdpa")
    with pytest.raises(ValueError, match="genrec_gqa"):
        sdpa.generate_topk(ids, prefill="packed", beam_cache="shared_prefix",
                           **kw)
