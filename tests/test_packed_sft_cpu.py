"""Padding-free (packed) LCRec SFT on the CPU: the eager varlen attention,
the packing collate, the packed model path against the padded one, the
error paths and the trainer switch.

Model tolerance (loss and every parameter gradient, fp32): the padded batch
is run twice, once with its rows in reversed order, which changes only the
order of summation. A packed run may differ from the padded run by

    4 * max|padded - padded_reversed| + ulp_fp32(max|padded|)

per compared tensor; 4x because a different row count reorders more sums
than a permutation does.
"""

import copy
import functools
import math

import pytest
import torch

from genrec_amd.models.lcrec import LCRec, default_qwen_config
from genrec_amd.ops import eager

TINY = dict(vocab_size=512, hidden_size=64, num_layers=2, num_heads=4,
            num_kv_heads=2, intermediate_size=128)
LENS = [5, 70, 33, 64]


def _ulp_fp32(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(max(x, 1e-37))) - 23)


# ------------------------------------------------------------- eager varlen

def test_eager_varlen_matches_per_sequence_calls():
    g = torch.Generator().manual_seed(0)
    lens = [1, 9, 0, 17, 4]
    T, hq, hkv, D = sum(lens) + 6, 4, 2, 16           # 6-token tail
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)),
                      dtype=torch.int32)
    q, k, v = (torch.randn(T, h, D, generator=g).requires_grad_()
               for h in (hq, hkv, hkv))
    dout = torch.randn(T, hq, D, generator=g)
    scale = D ** -0.5
    out = eager.gqa_varlen_attention(q, k, v, cu, max(lens), scale=scale)
    assert out.shape == (T, hq, D)
    out.backward(dout)

    ref_out = torch.zeros_like(out)
    ref_g = [torch.zeros_like(t) for t in (q, k, v)]
    for s, n in enumerate(lens):
        if n == 0:
            continue
        a, e = int(cu[s]), int(cu[s + 1])
        qs, ks, vs = (t.detach()[a:e].transpose(0, 1)[None].requires_grad_()
                      for t in (q, k, v))
        o = eager.gqa_attention(qs, ks, vs, scale=scale, causal=True)
        o.backward(dout[a:e][None])
        ref_out[a:e] = o.detach()[0]
        for dst, src in zip(ref_g, (qs, ks, vs)):
            dst[a:e] = src.grad[0].transpose(0, 1)
    torch.testing.assert_close(out.detach(), ref_out)
    for got, ref in zip((q.grad, k.grad, v.grad), ref_g):
        torch.testing.assert_close(got, ref)
    # the tail belongs to no sequence: exactly zero, forward and backward
    tail = int(cu[-1])
    assert (out.detach()[tail:] == 0).all()
    for t in (q, k, v):
        assert (t.grad[tail:] == 0).all()
    assert torch.isfinite(out).all()


def test_eager_varlen_all_empty():
    q = torch.randn(8, 2, 16)
    cu = torch.tensor([0, 0, 0], dtype=torch.int32)
    out = eager.gqa_varlen_attention(q, q, q, cu, 0, scale=0.25)
    assert (out == 0).all()


def test_op_takes_eager_path_on_cpu():
    from genrec_amd import ops

    q = torch.randn(12, 4, 64, requires_grad=True)
    k = torch.randn(12, 2, 64)
    cu = torch.tensor([0, 5, 12], dtype=torch.int32)
    out = ops.gqa_varlen_attention(q, k, k, cu, 7, scale=0.125)
    assert "GqaVarlen" not in type(out.grad_fn).__name__
    assert not ops.gqa_varlen_supported(q, k, k, cu)
    torch.testing.assert_close(
        out, eager.gqa_varlen_attention(q, k, k, cu, 7, scale=0.125))


# ------------------------------------------------------------------ collate

@pytest.fixture(scope="module")
def tok_model():
    torch.manual_seed(0)
    m = LCRec(config=default_qwen_config(**TINY),
              attn_implementation="genrec_gqa")
    m.add_codebook_tokens(3, 8)
    return m


SAMPLES = [
    {"prompt": "predict: <C0_1>", "response": "<C1_2>"},
    {"prompt": "a much longer prompt with history <C0_3><C1_4><C2_5> " * 3,
     "response": "<C0_2><C1_5><C2_5>"},
    {"prompt": "", "response": "<C2_5> and some text"},
    {"prompt": "title of item <C0_7>", "response": "a title"},
]


def _supervised_pairs(ids, labels):
    """Multiset of (context token, target) pairs the shifted loss scores."""
    pairs = []
    for row_i, row_l in zip(ids.tolist(), labels.tolist()):
        pairs += [(a, b) for a, b in zip(row_i[:-1], row_l[1:]) if b != -100]
    return sorted(pairs)


def test_collate_packing_layout(tok_model):
    from genrec_amd.trainers.lcrec_trainer import sft_collate

    padded = sft_collate(SAMPLES, tok_model, max_len=48)
    packed = sft_collate(SAMPLES, tok_model, max_len=48, packing=True)
    lens = padded["attention_mask"].sum(1).tolist()
    assert max(lens) == 48 and min(lens) < 48          # truncation is hit
    cu = packed["cu_seq_lens"]
    assert cu.dtype == torch.int32 and cu.tolist() == \
        [0] + torch.tensor(lens).cumsum(0).tolist()
    assert packed["max_length"] == max(lens)
    assert isinstance(packed["max_length"], int)
    T = packed["input_ids"].size(1)
    assert T % 64 == 0 and 0 <= T - sum(lens) < 64
    for key in ("input_ids", "labels", "position_ids"):
        assert packed[key].shape == (1, T) and packed[key].dtype == torch.long
    assert "attention_mask" not in packed
    pos = packed["position_ids"][0]
    for s, n in enumerate(lens):
        a = int(cu[s])
        assert pos[a:a + n].tolist() == list(range(n))
        assert packed["input_ids"][0, a:a + n].tolist() == \
            padded["input_ids"][s, :n].tolist()
        assert packed["labels"][0, a].item() == -100   # first token masked
    tail = int(cu[-1])
    assert (packed["labels"][0, tail:] == -100).all()
    assert (pos[tail:] == 0).all()
    assert (packed["input_ids"][0, tail:]
            == tok_model.tokenizer.pad_token_id).all()
    assert _supervised_pairs(packed["input_ids"], packed["labels"]) == \
        _supervised_pairs(padded["input_ids"], padded["labels"])
    # another multiple, and an exact fit adds nothing
    p8 = sft_collate(SAMPLES, tok_model, max_len=48, packing=True,
                     pad_to_multiple_of=8)
    assert p8["input_ids"].size(1) == -(-sum(lens) // 8) * 8
    with pytest.raises(ValueError):
        sft_collate(SAMPLES, tok_model, for_generation=True, packing=True)


def test_collate_without_packing_is_unchanged(tok_model):
    from genrec_amd.trainers.lcrec_trainer import sft_collate

    tok = tok_model.tokenizer
    out = sft_collate(SAMPLES, tok_model, max_len=48)
    assert set(out) == {"input_ids", "attention_mask", "labels"}
    rows = []
    for s in SAMPLES:
        p = tok(s["prompt"]).input_ids
        r = tok(s["response"]).input_ids + [tok.eos_token_id]
        rows.append(((p + r)[:48], ([-100] * len(p) + r)[:48]))
    L = max(len(i) for i, _ in rows)
    exp_ids = [i + [tok.pad_token_id] * (L - len(i)) for i, _ in rows]
    exp_lab = [l + [-100] * (L - len(l)) for _, l in rows]
    exp_att = [[1] * len(i) + [0] * (L - len(i)) for i, _ in rows]
    assert out["input_ids"].tolist() == exp_ids
    assert out["labels"].tolist() == exp_lab
    assert out["attention_mask"].tolist() == exp_att
    gen = sft_collate(SAMPLES, tok_model, max_len=48, for_generation=True)
    assert set(gen) == {"input_ids", "attention_mask", "meta"}
    assert gen["attention_mask"][0, 0].item() == 0      # left-padded


# -------------------------------------------------------------------- model

@functools.lru_cache(maxsize=None)
def _batches():
    """The padded batch (and its row-reversed copy) and the packed batch of
    the same four samples."""
    g = torch.Generator().manual_seed(1)
    L = max(LENS)
    ids = torch.zeros(len(LENS), L, dtype=torch.long)
    labels = torch.full((len(LENS), L), -100, dtype=torch.long)
    attn = torch.zeros(len(LENS), L, dtype=torch.long)
    for s, n in enumerate(LENS):
        ids[s, :n] = torch.randint(1, 256, (n,), generator=g)
        attn[s, :n] = 1
        n_prompt = n // 2
        labels[s, n_prompt:n] = ids[s, n_prompt:n]
        labels[s, 0] = -100
    T = -(-sum(LENS) // 64) * 64
    p_ids = torch.zeros(1, T, dtype=torch.long)
    p_lab = torch.full((1, T), -100, dtype=torch.long)
    p_pos = torch.zeros(1, T, dtype=torch.long)
    cu = [0]
    for s, n in enumerate(LENS):
        a = cu[-1]
        p_ids[0, a:a + n] = ids[s, :n]
        p_lab[0, a:a + n] = labels[s, :n]
        p_pos[0, a:a + n] = torch.arange(n)
        cu.append(a + n)
    padded = dict(input_ids=ids, attention_mask=attn, labels=labels)
    rev = {k: v.flip(0) for k, v in padded.items()}
    packed = dict(input_ids=p_ids, labels=p_lab, position_ids=p_pos,
                  cu_seq_lens=torch.tensor(cu, dtype=torch.int32),
                  max_length=max(LENS))
    return padded, rev, packed


def _loss_and_grads(model, batch):
    model.zero_grad()
    out = model(**batch)
    out.loss.backward()
    res = {"loss": out.loss.detach().clone()}
    for n, p in model.named_parameters():
        if p.grad is not None:
            res[n] = p.grad.detach().clone()
    model.zero_grad()
    return res


@pytest.mark.parametrize("layers", [None, "genrec_fused"])
@pytest.mark.parametrize("loss", [None, "genrec_lce"])
def test_packed_model_matches_padded(loss, layers):
    torch.manual_seed(0)
    m = LCRec(config=default_qwen_config(**TINY),
              attn_implementation="genrec_gqa", loss_implementation=loss,
              layer_implementation=layers).float()
    padded, rev, packed = _batches()
    ref = _loss_and_grads(m, padded)
    perm = _loss_and_grads(m, rev)
    got = _loss_and_grads(m, packed)
    assert set(got) == set(ref) and len(ref) > 10
    worst = 0.0
    for name, r in ref.items():
        noise = (perm[name] - r).abs().max().item()
        bound = 4 * noise + _ulp_fp32(r.abs().max().item())
        err = (got[name] - r).abs().max().item()
        worst = max(worst, err / bound)
        if name == "loss" or err > bound:
            print(f"{loss}/{layers} {name}: packed {err:.3e} permuted "
                  f"{noise:.3e} bound {bound:.3e}")
        assert math.isfinite(err) and err <= bound, (name, err, noise, bound)
    print(f"{loss}/{layers}: worst err/bound {worst:.3f}")


def test_packed_samples_do_not_see_each_other(tok_model):
    """Logits of each packed sample equal a forward of that sample alone."""
    m = copy.deepcopy(tok_model).float().eval()
    _, _, packed = _batches()
    with torch.no_grad():
        logits = m(packed["input_ids"], position_ids=packed["position_ids"],
                   cu_seq_lens=packed["cu_seq_lens"],
                   max_length=packed["max_length"]).logits[0]
        cu = packed["cu_seq_lens"].tolist()
        for s in range(len(LENS)):
            alone = m(packed["input_ids"][:, cu[s]:cu[s + 1]]).logits[0]
            torch.testing.assert_close(logits[cu[s]:cu[s + 1]], alone,
                                       atol=2e-5, rtol=1e-4)


# -------------------------------------------------------------- error paths

def test_cu_seq_lens_needs_genrec_gqa():
    torch.manual_seed(0)
    m = LCRec(config=default_qwen_config(**TINY), attn_implementation="sdpa")
    _, _, packed = _batches()
    with pytest.raises(ValueError, match="genrec_gqa"):
        m(**packed)
    m2 = LCRec(config=default_qwen_config(**TINY))
    with pytest.raises(ValueError, match="genrec_gqa"):
        m2(**packed)


def test_packed_model_input_checks(tok_model):
    _, _, packed = _batches()
    bad = dict(packed, position_ids=None)
    with pytest.raises(ValueError, match="position_ids"):
        tok_model(**bad)
    two = dict(packed, input_ids=packed["input_ids"].expand(2, -1))
    with pytest.raises(ValueError, match=r"\[1,T\]"):
        tok_model(**two)


def test_adapter_raises_instead_of_falling_back():
    from genrec_amd.modules.hf_attention import genrec_gqa_attention_forward

    class Mod(torch.nn.Module):
        is_causal = True
        layer_idx = 0

    mod = Mod()
    q = torch.randn(1, 4, 12, 16)
    k = torch.randn(1, 2, 12, 16)
    cu = torch.tensor([0, 5, 12], dtype=torch.int32)
    kw = dict(cu_seq_lens_q=cu, cu_seq_lens_k=cu, max_length_q=7,
              max_length_k=7)
    out, _ = genrec_gqa_attention_forward(mod, q, k, k, None, **kw)
    assert out.shape == (1, 12, 4, 16)
    with pytest.raises(ValueError, match="sliding window"):
        genrec_gqa_attention_forward(mod, q, k, k, None, sliding_window=8,
                                     **kw)
    with pytest.raises(ValueError, match="dropout"):
        genrec_gqa_attention_forward(mod.train(), q, k, k, None, dropout=0.1,
                                     **kw)
    with pytest.raises(ValueError, match="causal"):
        genrec_gqa_attention_forward(mod, q, k, k, None, is_causal=False,
                                     **kw)
    with pytest.raises(ValueError, match="position_bias"):
        genrec_gqa_attention_forward(mod, q, k, k, None,
                                     position_bias=torch.zeros(1), **kw)
    with pytest.raises(ValueError, match="one row"):
        genrec_gqa_attention_forward(mod, q.expand(2, -1, -1, -1),
                                     k.expand(2, -1, -1, -1),
                                     k.expand(2, -1, -1, -1), None, **kw)
    with pytest.raises(ValueError, match="same offsets"):
        genrec_gqa_attention_forward(mod, q, k, k, None,
                                     **dict(kw, cu_seq_lens_k=cu.clone()))


# ------------------------------------------------------------------ trainer

def test_trainer_packing_with_gradient_checkpointing(tmp_path, monkeypatch):
    from genrec_amd.trainers import lcrec_trainer

    seen = []
    fwd = LCRec.forward

    def spy(self, *a, **kw):
        out = fwd(self, *a, **kw)
        if kw.get("cu_seq_lens") is not None:
            seen.append((kw["input_ids"].shape, float(out.loss.detach())))
        return out

    monkeypatch.setattr(LCRec, "forward", spy)
    lcrec_trainer.train(
        epochs=1, max_steps=2, batch_size=4, max_seq_len=64,
        n_codebooks=3, codebook_size=8, backbone_config=dict(TINY),
        gradient_checkpointing=True, use_lora=False, packing=True,
        attn_implementation="genrec_gqa",
        max_train_samples=8, max_eval_samples=2, do_eval=False,
        save_dir_root=str(tmp_path), save_every_epoch=10,
        wandb_logging=False, num_workers=0)
    assert len(seen) == 2
    for shape, loss in seen:
        assert shape[0] == 1 and shape[1] % 64 == 0
        assert math.isfinite(loss)
