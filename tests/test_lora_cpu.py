"""LoRA on the CPU: the torch form of the adapted linear (eager.lora_linear,
the reference for the kernels of csrc/kernels/lora.hip), the LoRALinear /
apply_lora module layer, merged and adapter checkpoints, and the LCRec
trainer with lora_implementation="genrec"."""

import json
import math
import os

import pytest
import torch
from torch import nn

from genrec_amd import ops
from genrec_amd.models.lcrec import LCRec, default_qwen_config
from genrec_amd.modules import lora
from genrec_amd.ops import eager

TINY = dict(vocab_size=512, hidden_size=64, num_layers=2, num_heads=4,
            num_kv_heads=2, intermediate_size=128)


def _inputs(M, K, N, r, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) \
        .to(dtype).requires_grad_(True)
    return mk(M, K), mk(N, K), mk(N), mk(r, K), mk(N, r)


# ------------------------------------------------------------------- op

@pytest.mark.parametrize("p", [0.0, 0.25])
def test_eager_lora_linear_matches_formula(p):
    M, K, N, r, s, seed = 7, 24, 16, 16, 2.0, 1234
    x, w, b, a, bb = _inputs(M, K, N, r, torch.float64)
    y = eager.lora_linear(x, w, b, a, bb, s, p=p, training=True, seed=seed)
    dy = torch.randn(M, N, dtype=torch.float64,
                     generator=torch.Generator().manual_seed(1))
    got = torch.autograd.grad(y, (x, a, bb, w, b), dy)

    x2, w2, b2, a2, bb2 = (t.detach().clone().requires_grad_(True)
                           for t in (x, w, b, a, bb))
    mask = eager.lora_dropout_mask(M, K, p, seed).double() if p > 0 \
        else torch.ones(M, K, dtype=torch.float64)
    keep = 1.0 - p
    ref = x2 @ w2.t() + b2 + s * (((x2 * mask / keep) @ a2.t()) @ bb2.t())
    want = torch.autograd.grad(ref, (x2, a2, bb2, w2, b2), dy)
    torch.testing.assert_close(y, ref, rtol=1e-12, atol=1e-12)
    for name, g_, w_ in zip(("dx", "dA", "dB", "dweight", "dbias"), got, want):
        torch.testing.assert_close(g_, w_, rtol=1e-12, atol=1e-12, msg=name)
    if p > 0:
        assert 0 < mask.sum() < mask.numel()


def test_eager_lora_linear_eval_ignores_dropout():
    x, w, b, a, bb = _inputs(5, 16, 8, 16, torch.float64)
    y0 = eager.lora_linear(x, w, b, a, bb, 0.5, p=0.5, training=False)
    y1 = eager.lora_linear(x, w, b, a, bb, 0.5, p=0.0, training=True)
    assert torch.equal(y0, y1)


def test_eager_lora_linear_skips_frozen_base_grads():
    x, w, b, a, bb = _inputs(5, 16, 8, 16, torch.float32)
    w.requires_grad_(False)
    b.requires_grad_(False)
    y = ops.lora_linear(x, w, b, a, bb, 2.0)
    y.sum().backward()
    assert w.grad is None and b.grad is None
    assert x.grad is not None and a.grad is not None and bb.grad is not None


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_gradcheck(p):
    x, w, b, a, bb = _inputs(5, 16, 8, 16, torch.float64, seed=3)
    fn = lambda *t: eager.lora_linear(*t, 2.0, p=p, training=True, seed=77)
    assert torch.autograd.gradcheck(fn, (x, w, b, a, bb))


def test_lora_dropout_mask():
    # 2^16 elements. One fixed seed is one draw: 3 sigma leaves 0.3 % of
    # the seeds outside (99 is such a seed, at 3.1 sigma).
    M, K, p, seed = 256, 256, 0.25, 7
    m0 = eager.lora_dropout_mask(M, K, p, seed)
    assert m0.dtype == torch.uint8 and m0.shape == (M, K)
    assert torch.equal(m0, eager.lora_dropout_mask(M, K, p, seed))
    assert not torch.equal(m0, eager.lora_dropout_mask(M, K, p, seed + 1))
    # the position is row * K + col: the same flat stream for any shape
    assert torch.equal(m0.view(-1),
                       eager.lora_dropout_mask(M * 2, K // 2, p, seed)
                       .view(-1))
    n = M * K
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(m0.float().mean().item() - (1 - p)) <= 3 * sigma
    assert eager.lora_dropout_mask(4, 8, 0.0, seed).all()


def test_mask_independent_of_strides():
    M, K, N, r, seed = 6, 16, 8, 16, 5
    x, w, b, a, bb = _inputs(M, K, N, r, torch.float32)
    wide = torch.zeros(M, K + 8)
    wide[:, :K] = x.detach()
    view = wide[:, :K]
    assert not view.is_contiguous()
    y0 = eager.lora_linear(x.detach(), w, b, a, bb, 2.0, p=0.25,
                           training=True, seed=seed)
    y1 = eager.lora_linear(view, w, b, a, bb, 2.0, p=0.25, training=True,
                           seed=seed)
    assert torch.equal(y0, y1)


# --------------------------------------------------------------- module

def test_fresh_adapter_is_identity():
    torch.manual_seed(0)
    base = nn.Linear(24, 16)
    x = torch.randn(3, 5, 24)
    want = base(x)
    for dropout, train in ((0.05, False), (0.0, True)):
        m = lora.LoRALinear(base, r=16, alpha=32, dropout=dropout)
        m.train(train)
        assert torch.equal(m(x), want)
    m = lora.LoRALinear(base, r=16, alpha=32, dropout=0.0)
    assert m.weight is base.weight and m.bias is base.bias
    assert (m.in_features, m.out_features) == (24, 16)
    assert m.scaling == 2.0
    assert tuple(m.lora_A.weight.shape) == (16, 24)
    assert tuple(m.lora_B.weight.shape) == (16, 16)
    assert not m.lora_B.weight.any() and m.lora_A.weight.any()
    assert not base.weight.requires_grad and not base.bias.requires_grad


def _tiny_causal_lm(layer_implementation=None):
    torch.manual_seed(0)
    return LCRec(config=default_qwen_config(**TINY),
                 layer_implementation=layer_implementation)


def _randomize_adapters(model, seed=1):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, lora.LoRALinear):
                m.lora_B.weight.copy_(
                    torch.randn(m.lora_B.weight.shape, generator=g) * 0.05)


def test_apply_lora_on_tiny_qwen2():
    m = _tiny_causal_lm()
    n = m.apply_lora(r=16, alpha=32, dropout=0.05)
    assert n == 14
    assert m.lora_config["r"] == 16 and m.lora_config["peft_type"] == "LORA"
    for name, prm in m.model.named_parameters():
        assert prm.requires_grad == (".lora_A." in name or ".lora_B." in name), name


def test_apply_lora_modules_to_save_and_subset():
    m = _tiny_causal_lm()
    n = m.apply_lora(target_modules=("q_proj", "v_proj"),
                     modules_to_save=("embed_tokens", "lm_head"))
    assert n == 4
    wrapped = {name.rsplit(".", 1)[-1] for name, mod in
               m.model.named_modules() if isinstance(mod, lora.LoRALinear)}
    assert wrapped == {"q_proj", "v_proj"}
    for name, prm in m.model.named_parameters():
        want = (".lora_A." in name or ".lora_B." in name
                or "embed_tokens" in name or "lm_head" in name)
        assert prm.requires_grad == want, name


def test_apply_lora_under_genrec_fused():
    m = _tiny_causal_lm("genrec_fused")
    plain = _tiny_causal_lm()
    assert m.apply_lora(dropout=0.0) == 14
    ids = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        assert torch.equal(m(ids).logits, plain(ids).logits)   # B = 0
    _randomize_adapters(m.model)
    out = m(ids, labels=ids)
    out.loss.backward()
    assert not torch.equal(out.logits, plain(ids).logits)
    for mod in m.model.modules():
        if isinstance(mod, lora.LoRALinear):
            assert mod.lora_A.weight.grad is not None
            assert mod.lora_B.weight.grad is not None


def test_merged_state_dict_matches_wrapped_model():
    m = _tiny_causal_lm()
    m.apply_lora()
    _randomize_adapters(m.model)
    m.eval()
    base_before = {k: v.clone() for k, v in m.model.state_dict().items()
                   if ".lora_" not in k}
    merged = lora.merged_state_dict(m.model)
    plain = _tiny_causal_lm()
    assert set(merged) == set(plain.model.state_dict())
    plain.model.load_state_dict(merged)
    plain.eval()
    ids = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        a, b = m(ids).logits, plain(ids).logits
    assert a.dtype == torch.float32
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    assert not torch.equal(b, _tiny_causal_lm().eval()(ids).logits)
    for k, v in m.model.state_dict().items():
        if ".lora_" not in k:
            assert torch.equal(v, base_before[k]), k


def test_adapter_save_load_roundtrip(tmp_path):
    from safetensors.torch import load_file

    m = _tiny_causal_lm()
    m.apply_lora(modules_to_save=("lm_head",))
    _randomize_adapters(m.model)
    m.eval()
    lora.save_adapter(m.model, str(tmp_path))
    tensors = load_file(str(tmp_path / lora.ADAPTER_WEIGHTS))
    key = "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"
    assert key in tensors and key.replace("lora_A", "lora_B") in tensors
    assert "base_model.model.lm_head.weight" in tensors
    lora_keys = [k for k in tensors if ".lora_" in k]
    assert len(lora_keys) == 28
    assert all(k.startswith("base_model.model.") and
               k.endswith((".lora_A.weight", ".lora_B.weight"))
               for k in lora_keys)
    cfg = json.load(open(tmp_path / lora.ADAPTER_CONFIG))
    assert cfg["peft_type"] == "LORA" and cfg["r"] == 16
    assert cfg["lora_alpha"] == 32 and cfg["lora_dropout"] == 0.05
    assert sorted(cfg["target_modules"]) == sorted(lora.DEFAULT_TARGET_MODULES)
    assert cfg["modules_to_save"] == ["lm_head"]

    m2 = _tiny_causal_lm()
    m2.apply_lora(modules_to_save=("lm_head",))
    lora.load_adapter(m2.model, str(tmp_path))
    m2.eval()
    ids = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        assert torch.equal(m(ids).logits, m2(ids).logits)


# -------------------------------------------------------------- trainer

@pytest.mark.parametrize("loss_implementation", [None, "genrec_lce"])
def test_trainer_with_native_lora(tmp_path, monkeypatch, loss_implementation):
    from genrec_amd.trainers import lcrec_trainer

    initial = {}
    real_apply = LCRec.apply_lora

    def spy(self, **kw):
        initial.update({k: v.detach().clone()
                        for k, v in self.model.state_dict().items()})
        return real_apply(self, **kw)

    monkeypatch.setattr(LCRec, "apply_lora", spy)
    model = lcrec_trainer.train(
        epochs=1, max_steps=3, batch_size=2, max_seq_len=64,
        n_codebooks=3, codebook_size=8, backbone_config=dict(TINY),
        gradient_checkpointing=True, use_lora=True,
        lora_implementation="genrec", learning_rate=1e-2,
        num_warmup_steps=1, loss_implementation=loss_implementation,
        max_train_samples=8, max_eval_samples=2, do_eval=False,
        save_dir_root=str(tmp_path), save_every_epoch=1,
        wandb_logging=False, num_workers=0)
    assert initial, "apply_lora was not called"
    adapters = [m for m in model.model.modules()
                if isinstance(m, lora.LoRALinear)]
    assert len(adapters) == 14
    for m in adapters:
        assert m.lora_A.weight.grad is not None
        assert m.lora_B.weight.grad is not None
        assert m.lora_B.weight.detach().abs().max() > 0
    for k, v in model.model.state_dict().items():
        if ".lora_" not in k:
            assert torch.equal(v.cpu(), initial[k.replace(".base_layer.", ".")]), k
    ck = os.path.join(tmp_path, "epoch_0")
    assert os.path.exists(os.path.join(ck, lora.ADAPTER_WEIGHTS))
    assert os.path.exists(os.path.join(ck, lora.ADAPTER_CONFIG))
    fresh = LCRec(config=default_qwen_config(**TINY))
    fresh.load_pretrained(ck)
    assert not any(isinstance(m, lora.LoRALinear)
                   for m in fresh.model.modules())
    merged = lora.merged_state_dict(model.model)
    got = fresh.model.state_dict()
    k = "model.layers.0.self_attn.q_proj.weight"
    torch.testing.assert_close(got[k].float(), merged[k].float().cpu(),
                               rtol=0, atol=1e-2)
    assert not torch.equal(got[k].float(), initial[k].float())


def test_trainer_rejects_unknown_lora_implementation(tmp_path):
    from genrec_amd.trainers import lcrec_trainer

    with pytest.raises(ValueError, match="lora_implementation"):
        lcrec_trainer.train(
            epochs=1, max_steps=1, batch_size=2, max_seq_len=64,
            n_codebooks=3, codebook_size=8, backbone_config=dict(TINY),
            use_lora=True, lora_implementation="peft2",
            save_dir_root=str(tmp_path), wandb_logging=False)
