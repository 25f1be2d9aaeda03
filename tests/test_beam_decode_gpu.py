"""Shared-prefix beam-search decode attention
(csrc/kernels/attention_beam.hip) and LCRec.generate_topk's
beam_cache="shared_prefix" path, on the GPU.

Kernel tolerance rule (that of test_gqa_attention_gpu.py): the kernel and
PyTorch's own bf16 SDPA (math backend, on the expanded per-beam K/V) are
both diffed against the fp32 eager op on the same bf16-rounded inputs, and

    max|kernel - ref| <= 2 * max|sdpa_bf16 - ref| + ulp_bf16(max|ref|)
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


def _dev():
    return torch.device("cuda:0")


def _ulp_bf16(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


@functools.lru_cache(maxsize=None)
def _case(D, hq, hkv, W, lp, T, t, pads=None):
    """Inputs ([B,L,H,D] storage), fp32 reference and bf16-SDPA baseline of
    one case, computed once and shared (never modified) by the tests."""
    g = torch.Generator(device="cpu").manual_seed(
        D * 1000003 + hq * 10007 + W * 101 + lp * 7 + T + t)
    dev = _dev()

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)

    q_s = rnd(B * W, 1, hq, D)
    k_s, v_s = rnd(B, lp, hkv, D), rnd(B, lp, hkv, D)
    k_suf, v_suf = rnd(B, T, W, hkv, D), rnd(B, T, W, hkv, D)
    anc = torch.randint(0, W, (B, W, T), generator=g, dtype=torch.int32)
    if W > 1:
        anc[:, 1] = anc[:, 0]          # two beams inherit the same slots
    anc = anc.to(dev)
    pad = None
    if pads is not None:
        pad = (torch.arange(lp, device=dev)[None, :]
               < torch.tensor(pads, device=dev)[:, None])
    scale = D ** -0.5

    ref = eager.beam_decode_attention(
        q_s.float().transpose(1, 2), k_s.float().transpose(1, 2),
        v_s.float().transpose(1, 2), k_suf.float(), v_suf.float(), anc, t,
        pre_pad=pad, scale=scale)

    from torch.nn.attention import SDPBackend, sdpa_kernel

    k, v, key_pad = eager.beam_kv_expand(
        k_s.transpose(1, 2), v_s.transpose(1, 2), k_suf, v_suf, anc, t, pad)
    mask = None if key_pad is None else ~key_pad[:, None, None, :]
    rep = hq // hkv
    with sdpa_kernel(SDPBackend.MATH):
        base = F.scaled_dot_product_attention(
            q_s.transpose(1, 2), k.repeat_interleave(rep, 1),
            v.repeat_interleave(rep, 1), attn_mask=mask, scale=scale)
    base = base.transpose(1, 2)                             # [B*W,1,Hq,D]
    return dict(q_s=q_s, k_s=k_s, v_s=v_s, k_suf=k_suf, v_suf=v_suf, anc=anc,
                pad=pad, t=t, scale=scale, ref=ref, base=base)


def _run_kernel(c, splits=0, contiguous=False, **over):
    q, k, v = (x.transpose(1, 2) for x in (c["q_s"], c["k_s"], c["v_s"]))
    if contiguous:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    a = dict(k_pre=k, v_pre=v, k_suf=c["k_suf"], v_suf=c["v_suf"],
             anc=c["anc"], pad=c["pad"])
    a.update(over)
    assert ops.beam_decode_supported(q, a["k_pre"], a["v_pre"], a["k_suf"],
                                     a["v_suf"], a["anc"])
    return ops.beam_decode_attention(
        q, a["k_pre"], a["v_pre"], a["k_suf"], a["v_suf"], a["anc"], c["t"],
        pre_pad=a["pad"], scale=c["scale"], _splits=splits)


def _check(c, got, label):
    ref, base = c["ref"], c["base"].float()
    assert got.shape == ref.shape and got.dtype == torch.bfloat16
    assert got.is_contiguous() and torch.isfinite(got).all(), label
    err_k = (got.float() - ref).abs().max().item()
    err_b = (base - ref).abs().max().item()
    bound = 2 * err_b + _ulp_bf16(ref.abs().max().item())
    print(f"{label}: kernel {err_k:.3e} sdpa_bf16 {err_b:.3e} "
          f"bound {bound:.3e}")
    assert err_k <= bound, (label, err_k, err_b, bound)


PACK = {"60rows": (12, 2, 10), "70rows": (14, 2, 10), "6rows": (4, 2, 3),
        "1row": (2, 2, 1)}

# (D, packing, Lp, T, t, pads per prompt, _splits, contiguous inputs)
CASES = [
    # every packing at both head dims: ragged 3-tile prefix, pads, default
    # split choice
    (64, "60rows", 130, 4, 2, (3, 0), 0, False),
    (128, "60rows", 130, 4, 2, (3, 0), 0, False),
    (64, "70rows", 130, 16, 16, (0, 129), 0, False),
    (128, "70rows", 130, 16, 16, (0, 129), 0, False),
    (64, "6rows", 130, 4, 4, None, 0, True),
    (128, "6rows", 130, 4, 4, None, 0, True),
    (64, "1row", 130, 4, 1, (70, 0), 0, False),
    (128, "1row", 130, 4, 1, (70, 0), 0, False),
    # prefix lengths around the tile edge
    (128, "60rows", 1, 4, 1, None, 0, False),
    (64, "6rows", 1, 16, 2, None, 3, True),       # 3 splits of one tile
    (128, "6rows", 63, 4, 2, (62, 0), 1, False),
    (64, "60rows", 63, 16, 16, (0, 5), 2, True),
    (128, "70rows", 64, 4, 4, (63, 0), 1, True),
    (64, "6rows", 64, 16, 1, None, 2, False),
    (128, "60rows", 65, 16, 2, (0, 64), 2, False),
    (64, "70rows", 65, 4, 1, (64, 3), 3, False),  # more splits than tiles
    (128, "1row", 65, 16, 16, None, 1, True),
    # split counts on the 3-tile prefix, whole leading tile padded
    (128, "60rows", 130, 16, 2, (70, 0), 1, False),
    (128, "60rows", 130, 16, 2, (70, 0), 2, False),
    (128, "60rows", 130, 16, 2, (70, 0), 3, True),
    (128, "60rows", 130, 16, 2, (70, 0), 5, False),
    (64, "70rows", 130, 4, 2, (129, 64), 2, True),
    (64, "70rows", 130, 4, 2, (129, 64), 5, False),
    (64, "6rows", 130, 16, 16, (0, 129), 3, False),
    (128, "1row", 130, 4, 4, (129, 0), 7, False),
]


def _id(case):
    D, pack, lp, T, t, pads, splits, contig = case
    return (f"D{D}-{pack}-Lp{lp}-T{T}-t{t}-pad{pads}-s{splits}-"
            f"{'contig' if contig else 'view'}")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernel_matches_reference(case):
    D, pack, lp, T, t, pads, splits, contig = case
    hq, hkv, W = PACK[pack]
    c = _case(D, hq, hkv, W, lp, T, t, pads)
    _check(c, _run_kernel(c, splits, contig), _id(case))


@pytest.mark.parametrize("D", [64, 128])
def test_layouts_and_split_counts_agree(D):
    c = _case(D, 12, 2, 10, 130, 4, 2, (3, 0))
    view = _run_kernel(c, 2, contiguous=False)
    assert torch.equal(view, _run_kernel(c, 2, contiguous=True))
    # another split count only changes the fold order
    other = _run_kernel(c, 3)
    assert (view.float() - other.float()).abs().max().item() \
        <= 2 * _ulp_bf16(c["ref"].abs().max().item())


@pytest.mark.parametrize("D,pack", [(64, "70rows"), (128, "60rows")])
def test_garbage_outside_live_region(D, pack):
    hq, hkv, W = PACK[pack]
    c = _case(D, hq, hkv, W, 130, 16, 2, (70, 0))
    t = c["t"]
    clean = _run_kernel(c, 2)
    k_suf, v_suf, anc = c["k_suf"].clone(), c["v_suf"].clone(), \
        c["anc"].clone()
    k_suf[:, t:] = float("nan")
    v_suf[:, t:] = float("nan")
    anc[:, :, t:] = 1 << 30
    anc[:, 0, t:] = -7
    assert torch.equal(clean, _run_kernel(c, 2, k_suf=k_suf, v_suf=v_suf,
                                          anc=anc))
    # whatever padded prompt positions hold never reaches the output
    k_s, v_s = c["k_s"].clone(), c["v_s"].clone()
    k_s[c["pad"]] = float("nan")
    v_s[c["pad"]] = float("nan")
    dirty = _run_kernel(c, 2, k_pre=k_s.transpose(1, 2),
                        v_pre=v_s.transpose(1, 2))
    assert torch.isfinite(dirty).all()
    _check(c, dirty, f"NaN pads D{D} {pack}")


@pytest.mark.parametrize("splits", [0, 3])
def test_determinism(splits):
    c = _case(128, 14, 2, 10, 130, 16, 16, (0, 129))
    assert torch.equal(_run_kernel(c, splits), _run_kernel(c, splits))


def test_pick_splits_is_bounded_by_tiles():
    ext = ops.ext()
    assert ext.beam_attn_pick_splits(32, 2, 60, 512) <= 8
    assert ext.beam_attn_pick_splits(1, 2, 60, 512) == 8
    assert ext.beam_attn_pick_splits(1, 2, 60, 1) == 1
    assert ext.beam_attn_pick_splits(4096, 2, 60, 512) == 1


def test_unsupported_inputs_fall_back(monkeypatch):
    c = _case(64, 4, 2, 3, 130, 4, 2, (3, 0))
    q, k, v = (x.transpose(1, 2) for x in (c["q_s"], c["k_s"], c["v_s"]))
    args = (q, k, v, c["k_suf"], c["v_suf"], c["anc"])
    want = _run_kernel(c)
    bound = 2 * _ulp_bf16(c["ref"].abs().max().item())
    # the kill switch
    monkeypatch.setenv("GENREC_DISABLE_ATTN_BEAM", "1")
    assert not ops.beam_decode_supported(*args)
    got = ops.beam_decode_attention(*args, c["t"], pre_pad=c["pad"],
                                    scale=c["scale"])
    monkeypatch.delenv("GENREC_DISABLE_ATTN_BEAM")
    assert got.shape == want.shape
    assert (got.float() - want.float()).abs().max().item() <= bound
    # more suffix slots than the kernel unrolls: T = 17
    k17 = torch.cat([c["k_suf"]] * 5, 1)[:, :17].contiguous()
    v17 = torch.cat([c["v_suf"]] * 5, 1)[:, :17].contiguous()
    a17 = torch.cat([c["anc"]] * 5, 2)[:, :, :17].contiguous()
    assert not ops.beam_decode_supported(q, k, v, k17, v17, a17)
    got = ops.beam_decode_attention(q, k, v, k17, v17, a17, c["t"],
                                    pre_pad=c["pad"], scale=c["scale"])
    assert (got.float() - want.float()).abs().max().item() <= bound
    # the host wrapper itself rejects what the predicate keeps away from it
    with pytest.raises(RuntimeError, match="T <= 16"):
        ops.ext().beam_attn_fwd(q, k, v, c["pad"], k17, v17, a17, 2,
                                c["scale"], 0)
    with pytest.raises(RuntimeError, match="head dim"):
        ops.ext().beam_attn_fwd(q[..., :32], k[..., :32], v[..., :32],
                                c["pad"], c["k_suf"][..., :32].contiguous(),
                                c["v_suf"][..., :32].contiguous(), c["anc"],
                                2, c["scale"], 0)


# --------------------------------------------------------------- model level

QWEN = dict(vocab_size=512, hidden_size=256, num_layers=2, num_heads=4,
            num_kv_heads=2, intermediate_size=256)   # head_dim 64
N_NEW, M_W = 4, 4
M_L, M_PADS = 70, [66, 0, 3]


@functools.lru_cache(maxsize=None)
def _model():
    from genrec_amd.models.lcrec import LCRec, default_qwen_config

    torch.manual_seed(0)
    m = LCRec(config=default_qwen_config(**QWEN),
              attn_implementation="genrec_gqa")
    m.add_codebook_tokens(N_NEW, 8)
    # spread the (tied-head) logits so that few candidates nearly tie, and
    # keep the attention scores moderate
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.normal_(0, 0.25 if "embed_tokens" in name else 0.05)
    m = m.to(_dev()).to(torch.bfloat16).eval()
    ids = torch.randint(0, 256, (len(M_PADS), M_L),
                        generator=torch.Generator().manual_seed(1)).to(_dev())
    attn = (torch.arange(M_L, device=_dev())[None, :]
            >= torch.tensor(M_PADS, device=_dev())[:, None]).long()
    return m, ids, attn


def _generate(m, ids, attn, beam_cache, n_new=N_NEW, width=M_W):
    allowed = list(m.codebook_token_ids(N_NEW, 8))[:n_new]
    return m.generate_topk(ids, attention_mask=attn, max_new_tokens=n_new,
                           beam_width=width, allowed_token_ids=allowed,
                           beam_cache=beam_cache)


class _CountingExt:
    """ops.ext() stand-in that counts beam_attn_fwd calls."""

    def __init__(self, real):
        self._real, self.calls = real, 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name != "beam_attn_fwd":
            return fn

        def counted(*args, **kwargs):
            self.calls += 1
            return fn(*args, **kwargs)

        return counted


def test_dispatch_proof(monkeypatch):
    m, ids, attn = _model()
    ext = _CountingExt(ops.ext())
    monkeypatch.setattr(ops, "ext", lambda: ext)
    _generate(m, ids, attn, None, 3, 2)
    assert ext.calls == 0
    on = _generate(m, ids, attn, "shared_prefix", 3, 2)
    # every layer of every decode step
    assert ext.calls == QWEN["num_layers"] * 2
    monkeypatch.setenv("GENREC_DISABLE_ATTN_BEAM", "1")
    off = _generate(m, ids, attn, "shared_prefix", 3, 2)
    assert ext.calls == QWEN["num_layers"] * 2
    for row_a, row_b in zip(on, off):
        for (seq_a, _), (seq_b, _) in zip(row_a, row_b):
            assert torch.equal(seq_a, seq_b)


def _rescore(m, seq, pad_count):
    """Summed log-probability of seq's N_NEW generated tokens from one
    uncached full forward (what the beam score accumulates)."""
    attn = (torch.arange(seq.numel(), device=seq.device)
            >= pad_count).long()[None]
    with torch.no_grad():
        logits = m.model(input_ids=seq[None], attention_mask=attn,
                         use_cache=False).logits[0]
    lp = F.log_softmax(logits[M_L - 1:-1], dim=-1)
    return float(lp.gather(1, seq[M_L:, None]).sum())


def test_end_to_end_scores_match_uncached_forward():
    m, ids, attn = _model()
    worst, top = {}, 0.0
    for name, mode in (("default", None), ("shared_prefix", "shared_prefix")):
        res = _generate(m, ids, attn, mode)
        assert len(res) == len(M_PADS) and all(len(r) == M_W for r in res)
        err = 0.0
        for pad_count, row in zip(M_PADS, res):
            scores = [s for _, s in row]
            assert scores == sorted(scores, reverse=True)
            for seq, score in row:
                assert math.isfinite(score) and seq.numel() == M_L + N_NEW
                err = max(err, abs(score - _rescore(m, seq, pad_count)))
                top = max(top, abs(score))
        worst[name] = err
    bound = 2 * worst["default"] + _ulp_bf16(top)
    print(f"worst |beam score - uncached rescoring|: default "
          f"{worst['default']:.3e} shared_prefix "
          f"{worst['shared_prefix']:.3e} bound {bound:.3e}")
    assert worst["shared_prefix"] <= bound, (worst, bound)


def test_peak_memory_below_expanded_cache():
    m, _, _ = _model()
    Bm, Wm, Lm = 4, 8, 256
    ids = torch.randint(0, 256, (Bm, Lm),
                        generator=torch.Generator().manual_seed(2)).to(_dev())
    allowed = list(m.codebook_token_ids(N_NEW, 8))
    peak = {}
    for name, mode in (("default", None), ("shared_prefix", "shared_prefix")):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        m.generate_topk(ids, max_new_tokens=N_NEW, beam_width=Wm,
                        allowed_token_ids=allowed, beam_cache=mode)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - before
    assert peak["shared_prefix"] < peak["default"], (
        f"peak bytes above the start of generate_topk: shared_prefix "
        f"{peak['shared_prefix']} default {peak['default']}")
