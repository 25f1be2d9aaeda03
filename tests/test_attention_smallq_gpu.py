"""Small-query T5 attention kernels (attention_mfma.hip, Lq <= 16).

The small-query forward and backward must give, bit for bit, what the
64-row kernels give: the same MFMAs on the same operands, the same softmax
and Jacobian reduction orders, only all-padding fragments and k steps left
out. GENREC_ATTN_SMALLQ=0 keeps a call on the 64-row kernels, so every case
runs both on the same inputs and seed and compares every output with
torch.equal. The fp32 reference comparison of these shapes lives in
test_attention_tr_gpu.py, which now runs the new path.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KNOB = "GENREC_ATTN_SMALLQ"
# (Lq, Lk, D): the two decoder shapes of the TIGER step, the one-element
# case, the largest Lq with one / four key fragments, sizes that are no
# multiple of a fragment, and one query against a full key tile
SHAPES = [(4, 4, 64), (4, 61, 64), (1, 1, 32), (16, 16, 64), (16, 64, 64),
          (3, 17, 32), (1, 64, 64)]
KINDS = ["bias_pad", "causal_addmask", "causal_qmask", "none"]
OUTPUTS = ("out", "p_saved", "keep", "dq", "dk", "dv", "dbias")


def _ext():
    from genrec_amd import ops

    return ops.ext()


def _inputs(b, h, lq, lk, d, layout, kind):
    g = torch.Generator(device=DEV).manual_seed(1000 * lq + 10 * lk + d)

    def rn(*shape):
        return torch.randn(*shape, device=DEV, generator=g)

    if layout == "contig":
        q = rn(b, h, lq, d).bfloat16()
        k = rn(b, h, lk, d).bfloat16()
        v = rn(b, h, lk, d).bfloat16()
        dout = rn(b, h, lq, d).bfloat16()
    else:  # transpose views of the chunks of a fused projection output
        qkv_q = rn(b, lq, 3 * h * d).bfloat16()
        qkv_k = rn(b, lk, 3 * h * d).bfloat16()
        q = qkv_q.chunk(3, dim=-1)[0].view(b, lq, h, d).transpose(1, 2)
        k = qkv_k.chunk(3, dim=-1)[1].view(b, lk, h, d).transpose(1, 2)
        v = qkv_k.chunk(3, dim=-1)[2].view(b, lk, h, d).transpose(1, 2)
        dout = rn(b, lq, h, d).bfloat16().transpose(1, 2)
        assert q.stride(3) == 1 and q.stride(1) == d
    args = dict(q=q, k=k, v=v, dout=dout, bias=None, pad=None, am=None,
                qm=None, causal=False)
    if kind in ("bias_pad", "bias4d", "bias_bf16"):
        # the bias_pad setup of test_attention_tr_gpu.py, plus one batch
        # row whose keys are all padded
        shape = (b, h, lq, lk) if kind == "bias4d" else (h, lq, lk)
        bias = rn(*shape)
        args["bias"] = bias.bfloat16() if kind == "bias_bf16" else bias
        pad = torch.zeros(b, lk, dtype=torch.bool, device=DEV)
        if lk > 1 and b > 1:
            pad[1, (3 * lk) // 4:] = True
        pad[b - 1, :] = True
        args["pad"] = pad
    elif kind == "causal_addmask":
        args["am"] = torch.triu(
            torch.full((lq, lk), float("-inf"), device=DEV), 1)
    elif kind == "causal_qmask":
        args["causal"] = True
        qm = torch.ones(b, lq, device=DEV)
        qm[b - 1, lq // 2:] = 0.0
        args["qm"] = qm
    return args


def _run(a, p, seed=1234, seed_dev=None):
    ext = _ext()
    bias = a["bias"]
    out, p_saved, keep = ext.attn_fwd_mfma(
        a["q"], a["k"], a["v"], bias, a["pad"], a["am"], a["qm"], 0.125,
        a["causal"], 0, p, seed, seed_dev)
    dq, dk, dv, dbias = ext.attn_bwd_mfma(
        a["dout"], a["q"], a["k"], a["v"], p_saved, keep, a["qm"], 0.125, 0,
        p, seed, bias is not None, bias.dim() if bias is not None else 0)
    torch.cuda.synchronize()
    return dict(out=out, p_saved=p_saved, keep=keep, dq=dq, dk=dk, dv=dv,
                dbias=dbias)


def _parity(monkeypatch, b, h, shape, layout, kind, p, seed_dev=None):
    lq, lk, d = shape
    ext = _ext()
    a = _inputs(b, h, lq, lk, d, layout, kind)
    monkeypatch.delenv(KNOB, raising=False)
    assert ext.attn_mfma_path(lq, lk, d) == "smallq"
    new = _run(a, p, seed_dev=seed_dev)
    monkeypatch.setenv(KNOB, "0")
    assert ext.attn_mfma_path(lq, lk, d) == "tile64"
    old = _run(a, p, seed_dev=seed_dev)
    assert old["p_saved"].shape == (b, h, lq, lk)
    assert torch.isfinite(old["out"].float()).all()
    if p > 0:
        assert old["keep"].shape == (b, h, lq, lk)
    for name in OUTPUTS:
        assert new[name].shape == old[name].shape, name
        assert new[name].dtype == old[name].dtype, name
        assert torch.equal(new[name], old[name]), (
            name, (new[name].float() - old[name].float()).abs().max().item())


@pytest.mark.parametrize("p", [0.3, 0.0], ids=["drop", "nodrop"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", ["contig", "chunk"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_smallq_equals_tile64(monkeypatch, shape, layout, kind, p):
    """B*H = 6 heads: three full workgroups of two heads"""
    _parity(monkeypatch, 3, 2, shape, layout, kind, p)


@pytest.mark.parametrize("kind", ["bias4d", "bias_bf16"])
@pytest.mark.parametrize("shape", [(4, 4, 64), (4, 61, 64), (3, 17, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_smallq_bias_forms(monkeypatch, shape, kind):
    """[B,H,Lq,Lk] bias (per-element bias gradient) and bf16 bias"""
    _parity(monkeypatch, 3, 2, shape, "chunk", kind, 0.3)


@pytest.mark.parametrize("shape", [(4, 61, 64), (1, 1, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_smallq_partial_workgroup(monkeypatch, shape):
    """one head: the second wave of the only workgroup has no head"""
    _parity(monkeypatch, 1, 1, shape, "contig", "bias_pad", 0.3)
    _parity(monkeypatch, 1, 3, shape, "chunk", "causal_qmask", 0.3)


def test_smallq_seed_dev(monkeypatch):
    """the device-side seed offset reaches the dropout hash of both paths,
    and changes the mask"""
    seed_dev = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    _parity(monkeypatch, 3, 2, (4, 61, 64), "chunk", "bias_pad", 0.3,
            seed_dev=seed_dev)
    monkeypatch.delenv(KNOB, raising=False)
    a = _inputs(3, 2, 4, 61, 64, "chunk", "bias_pad")
    assert not torch.equal(_run(a, 0.3, seed_dev=seed_dev)["keep"],
                           _run(a, 0.3)["keep"])


def test_dispatch(monkeypatch):
    ext = _ext()
    monkeypatch.delenv(KNOB, raising=False)
    for lq, lk, d in SHAPES:
        assert ext.attn_mfma_path(lq, lk, d, 0, False) == "smallq"
    assert ext.attn_mfma_path(17, 61, 64, 0, False) == "tile64"
    assert ext.attn_mfma_path(4, 61, 64, 1, False) == "tile64"   # SiLU
    assert ext.attn_mfma_path(4, 61, 64, 0, True) == "tile64"    # table mode
    # the backward takes the small-query kernel up to one key strip only
    for lq, lk, d in SHAPES:
        want = "smallq" if lk <= 16 else "tile64"
        assert ext.attn_mfma_path(lq, lk, d, backward=True) == want
    assert ext.attn_mfma_path(17, 4, 64, backward=True) == "tile64"
    monkeypatch.setenv(KNOB, "0")
    for lq, lk, d in SHAPES:
        assert ext.attn_mfma_path(lq, lk, d, 0, False) == "tile64"
        assert ext.attn_mfma_path(lq, lk, d, backward=True) == "tile64"
    monkeypatch.setenv(KNOB, "1")
    assert ext.attn_mfma_path(4, 4, 64) == "smallq"
