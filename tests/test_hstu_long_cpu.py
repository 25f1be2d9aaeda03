"""Long-sequence HSTU attention without a GPU: the Toeplitz bucket vector,
eager.hstu_attention (the fp32 reference and CPU path) against the
bias-tensor composition, and the model beyond one 64-row tile.

hstu_long_case and emulate_kernel are shared with test_hstu_long_gpu.py:
the kernel tests there run on the cases whose bounds are checked here.
"""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

N_POS, N_TIME = 32, 64
LEFT_PAD = 40     # item 0: the first 40 keys are pad (a left-padded history)
TAIL_PAD = 7      # item 1: the last 7 keys are pad


def left_pad(L):
    """40 at L = 130; a third of the sequence where that is shorter"""
    return min(LEFT_PAD, L // 3)


def _module_rel(L):
    from genrec_amd.models.hstu import RelativePositionBias

    return RelativePositionBias(N_POS, 128, 2).rel_bucket_table(L, "cpu")


def custom_rel(L):
    """min(|j - i|, 15), plus 16 for j > i. The module's table is 0 over the
    whole causal half and cannot tell a wrong sign or offset apart; this one
    differs from diagonal to diagonal and between the two signs."""
    rel = torch.arange(-(L - 1), L)
    half = N_POS // 2
    return (rel.abs().clamp(max=half - 1) + half * (rel > 0)).to(torch.int32)


def _materialise(rel, L):
    pos = torch.arange(L, device=rel.device)
    return rel.long()[pos[None, :] - pos[:, None] + (L - 1)]  # [i, j]


@functools.lru_cache(maxsize=None)
def hstu_long_case(L, D, use_time, custom, B=2, H=2):
    """bf16 inputs on the CPU. Input scale 0.5 as in the one-tile kernel's
    tests; timestamps are spaced multiples (test_timestamps_off_boundaries
    checks that no pair sits on a bucket boundary).

    The seed is one at which the fp32 bias-tensor composition is itself
    within allclose(1e-5, 1e-5) of the same computation in fp64. Its table
    gradients are fp32 running sums of up to 2*130*130 terms, which at some
    seeds miss that bound on their own; eager.hstu_attention sums them in
    fp64 and does not."""
    g = torch.Generator().manual_seed(35)

    def rnd(*shape):
        return torch.randn(*shape, generator=g)

    q, k, v = ((rnd(B, H, L, D) * 0.5).to(torch.bfloat16) for _ in range(3))
    pos_w = (rnd(N_POS, H) * 0.5).to(torch.bfloat16)
    time_w = (rnd(N_TIME, H) * 0.5).to(torch.bfloat16) if use_time else None
    rel = custom_rel(L) if custom else _module_rel(L)
    ts = (torch.arange(L) * 3600 + 10 ** 9).unsqueeze(0).expand(B, -1) \
        .contiguous() if use_time else None
    pad = torch.zeros(B, L, dtype=torch.bool)
    pad[0, :left_pad(L)] = True
    pad[1, L - TAIL_PAD:] = True
    dout = rnd(B, H, L, D).to(torch.bfloat16)
    return dict(q=q, k=k, v=v, pos_w=pos_w, time_w=time_w, rel=rel, ts=ts,
                pad=pad, dout=dout)


def reference(case, device="cpu", block=48):
    """eager.hstu_attention on the bf16 inputs upcast to fp32 -> out and the
    gradients of q, k, v, pos_w (, time_w), all fp32."""
    from genrec_amd.ops import eager

    leaves = [case[n].to(device).float().requires_grad_(True)
              for n in ("q", "k", "v", "pos_w")]
    if case["time_w"] is not None:
        leaves.append(case["time_w"].to(device).float().requires_grad_(True))
    ts = case["ts"].to(device) if case["ts"] is not None else None
    out = eager.hstu_attention(
        leaves[0], leaves[1], leaves[2], case["rel"].to(device), leaves[3],
        leaves[4] if len(leaves) == 5 else None, ts,
        case["pad"].to(device), block=block)
    grads = torch.autograd.grad(out, leaves, case["dout"].to(device).float())
    return [out.detach()] + list(grads)


def composed(case):
    """hstu_pointwise_attention on the materialised [H,L,L] / [B,H,L,L]
    bias tensors, fp32 (the path of the parent of this op)."""
    from genrec_amd.ops.attention import hstu_pointwise_attention

    leaves = [case[n].float().requires_grad_(True)
              for n in ("q", "k", "v", "pos_w")]
    L = leaves[0].size(2)
    pos_bias = F.embedding(_materialise(case["rel"], L), leaves[3]) \
        .permute(2, 0, 1)
    time_bias = None
    if case["time_w"] is not None:
        leaves.append(case["time_w"].float().requires_grad_(True))
        ts = case["ts"]
        diff = ts.unsqueeze(2) - ts.unsqueeze(1)
        tb = (torch.log(diff.abs().clamp(min=1).float()) / 0.693).long() \
            .clamp(min=0, max=N_TIME - 1)
        time_bias = F.embedding(tb, leaves[4]).permute(0, 3, 1, 2)
    out = hstu_pointwise_attention(leaves[0], leaves[1], leaves[2], pos_bias,
                                   time_bias, case["pad"])
    grads = torch.autograd.grad(out, leaves, case["dout"].float())
    return [out.detach()] + list(grads)


def emulate_kernel(case):
    """The tiled kernel's arithmetic on the CPU: bf16 operands, fp32
    accumulation, P / A and dS rounded to bf16 before their products, bias
    gradients summed from the unrounded dS, bf16 outputs."""
    bf = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    q, k, v, dout = (case[n].float() for n in ("q", "k", "v", "dout"))
    L = q.size(2)
    bucket = _materialise(case["rel"], L)
    s = q @ k.transpose(-2, -1) + case["pos_w"].float()[bucket] \
        .permute(2, 0, 1)
    tb = None
    if case["time_w"] is not None:
        ts = case["ts"]
        diff = ts.unsqueeze(2) - ts.unsqueeze(1)
        tb = (torch.log(diff.abs().clamp(min=1).float()) / 0.693).long() \
            .clamp(min=0, max=N_TIME - 1)
        s = s + case["time_w"].float()[tb].permute(0, 3, 1, 2)
    pos = torch.arange(L)
    masked = (pos[None, :] > pos[:, None])[None, None] \
        | case["pad"][:, None, None, :]
    s = s.masked_fill(masked, -1e9)
    sg = torch.sigmoid(s)
    a = bf(s * sg)
    out = bf(a @ v)
    ds = (dout @ v.transpose(-2, -1)) * sg * (1 + s * (1 - sg))
    dsb = bf(ds)
    res = [out, bf(dsb @ k), bf(dsb.transpose(-2, -1) @ q),
           bf(a.transpose(-2, -1) @ dout)]
    H = q.size(1)
    dpos = torch.zeros(N_POS, H)
    for h in range(H):
        dpos[:, h].index_add_(0, bucket.reshape(-1),
                              ds[:, h].sum(0).reshape(-1))
    res.append(bf(dpos))
    if tb is not None:
        dtime = torch.zeros(N_TIME, H)
        for h in range(H):
            dtime[:, h].index_add_(0, tb.reshape(-1), ds[:, h].reshape(-1))
        res.append(bf(dtime))
    return res


def rel_err_ok(a, b, rel=0.08, eps=1.0, frac=0.999):
    """test_kernels_gpu._rel_err_ok: |a-b| / (|b|+eps) <= rel for at least
    frac of the elements."""
    r = (a.float() - b.float()).abs() / (b.float().abs() + eps)
    got = (r <= rel).float().mean().item()
    assert got >= frac, f"only {got:.4f} of elements within rel {rel}"


def within_hstu_bounds(got, ref):
    """the project's HSTU bounds, on out and every gradient"""
    for a, b in zip(got, ref):
        a, b = a.float().cpu(), b.float().cpu()
        assert torch.allclose(a, b, atol=0.5, rtol=0.1), (a - b).abs().max()
        rel_err_ok(a, b)


# ------------------------------------------------------------------- tests


@pytest.mark.parametrize("L", [1, 33, 64, 130])
def test_rel_bucket_is_the_toeplitz_vector_of_bucket_table(L):
    from genrec_amd.models.hstu import RelativePositionBias

    m = RelativePositionBias(N_POS, 128, 2)
    rel = m.rel_bucket_table(L, "cpu")
    assert rel.dtype == torch.int32 and rel.shape == (2 * L - 1,)
    assert torch.equal(_materialise(rel, L), m.bucket_table(L, "cpu"))
    assert m.rel_bucket_table(L, "cpu") is rel  # cached


@pytest.mark.parametrize("use_time", [False, True])
def test_eager_matches_composed(use_time):
    """forward and the gradients of q, k, v, pos_weight (, time_weight) at
    L=130 with ragged row blocks (block=48): both sides fp32, one formula"""
    case = hstu_long_case(130, 32, use_time, False)
    for a, b in zip(reference(case), composed(case)):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5), (a - b).abs().max()


@pytest.mark.parametrize("use_time", [False, True])
def test_eager_sign_and_offset_custom_table(use_time):
    """a rel_bucket that differs on every diagonal, against the
    materialised [L,L] gather of the same table"""
    case = hstu_long_case(130, 32, use_time, True)
    got, ref = reference(case), composed(case)
    for a, b in zip(got, ref):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5), (a - b).abs().max()
    # the check has teeth: the table read with the wrong sign, or one
    # entry off, gives another result
    for wrong in (case["rel"].flip(0), case["rel"].roll(1)):
        assert not torch.allclose(reference(dict(case, rel=wrong))[0],
                                  ref[0], atol=1e-3)


def test_eager_blocks_and_no_grad_agree():
    from genrec_amd.ops import eager

    case = hstu_long_case(130, 32, True, True)
    args = [case[n].float() for n in ("q", "k", "v")] + [
        case["rel"], case["pos_w"].float(), case["time_w"].float(),
        case["ts"], case["pad"]]
    with torch.no_grad():
        whole = eager.hstu_attention(*args, block=130)
        ragged = eager.hstu_attention(*args, block=48)
    assert torch.allclose(whole, ragged, rtol=1e-5, atol=1e-5)
    assert torch.allclose(whole, reference(case)[0], rtol=1e-5, atol=1e-5)
    # fully masked rows (item 0 is left-padded) are exactly zero
    assert (whole[0, :, :LEFT_PAD] == 0).all()
    with pytest.raises(ValueError):
        eager.hstu_attention(*args[:3], case["rel"][:-1], *args[4:])


def test_ops_hstu_attention_on_cpu_is_the_eager_op():
    from genrec_amd import ops

    case = hstu_long_case(130, 32, True, True)
    out = ops.hstu_attention(case["q"], case["k"], case["v"], case["rel"],
                             case["pos_w"], case["time_w"], case["ts"],
                             case["pad"])
    assert out.dtype == torch.bfloat16
    ref = reference(case)[0]
    assert torch.allclose(out.float(), ref, atol=0.05, rtol=0.02)


def test_timestamps_off_boundaries():
    """no |ts_i - ts_j| of the cases within 1e-3 relative of a difference at
    which ln(d)/0.693 is an integer: a float-log difference between device
    and host cannot move a pair into another bucket. That covers the
    kernel-against-eager cases (L <= 130). The L = 1024 memory test uses the
    same spacing and compares `out` only; over its differences the closest
    is 4.4e-4 (581 steps), asserted below at 1e-4, which is still a thousand
    times a float log's error."""
    def closest(n):
        d = torch.arange(1, n, dtype=torch.float64) * 3600
        boundary = torch.exp(0.693 * (torch.log(d) / 0.693).round())
        return (d / boundary - 1).abs().min()

    assert closest(130) > 1e-3, closest(130)
    assert closest(1024) > 1e-4, closest(1024)


@pytest.mark.parametrize("L,D,use_time,custom", [
    (65, 32, True, True), (65, 64, False, False),
    (130, 32, False, False), (130, 32, True, True),
    (130, 64, True, True), (130, 64, False, False),
])
def test_kernel_arithmetic_stays_inside_the_hstu_bounds(L, D, use_time,
                                                        custom):
    """The GPU tests hold the kernel to allclose(atol=0.5, rtol=0.1) and a
    0.1 % allowance at rel 0.08: the seed and the 0.5 input scale of
    hstu_long_case are such that the kernel's arithmetic alone (bf16 P and
    dS, fp32 accumulation, bf16 outputs) is inside both."""
    case = hstu_long_case(L, D, use_time, custom)
    within_hstu_bounds(emulate_kernel(case), reference(case))


def _model(max_seq_len, **kw):
    from genrec_amd.models.hstu import HSTU

    torch.manual_seed(5)
    return HSTU(num_items=200, max_seq_len=max_seq_len, embed_dim=16,
                num_heads=2, num_blocks=2, dropout=0.0, **kw)


def test_model_long_sequence_cpu(monkeypatch):
    """beyond 64 positions every layer goes through ops.hstu_attention,
    which off the GPU is eager.hstu_attention"""
    from genrec_amd import ops
    from genrec_amd.ops import eager

    calls = {"op": 0, "eager": 0}

    def spy(name, fn):
        def wrapped(*args, **kw):
            calls[name] += 1
            return fn(*args, **kw)
        return wrapped

    monkeypatch.setattr(ops, "hstu_attention", spy("op", ops.hstu_attention))
    monkeypatch.setattr(eager, "hstu_attention",
                        spy("eager", eager.hstu_attention))
    monkeypatch.setattr(
        ops, "hstu_pointwise_attention",
        lambda *a, **k: pytest.fail("bias tensors materialised at L = 130"))
    L = 130
    m = _model(L)
    m.train()
    ids = torch.randint(1, 201, (3, L))
    ids[0, :LEFT_PAD] = 0
    ts = (torch.arange(L) * 3600 + 10 ** 9).unsqueeze(0).expand(3, -1) \
        .contiguous()
    _, loss = m(ids, ts, ids)
    assert torch.isfinite(loss)
    assert calls == {"op": 2, "eager": 2}
    loss.backward()
    for layer in m.layers:
        for w in (layer.position_bias.relative_attention_bias.weight,
                  layer.temporal_bias.temporal_attention_bias.weight):
            assert w.grad is not None and torch.isfinite(w.grad).all()
            assert w.grad.abs().sum() > 0


def test_layer_at_shipped_length_is_the_composed_path():
    """max_seq_len = 50: bit-identical to the bias-tensor composition the
    layer ran before ops.hstu_attention existed"""
    from genrec_amd import ops
    from genrec_amd.models.hstu import HSTULayer

    torch.manual_seed(6)
    layer = HSTULayer(embed_dim=16, num_heads=2, dropout=0.0,
                      num_position_buckets=32, num_time_buckets=64,
                      max_position_distance=128, use_temporal_bias=True)
    layer.eval()
    b, l, d = 3, 50, 16
    x = torch.randn(b, l, d)
    pad = torch.zeros(b, l, dtype=torch.bool)
    pad[0, :10] = True
    ts = (torch.arange(l) * 86400 + 10 ** 9).unsqueeze(0).expand(b, -1) \
        .contiguous()
    with torch.no_grad():
        got = layer(x, pad, ts)

        u, v, q, k = F.silu(layer.projection(x)).chunk(4, dim=-1)
        q, k, v = (t.view(b, l, 2, d // 2).transpose(1, 2)
                   for t in (q, k, v))
        attn = ops.hstu_pointwise_attention(
            q, k, v, layer.position_bias(l, x.device),
            layer.temporal_bias(ts), pad)
        attn = attn.transpose(1, 2).reshape(b, l, d)
        h = ops.dropout_add(layer.attn_norm(attn) * u, x, 0.0, False)
        f = layer.ffn[3](F.silu(layer.ffn[0](layer.ffn_norm(h))))
        want = ops.dropout_add(f, h, 0.0, False)
    assert torch.equal(got, want)
    assert math.isfinite(got.sum().item())
