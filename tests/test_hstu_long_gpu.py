"""The tiled HSTU attention kernels (csrc/kernels/hstu_attn_flash.hip) and
ops.hstu_attention on the GPU.

The cases are test_hstu_long_cpu.hstu_long_case: bf16 inputs at scale 0.5
with a fixed seed, a left-padded item whose first rows see no key, an item
with a padded tail. The oracle is eager.hstu_attention on the same inputs
upcast to fp32. The bounds are the project's HSTU bounds, allclose(atol=0.5,
rtol=0.1) and at least 99.9 % of the elements within rel 0.08;
test_kernel_arithmetic_stays_inside_the_hstu_bounds (CPU) shows that an
emulation of the kernel's arithmetic (fp32 accumulation, P and dS rounded to
bf16 before their products, bf16 outputs) meets both on these cases, and
test_timestamps_off_boundaries that no timestamp pair sits where a float log
could change its bucket.
"""

import functools

import pytest
import torch

from test_hstu_long_cpu import (N_POS, N_TIME, TAIL_PAD, _materialise,
                                hstu_long_case, left_pad, reference,
                                within_hstu_bounds)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("q", "k", "v", "pos_w", "time_w")


@functools.lru_cache(maxsize=None)
def _reference(L, D, use_time, custom):
    """computed once per case, on the GPU, and never written to"""
    return tuple(reference(hstu_long_case(L, D, use_time, custom), DEV))


@functools.lru_cache(maxsize=None)
def _gpu_case(L, D, use_time, custom):
    """hstu_long_case on the device; the tests clone what they change"""
    case = hstu_long_case(L, D, use_time, custom)
    return {n: t.to(DEV) if t is not None else None for n, t in case.items()}


def _leaves(case):
    return [case[n].detach().clone().requires_grad_(True) for n in NAMES
            if case[n] is not None]


def _run_op(case, leaves=None):
    """ops.hstu_attention forward + backward -> [out, dq, dk, dv, dpos
    (, dtime)]"""
    from genrec_amd import ops

    leaves = leaves or _leaves(case)
    out = ops.hstu_attention(
        leaves[0], leaves[1], leaves[2], case["rel"], leaves[3],
        leaves[4] if len(leaves) == 5 else None, case["ts"],
        case["pad"])
    grads = torch.autograd.grad(out, leaves, case["dout"])
    return [out.detach()] + list(grads)


def _flash_args(case, q=None, k=None, v=None):
    """arguments of the extension's entry points after q, k, v"""
    return (q if q is not None else case["q"],
            k if k is not None else case["k"],
            v if v is not None else case["v"],
            case["rel"], case["pos_w"],
            case["time_w"], case["ts"],
            case["pad"])


@pytest.mark.parametrize("custom", [False, True])
@pytest.mark.parametrize("use_time", [False, True])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("L", [65, 130])
def test_kernel_vs_eager(L, D, use_time, custom):
    """L=65: the second tile is one row. L=130: diagonal tiles, a full
    off-diagonal tile, skipped tiles, a two-row ragged tile."""
    from genrec_amd import ops

    case = _gpu_case(L, D, use_time, custom)
    leaves = _leaves(case)
    assert ops.hstu_flash_supported(*leaves[:4], case["time_w"])
    got = _run_op(case, leaves)
    within_hstu_bounds(got, _reference(L, D, use_time, custom))
    out, dq, dk, dv = got[:4]
    n = left_pad(L)
    # item 0, rows below n: every key is pad or ahead -> exactly 0, and no
    # gradient reaches those queries or comes from those keys
    assert (out[0, :, :n] == 0).all() and (dq[0, :, :n] == 0).all()
    assert (dk[0, :, :n] == 0).all() and (dv[0, :, :n] == 0).all()
    assert (dk[1, :, L - TAIL_PAD:] == 0).all()
    assert (dv[1, :, L - TAIL_PAD:] == 0).all()
    assert all(torch.isfinite(t).all() for t in got)


def test_strided_views_are_read_in_place():
    """q/k/v as the layer makes them: chunk views of one [B,L,4*H*D]
    projection, head-split and transposed"""
    from genrec_amd import ops

    case = _gpu_case(130, 32, True, True)
    B, H, L, D = case["q"].shape
    torch.manual_seed(3)
    proj = (torch.randn(B, L, 4 * H * D, device=DEV) * 0.5).bfloat16()
    _, v, q, k = (t.view(B, L, H, D).transpose(1, 2)
                  for t in proj.chunk(4, dim=-1))
    assert not q.is_contiguous()
    ext = ops.ext()
    out = ext.hstu_attn_flash_fwd(*_flash_args(case, q, k, v))
    out_c = ext.hstu_attn_flash_fwd(*_flash_args(
        case, q.contiguous(), k.contiguous(), v.contiguous()))
    assert out.shape == (B, H, L, D)
    assert out.transpose(1, 2).is_contiguous()
    assert torch.equal(out, out_c)
    # dout as the layer's transpose(1,2).reshape hands it back
    dout = case["dout"].transpose(1, 2).contiguous().transpose(1, 2)
    g = ext.hstu_attn_flash_bwd(dout, *_flash_args(case, q, k, v))
    g_c = ext.hstu_attn_flash_bwd(dout.contiguous(), *_flash_args(
        case, q.contiguous(), k.contiguous(), v.contiguous()))
    # dk / dv are summed in registers in a fixed order; dq goes through
    # fp32 atomics and is not claimed bit-stable
    assert torch.equal(g[1], g_c[1]) and torch.equal(g[2], g_c[2])
    assert torch.allclose(g[0].float(), g_c[0].float(), atol=1e-2, rtol=1e-2)


def test_causality():
    from genrec_amd import ops

    case = _gpu_case(130, 32, True, True)
    ext = ops.ext()
    q, k, v = (case[n] for n in ("q", "k", "v"))
    out = ext.hstu_attn_flash_fwd(*_flash_args(case))
    k2, v2 = k.clone(), v.clone()
    k2[:, :, 70:] += 1.0
    v2[:, :, 70:] -= 2.0
    out2 = ext.hstu_attn_flash_fwd(*_flash_args(case, q, k2, v2))
    assert torch.equal(out[:, :, :70], out2[:, :, :70])
    assert not torch.equal(out[:, :, 70:], out2[:, :, 70:])

    dout = case["dout"]
    g = ext.hstu_attn_flash_bwd(dout, *_flash_args(case))
    dout2 = dout.clone()
    dout2[:, :, :64] *= -3.0
    g2 = ext.hstu_attn_flash_bwd(dout2, *_flash_args(case))
    assert torch.equal(g[1][:, :, 64:], g2[1][:, :, 64:])   # dk
    assert torch.equal(g[2][:, :, 64:], g2[2][:, :, 64:])   # dv
    assert not torch.equal(g[1][:, :, :64], g2[1][:, :, :64])


def _within_one_bf16_ulp(a, b):
    a, b = a.float(), b.float()
    mag = torch.maximum(a.abs(), b.abs()).clamp(min=2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    assert ((a - b).abs() <= ulp).all(), ((a - b).abs() / ulp).max()


@pytest.mark.parametrize("L", [33, 64])
@pytest.mark.parametrize("use_time", [False, True])
def test_continuity_with_the_one_tile_kernel(L, use_time):
    """the tiled kernel called at L <= 64 against hstu_attn_fwd / _bwd:
    same strip steps in the same order, so the same bits are expected"""
    from genrec_amd import ops

    case = _gpu_case(L, 32, use_time, True)
    ext = ops.ext()
    q, k, v, dout = (case[n] for n in ("q", "k", "v", "dout"))
    ts, pad = case["ts"], case["pad"]
    pb = _materialise(case["rel"], L)
    out1, s_saved = ext.hstu_attn_fwd(q, k, v, pb, case["pos_w"],
                                      case["time_w"], ts, pad)
    g1 = ext.hstu_attn_bwd(dout, q, k, v, s_saved, pb, ts, N_POS,
                           N_TIME if use_time else 0)
    out2 = ext.hstu_attn_flash_fwd(*_flash_args(case))
    g2 = ext.hstu_attn_flash_bwd(dout, *_flash_args(case))
    _within_one_bf16_ulp(out2, out1)
    for a, b in zip(g2[:3], g1[:3]):
        _within_one_bf16_ulp(a, b)
    assert torch.allclose(g2[3], g1[3], rtol=1e-3, atol=0)
    if use_time:
        assert torch.allclose(g2[4], g1[4], rtol=1e-3, atol=0)


def test_memory_is_linear_in_L():
    """B=1, H=2, L=1024, D=32: operands, outputs and the fp32 dQ buffer are
    under 2 MiB; one [B,H,L,L] fp32 tensor would be 8 MiB"""
    from genrec_amd import ops
    from genrec_amd.models.hstu import RelativePositionBias

    B, H, L, D = 1, 2, 1024, 32
    torch.manual_seed(11)
    q, k, v = ((torch.randn(B, H, L, D, device=DEV) * 0.5).bfloat16()
               .requires_grad_(True) for _ in range(3))
    pos_w = (torch.randn(N_POS, H, device=DEV) * 0.5).bfloat16() \
        .requires_grad_(True)
    time_w = (torch.randn(N_TIME, H, device=DEV) * 0.5).bfloat16() \
        .requires_grad_(True)
    rel = RelativePositionBias(N_POS, 128, H).rel_bucket_table(L, DEV)
    ts = (torch.arange(L, device=DEV) * 3600 + 10 ** 9).unsqueeze(0) \
        .contiguous()
    pad = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    pad[0, :100] = True
    dout = (torch.randn(B, H, L, D, device=DEV) * 0.1).bfloat16()
    with torch.no_grad():
        ref = ops.eager.hstu_attention(q.float(), k.float(), v.float(), rel,
                                       pos_w.float(), time_w.float(), ts, pad)
    ops.hstu_attention(q, k, v, rel, pos_w, time_w, ts, pad)  # warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.hstu_attention(q, k, v, rel, pos_w, time_w, ts, pad)
    out.backward(dout)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    assert grew < B * H * L * L * 4 // 2, grew
    within_hstu_bounds([out.detach()], [ref])
    assert all(torch.isfinite(t.grad).all() for t in (q, k, v, pos_w, time_w))


def test_model_long_sequence_and_dispatch(monkeypatch):
    """bf16 HSTU at max_seq_len=130 on left-padded data against the fp32
    model (bounds of test_hstu_fused_model_vs_fp32), through the tiled
    kernel unless GENREC_DISABLE_HSTU_FLASH=1"""
    from genrec_amd import ops
    from genrec_amd.models.hstu import HSTU

    monkeypatch.delenv("GENREC_DISABLE_HSTU_FLASH", raising=False)
    L = 130
    torch.manual_seed(21)
    m = HSTU(num_items=500, max_seq_len=L, embed_dim=64, num_heads=2,
             num_blocks=2, dropout=0.0, use_temporal_bias=True)
    ids = torch.randint(1, 501, (4, L))
    ids[0, :40] = 0
    ids[2, :100] = 0
    ts = (torch.arange(L) * 3600 + 10 ** 9).unsqueeze(0).expand(4, -1) \
        .contiguous()
    m.eval()
    with torch.no_grad():
        logits_ref, _ = m(ids, ts)
    m.train()
    _, loss_ref = m(ids, ts, ids)
    loss_ref.backward()
    grads_ref = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()

    ext = ops.ext()
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = ext.hstu_attn_flash_fwd, ext.hstu_attn_flash_bwd

    def count(name, fn):
        def wrapped(*args):
            calls[name] += 1
            return fn(*args)
        return wrapped

    monkeypatch.setattr(ext, "hstu_attn_flash_fwd", count("fwd", fwd))
    monkeypatch.setattr(ext, "hstu_attn_flash_bwd", count("bwd", bwd))

    mg = m.to(DEV).to(torch.bfloat16)
    idg, tsg = ids.to(DEV), ts.to(DEV)
    mg.eval()
    with torch.no_grad():
        logits, _ = mg(idg, tsg)
    assert calls == {"fwd": 2, "bwd": 0}
    within_hstu_bounds([logits], [logits_ref])
    mg.train()
    _, loss = mg(idg, tsg, idg)
    loss.backward()
    assert calls == {"fwd": 4, "bwd": 2}
    within_hstu_bounds([loss.detach().reshape(1)],
                       [loss_ref.detach().reshape(1)])
    for n, p in mg.named_parameters():
        assert p.grad is not None, n
        within_hstu_bounds([p.grad], [grads_ref[n]])
    for layer in mg.layers:
        for w in (layer.position_bias.relative_attention_bias.weight,
                  layer.temporal_bias.temporal_attention_bias.weight):
            assert torch.isfinite(w.grad).all() and w.grad.abs().sum() > 0

    monkeypatch.setenv("GENREC_DISABLE_HSTU_FLASH", "1")
    mg.eval()
    with torch.no_grad():
        logits_off, _ = mg(idg, tsg)
    assert calls == {"fwd": 4, "bwd": 2}
    within_hstu_bounds([logits_off], [logits_ref])


def test_autocast_model_with_fp32_parameters_takes_the_kernel(monkeypatch):
    """the trainers' configuration: fp32 parameters under bf16 autocast. q/k/v
    come out of the projection in bf16; the fp32 bias tables are rounded to
    bf16 for the kernel and get fp32 gradients"""
    from genrec_amd import ops
    from genrec_amd.models.hstu import HSTU

    monkeypatch.delenv("GENREC_DISABLE_HSTU_FLASH", raising=False)
    L = 130
    torch.manual_seed(22)
    m = HSTU(num_items=500, max_seq_len=L, embed_dim=64, num_heads=2,
             num_blocks=2, dropout=0.0, use_temporal_bias=True)
    m.train()
    ids = torch.randint(1, 501, (4, L))
    ids[0, :40] = 0
    ts = (torch.arange(L) * 3600 + 10 ** 9).unsqueeze(0).expand(4, -1) \
        .contiguous()
    _, loss_ref = m(ids, ts, ids)
    loss_ref.backward()
    grads_ref = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()

    ext = ops.ext()
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = ext.hstu_attn_flash_fwd, ext.hstu_attn_flash_bwd

    def fwd_spy(*args):
        calls["fwd"] += 1
        return fwd(*args)

    def bwd_spy(*args):
        calls["bwd"] += 1
        return bwd(*args)

    monkeypatch.setattr(ext, "hstu_attn_flash_fwd", fwd_spy)
    monkeypatch.setattr(ext, "hstu_attn_flash_bwd", bwd_spy)
    mg = m.to(DEV)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        _, loss = mg(ids.to(DEV), ts.to(DEV), ids.to(DEV))
    loss.backward()
    assert calls == {"fwd": 2, "bwd": 2}
    within_hstu_bounds([loss.detach().reshape(1)],
                       [loss_ref.detach().reshape(1)])
    for n, p in mg.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, n
        within_hstu_bounds([p.grad], [grads_ref[n]])
    for layer in mg.layers:
        for w in (layer.position_bias.relative_attention_bias.weight,
                  layer.temporal_bias.temporal_attention_bias.weight):
            assert torch.isfinite(w.grad).all() and w.grad.abs().sum() > 0


def test_inputs_on_another_device_are_moved():
    """rel_bucket, timestamps and the pad mask given on the CPU"""
    from genrec_amd import ops

    case = _gpu_case(130, 32, True, True)
    cpu = hstu_long_case(130, 32, True, True)
    args = [case[n] for n in ("q", "k", "v")]
    got = ops.hstu_attention(*args, cpu["rel"], case["pos_w"],
                             case["time_w"], cpu["ts"], cpu["pad"])
    want = ops.hstu_attention(*args, case["rel"], case["pos_w"],
                              case["time_w"], case["ts"], case["pad"])
    assert torch.equal(got, want)


def test_graph_capture_and_replay():
    """one forward + backward at L=130 under torch.cuda.graph, replayed
    twice: the hosts neither synchronise nor read a device value"""
    case = _gpu_case(130, 32, True, True)
    leaves = _leaves(case)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            _run_op(case, leaves)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _run_op(case, leaves)
    ref = _reference(130, 32, True, True)
    for _ in range(2):
        for t in got:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        within_hstu_bounds(got, ref)
