"""Fused cross-attention K/V projection on the GPU.

attn_bwd_mfma's dkv_out mode writes dK/dV into two column blocks of a
[B, Lk, W] buffer that several calls share; ops.project_cross_kv and
ops.cross_attention_kv build the decoder's cross attention on it (one
K/V projection GEMM trio per step instead of one per layer, no gradient
accumulation on the encoder memory).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, D = 2, 64
HD = H * D
KNOB = "GENREC_DISABLE_CROSS_KV_FUSE"


def _ext():
    from genrec_amd import ops

    return ops.ext()


def _blocks(t, n_blocks, i):
    """[B,H,L,D] view of column block i of a [B,L,n_blocks*H*D] tensor"""
    b, l, _ = t.shape
    return t.view(b, l, n_blocks, H, D)[:, :, i].transpose(1, 2)


# Lq <= 16 with Lk <= 16 runs attn_bwd_smallq_kernel, everything else
# attn_bwd_ds_kernel; 5, 17 and 61 leave a ragged last strip
@pytest.mark.parametrize("lk", [5, 16, 17, 61, 64])
@pytest.mark.parametrize("lq", [4, 16, 17])
def test_dkv_out_holds_what_the_separate_call_returns(lq, lk):
    ext = _ext()
    g = torch.Generator(device=DEV).manual_seed(lq * 100 + lk)
    scale, seed = 0.125, 4321
    # (n_blocks, dk block, dv block): first, middle and last pairs, and a
    # pair that is neither adjacent nor ordered
    places = [(2, 0, 1), (8, 0, 1), (8, 4, 5), (8, 6, 7), (8, 5, 2)]
    for b in (2, 3):
        pad = torch.zeros(b, lk, dtype=torch.bool, device=DEV)
        pad[1, (3 * lk) // 4:] = True           # a row with a padded tail
        for p in (0.0, 0.1):
            for n_blocks, ik, iv in places:
                w = n_blocks * HD
                kv = torch.randn(b, lk, w, device=DEV, generator=g).bfloat16()
                q = torch.randn(b, lq, H, D, device=DEV, generator=g) \
                    .bfloat16().transpose(1, 2)
                dout = torch.randn(b, lq, H, D, device=DEV, generator=g) \
                    .bfloat16().transpose(1, 2)
                kp, vp = _blocks(kv, n_blocks, ik), _blocks(kv, n_blocks, iv)
                k, v = kp.contiguous(), vp.contiguous()
                out, probs, keep = ext.attn_fwd_mfma(
                    q, k, v, None, pad, None, None, scale, False, 0, p, seed,
                    None)
                out2, probs2, keep2 = ext.attn_fwd_mfma(
                    q, kp, vp, None, pad, None, None, scale, False, 0, p,
                    seed, None)
                assert torch.equal(out2, out) and torch.equal(probs2, probs)
                assert torch.equal(keep2, keep)
                dq, dk, dv, _ = ext.attn_bwd_mfma(
                    dout, q, k, v, probs, keep, None, scale, 0, p, seed,
                    False, 0)
                dkv = torch.full((b, lk, w), float("nan"), device=DEV,
                                 dtype=torch.bfloat16)
                dq2, dk2, dv2, _ = ext.attn_bwd_mfma(
                    dout, q, kp, vp, probs, keep, None, scale, 0, p, seed,
                    False, 0, None, 0, None, dkv, ik * HD, iv * HD)
                tag = (b, p, n_blocks, ik, iv)
                assert torch.isfinite(dq.float()).all(), tag
                assert torch.equal(dq2, dq), tag
                got_k, got_v = _blocks(dkv, n_blocks, ik), \
                    _blocks(dkv, n_blocks, iv)
                # padded keys' rows included
                assert torch.isfinite(got_k.float()).all(), tag
                assert torch.isfinite(got_v.float()).all(), tag
                assert torch.equal(got_k, dk) and torch.equal(got_v, dv), tag
                assert torch.equal(dk2, dk) and torch.equal(dv2, dv), tag
                assert dk2.untyped_storage().data_ptr() == \
                    dkv.untyped_storage().data_ptr()
                rest = [i for i in range(n_blocks) if i not in (ik, iv)]
                if rest:
                    others = dkv.view(b, lk, n_blocks, HD)[:, :, rest]
                    assert torch.isnan(others).all(), tag


def test_dkv_out_is_checked():
    ext = _ext()
    b, lq, lk = 2, 4, 8
    q = torch.randn(b, H, lq, D, device=DEV).bfloat16()
    k = torch.randn(b, H, lk, D, device=DEV).bfloat16()
    out, probs, keep = ext.attn_fwd_mfma(q, k, k, None, None, None, None,
                                         0.125, False, 0, 0.0, 0, None)
    w = 4 * HD
    buf = torch.zeros(b, lk, w, device=DEV, dtype=torch.bfloat16)

    def call(dkv, ck, cv, dqkv=None):
        return ext.attn_bwd_mfma(out, q, k, k, probs, keep, None, 0.125, 0,
                                 0.0, 0, False, 0, None, 0, dqkv, dkv, ck, cv)

    call(buf, 0, HD)                                       # the valid form
    with pytest.raises(RuntimeError, match="bf16"):
        call(buf.float(), 0, HD)
    wide = torch.zeros(b, lk, 2 * w, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(wide[:, :, :w], 0, HD)
    with pytest.raises(RuntimeError, match="dk_col/dv_col"):
        call(buf, w, 0)                                    # out of range
    with pytest.raises(RuntimeError, match="dk_col/dv_col"):
        call(buf, 0, -HD)
    with pytest.raises(RuntimeError, match="dk_col/dv_col"):
        call(buf, 0, HD + 8)                               # not a block
    with pytest.raises(RuntimeError, match="dk_col/dv_col"):
        call(buf, HD, HD)                                  # same block
    with pytest.raises(RuntimeError, match=r"\[B, Lk, n_blocks\*H\*D\]"):
        call(buf[:, :lk - 1].contiguous(), 0, HD)          # wrong Lk
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        call(buf, 0, HD,
             dqkv=torch.zeros(b, lq, 3 * HD, device=DEV,
                              dtype=torch.bfloat16))
    assert torch.isfinite(buf.float()).all()


def _decoder(n_layers, dropout, dtype):
    from genrec_amd.modules.transformer import TransformerDecoder

    torch.manual_seed(5)
    dec = TransformerDecoder(HD, n_layers, H, dropout=dropout,
                             ff_hidden_dim=256).to(DEV).bfloat16()
    if dtype != torch.bfloat16:
        dec = dec.to(dtype)       # the bf16 weights, widened
    return dec.train()


def _data(b, lq, lk, dtype):
    g = torch.Generator(device=DEV).manual_seed(9)
    tgt = torch.randn(b, lq, HD, device=DEV, generator=g).bfloat16()
    mem = torch.randn(b, lk, HD, device=DEV, generator=g).bfloat16()
    pad = torch.zeros(b, lk, dtype=torch.bool, device=DEV)
    pad[1, (3 * lk) // 4:] = True
    return tgt.to(dtype), mem.to(dtype), pad


def _step(dec, tgt0, mem0, pad):
    dec.zero_grad(set_to_none=True)
    tgt, mem = tgt0.clone().requires_grad_(), mem0.clone().requires_grad_()
    out = dec(tgt, memory=mem, memory_key_padding_mask=pad)
    wgt = torch.linspace(-1.0, 1.0, out.numel(), device=DEV) \
        .view_as(out).to(out.dtype)
    (out * wgt).float().sum().backward()
    torch.cuda.synchronize()
    res = dict(out=out.detach(), d_memory=mem.grad, d_tgt=tgt.grad)
    for name, p in dec.named_parameters():
        res["d_" + name] = p.grad
    return res


def _rel(x, ref):
    return ((x.double() - ref.double()).norm() / ref.double().norm()).item()


# (3, 4, 61): the bench's decoder shape, plain weight-gradient GEMM;
# (160, 17, 64): 10,240 memory rows, the split-K weight gradient, and the
# 64-row backward kernel on the query side
@pytest.mark.parametrize("shape", [(3, 4, 61), (160, 17, 64)],
                         ids=lambda s: "x".join(map(str, s)))
def test_decoder_fused_is_as_close_to_fp32_as_per_layer(monkeypatch, shape):
    """Relative Frobenius error of each bf16 route against the fp32 module
    on the same (bf16-valued) weights, for the output and every gradient:
    the fused route's may be at most 1.5x the per-layer route's (another
    GEMM tiling moves single bf16 roundings, not the aggregate), and
    d_memory's not higher."""
    from genrec_amd import ops

    b, lq, lk = shape
    dec = _decoder(2, 0.0, torch.bfloat16)
    ref_dec = _decoder(2, 0.0, torch.float32)
    for p, r in zip(dec.parameters(), ref_dec.parameters()):
        assert torch.equal(p.float(), r)
    tgt, mem, pad = _data(b, lq, lk, torch.bfloat16)
    attns = [layer.cross_attn for layer in dec.layers]
    args = (mem, tgt, [a.k.weight for a in attns],
            [a.v.weight for a in attns], [None] * 4, H)

    monkeypatch.delenv(KNOB, raising=False)
    assert ops.cross_kv_eligible(*args)
    fused = _step(dec, tgt, mem, pad)
    kv_grads = [getattr(a, w).weight.grad for a in attns for w in "kv"]
    # the parameters' gradients are the row slices of one tensor, as they
    # came out of the one weight-gradient GEMM: no copy per parameter
    assert len({g.untyped_storage().data_ptr() for g in kv_grads}) == 1
    monkeypatch.setenv(KNOB, "1")
    assert not ops.cross_kv_eligible(*args)
    per_layer = _step(dec, tgt, mem, pad)
    kv_grads = [getattr(a, w).weight.grad for a in attns for w in "kv"]
    assert len({g.untyped_storage().data_ptr() for g in kv_grads}) == 4
    monkeypatch.delenv(KNOB)
    ref = _step(ref_dec, *_data(b, lq, lk, torch.float32))

    assert set(fused) == set(per_layer) == set(ref)
    for name in ref:
        assert torch.isfinite(fused[name].float()).all(), name
        e_f, e_p = _rel(fused[name], ref[name]), _rel(per_layer[name],
                                                      ref[name])
        print(f"{name}: fused {e_f:.3e} per-layer {e_p:.3e}")
        assert e_f <= 1.5 * e_p, (name, e_f, e_p)
    assert _rel(fused["d_memory"], ref["d_memory"]) <= \
        _rel(per_layer["d_memory"], ref["d_memory"])
    # d_memory is summed block by block in autograd's order with its
    # roundings: the per-layer route's bits, like the output's and d_tgt's
    for name in ("out", "d_memory", "d_tgt"):
        assert torch.equal(fused[name], per_layer[name]), name


def test_knobs_route_away(monkeypatch):
    from genrec_amd import ops
    from genrec_amd.ops.cross_kv import _ROUTING_KNOBS

    dec = _decoder(2, 0.0, torch.bfloat16)
    tgt, mem, pad = _data(2, 4, 5, torch.bfloat16)
    attns = [layer.cross_attn for layer in dec.layers]
    args = (mem, tgt, [a.k.weight for a in attns],
            [a.v.weight for a in attns], [None] * 4, H)
    for knob in _ROUTING_KNOBS:
        monkeypatch.delenv(knob, raising=False)
    assert ops.cross_kv_eligible(*args)
    assert not ops.cross_kv_eligible(*args, kv_caches=[{}, {}])
    for knob in _ROUTING_KNOBS:
        monkeypatch.setenv(knob, "1")
        assert not ops.cross_kv_eligible(*args), knob
        monkeypatch.delenv(knob)


def test_captured_step_replays_alike(monkeypatch):
    """forward + backward with dropout 0.1 under torch.cuda.graph: the
    shared gradient buffer's host-side state is rebuilt by every forward,
    so warm-up iterations, the capture and the replays all start clean"""
    monkeypatch.delenv(KNOB, raising=False)
    dec = _decoder(2, 0.1, torch.bfloat16)
    tgt0, mem0, pad = _data(3, 4, 61, torch.bfloat16)
    tgt, mem = tgt0.clone().requires_grad_(), mem0.clone().requires_grad_()
    wgt = torch.linspace(-1.0, 1.0, tgt.numel(), device=DEV) \
        .view_as(tgt).bfloat16()

    def step():
        dec.zero_grad(set_to_none=True)
        tgt.grad = mem.grad = None
        out = dec(tgt, memory=mem, memory_key_padding_mask=pad)
        (out * wgt).float().sum().backward()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()

    def grads():
        torch.cuda.synchronize()
        got = {"d_memory": mem.grad.clone(), "d_tgt": tgt.grad.clone()}
        for name, p in dec.named_parameters():
            got[name] = p.grad.clone()
        return got

    graph.replay()
    first = grads()
    graph.replay()
    second = grads()
    for name in first:
        assert torch.isfinite(first[name].float()).all(), name
        assert torch.equal(first[name], second[name]), name
    assert first["d_memory"].abs().max() > 0


def _count_ops(dec, tgt, mem, pad):
    """ATen calls of one forward + backward, by name and input shapes"""
    from torch.profiler import ProfilerActivity, profile

    _step(dec, tgt, mem, pad)      # warm up outside the profile
    with profile(activities=[ProfilerActivity.CPU], record_shapes=True) as pr:
        _step(dec, tgt, mem, pad)
    return [(e.name, [tuple(s) if isinstance(s, (list, tuple)) else s
                      for s in e.input_shapes]) for e in pr.events()]


def test_one_projection_gemm_trio_and_no_accumulation(monkeypatch):
    """4-layer decoder: the fused route issues one GEMM with the memory's
    B*Lk rows in each of the three roles (forward, input gradient — a
    batched one, a batch per column block —, weight gradient) and autograd
    adds nothing of the memory's shape; the same
    count on the per-layer route finds 8 of each and the 7 adds."""
    b, lq, lk, n = 3, 4, 61, 4
    rows, width = b * lk, 2 * n * HD
    dec = _decoder(n, 0.0, torch.bfloat16)
    tgt, mem, pad = _data(b, lq, lk, torch.bfloat16)

    def tally(events):
        fwd = dx = dw = adds = 0
        for name, shapes in events:
            if name in ("aten::mm", "aten::bmm"):
                a, c = shapes[0], shapes[1]
                if name == "aten::bmm":
                    # the fused input gradient: one batched GEMM, a batch
                    # per column block (split-K needs 8192 rows: no other
                    # bmm touches the memory at this size)
                    if tuple(a) == (2 * n, rows, HD):
                        dx += 1
                    continue
                if a[0] == rows and a[1] == HD:
                    fwd += 1                     # [rows,d] x [d,N]
                elif a[0] == rows and c[1] == HD:
                    dx += 1                      # [rows,N] x [N,d]
                elif a[1] == rows and c[0] == rows:
                    dw += 1                      # [N,rows] x [rows,d]
            elif name in ("aten::add", "aten::add_") and shapes \
                    and shapes[0] == (b, lk, HD):
                adds += 1
        return fwd, dx, dw, adds

    monkeypatch.delenv(KNOB, raising=False)
    events = _count_ops(dec, tgt, mem, pad)
    assert tally(events) == (1, 1, 1, 0)
    wide = [s for name, s in events if name == "aten::mm"
            and width in (s[0][0], s[0][1], s[1][1])]
    assert len(wide) == 2          # forward and weight gradient: all layers
    monkeypatch.setenv(KNOB, "1")
    # (a per-layer projection is d -> d: its forward and its input
    # gradient have the same shapes and both count as "forward")
    assert tally(_count_ops(dec, tgt, mem, pad)) == (4 * n, 0, 2 * n,
                                                     2 * n - 1)


@pytest.mark.parametrize("shape", [(8, 15616 * 4), (1, 64), (3, 1028)],
                         ids=lambda s: "x".join(map(str, s)))
def test_seq_sum_is_a_chain_of_bf16_adds(shape):
    """seq_sum_bf16 gives the bits of acc = acc + row, row after row, in
    either order; more than one block, a single row, a ragged grid"""
    ext = _ext()
    rows, cols = shape
    g = torch.Generator(device=DEV).manual_seed(rows + cols)
    x = (torch.randn(rows, cols, device=DEV, generator=g) * 3).bfloat16()
    for reverse in (False, True):
        order = list(range(rows))[::-1] if reverse else list(range(rows))
        want = x[order[0]].clone()
        for r in order[1:]:
            want = want + x[r]
        assert torch.equal(ext.seq_sum_bf16(x, reverse), want)
    with pytest.raises(RuntimeError, match="seq_sum_bf16"):
        ext.seq_sum_bf16(x[:, :cols - 1].contiguous(), False)
    with pytest.raises(RuntimeError, match="seq_sum_bf16"):
        ext.seq_sum_bf16(x.float(), False)
