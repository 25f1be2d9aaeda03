"""Fused residual+dropout -> RMSNorm (csrc/kernels/norms.hip,
ops.dropout_add_rms_norm) against the composed dropout_add -> rms_norm
path, on the GPU.

The fused kernels are built to round where the composed kernels round, so
every comparison here is torch.equal, not a tolerance: h, n, the two input
gradients and dw.

A fp32 weight promotes the norm output to fp32, which the fused kernels do
not produce; the op then composes, and those cases check exactly that.
"""

import os
import subprocess
import sys

import pytest
import torch

from genrec_amd import ops
from genrec_amd.ops.attention import _seed_counter

pytestmark = pytest.mark.gpu

P = 0.1
EPS = 1e-6
# [5,384] fewer rows than one block's waves; [1024,384] decoder shape;
# [4099,384] past the backward's 1024 blocks x 4 waves, ragged tail;
# [4099,128] exactly one dword per lane; [67,130] lane tail inside a row;
# [1029,1024] widest row (8 dwords per lane); [32771,128] past the
# forward's 8192 blocks x 4 waves.
SHAPES = [(5, 384), (1024, 384), (4099, 384), (4099, 128), (67, 130),
          (1029, 1024), (32771, 128)]


def _dev():
    return torch.device("cuda:0")


def _inputs(rows, d, w_dtype, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g)
    y = mk(rows, d).to(_dev(), dtype).requires_grad_()
    res = (2.0 * mk(rows, d)).to(_dev(), dtype).requires_grad_()
    w = (1.0 + 0.25 * mk(d)).to(_dev(), w_dtype).requires_grad_()
    gh = mk(rows, d).to(_dev(), dtype)
    gn = mk(rows, d).to(_dev())
    return y, res, w, gh, gn


def _run(fused, y, res, w, gh, gn, t5, *, use_h=True, use_n=True, p=P,
         training=True, seed=7):
    """(h, n, dy, d_residual, dw) of one path; same seed -> same mask."""
    os.environ["GENREC_DISABLE_ADDNORM"] = "0" if fused else "1"
    try:
        torch.manual_seed(seed)
        h, n = ops.dropout_add_rms_norm(y, res, w, p, EPS, t5, training)
    finally:
        del os.environ["GENREC_DISABLE_ADDNORM"]
    outs, gouts = [], []
    if use_h:
        outs.append(h)
        gouts.append(gh)
    if use_n:
        outs.append(n)
        gouts.append(gn.to(n.dtype))
    dy, dres, dw = torch.autograd.grad(outs, (y, res, w), gouts,
                                       allow_unused=True)
    return h, n, dy, dres, dw


def _assert_same(a, b):
    for name, x, z in zip(("h", "n", "dy", "d_residual", "dw"), a, b):
        if x is None or z is None:
            assert x is None and z is None, name
        else:
            assert x.dtype == z.dtype and x.shape == z.shape, name
            assert torch.equal(x, z), name


def _count_kernel_calls(monkeypatch):
    calls = {"fwd": 0, "bwd": 0}
    ext = ops.ext()
    fwd, bwd = ext.dropout_add_rms_norm_fwd, ext.dropout_add_rms_norm_bwd

    def cfwd(*a):
        calls["fwd"] += 1
        return fwd(*a)

    def cbwd(*a):
        calls["bwd"] += 1
        return bwd(*a)

    monkeypatch.setattr(ext, "dropout_add_rms_norm_fwd", cfwd)
    monkeypatch.setattr(ext, "dropout_add_rms_norm_bwd", cbwd)
    return calls


@pytest.mark.parametrize("t5", [True, False])
@pytest.mark.parametrize("w_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,d", SHAPES)
def test_fused_equals_composed(rows, d, w_dtype, t5, monkeypatch):
    args = _inputs(rows, d, w_dtype)
    ref = _run(False, *args, t5)
    calls = _count_kernel_calls(monkeypatch)
    got = _run(True, *args, t5)
    _assert_same(got, ref)
    n_kernel = 1 if w_dtype == torch.bfloat16 else 0
    assert calls == {"fwd": n_kernel, "bwd": n_kernel}
    # the mask really drops: about P of y's gradient entries are zero
    zero = (got[2] == 0).float().mean().item()
    assert 0.5 * P < zero < 1.5 * P + 0.2, zero


@pytest.mark.parametrize("rows,d", [(5, 384), (4099, 384), (67, 130)])
def test_no_dh(rows, d, monkeypatch):
    # h unused downstream: its gradient is the norm's alone
    args = _inputs(rows, d, torch.bfloat16, seed=1)
    ref = _run(False, *args, True, use_h=False)
    calls = _count_kernel_calls(monkeypatch)
    got = _run(True, *args, True, use_h=False)
    _assert_same(got, ref)
    assert calls == {"fwd": 1, "bwd": 1}


@pytest.mark.parametrize("rows,d", [(5, 384), (4099, 384), (67, 130)])
def test_no_dn(rows, d, monkeypatch):
    # n unused downstream: plain dropout_add backward, no weight gradient
    args = _inputs(rows, d, torch.bfloat16, seed=2)
    ref = _run(False, *args, False, use_n=False)
    calls = _count_kernel_calls(monkeypatch)
    got = _run(True, *args, False, use_n=False)
    _assert_same(got, ref)
    assert got[4] is None
    assert calls == {"fwd": 1, "bwd": 0}


def test_3d_input_and_seed_counter():
    # [B, L, d] input as the model passes it, and the device seed counter
    # shifts the mask the same way in both paths
    y, res, w, gh, gn = _inputs(6 * 61, 384, torch.bfloat16, seed=3)
    y3, res3 = (t.detach().view(6, 61, 384).requires_grad_()
                for t in (y, res))
    gh3, gn3 = gh.view(6, 61, 384), gn.view(6, 61, 384)
    ctr = _seed_counter(_dev())
    keep = ctr.clone()
    try:
        base = _run(True, y3, res3, w, gh3, gn3, True)
        ctr.add_(5)
        ref = _run(False, y3, res3, w, gh3, gn3, True)
        got = _run(True, y3, res3, w, gh3, gn3, True)
    finally:
        ctr.copy_(keep)
    _assert_same(got, ref)
    assert got[0].shape == (6, 61, 384)
    assert not torch.equal(got[0], base[0])


_CAP_CHILD = """
import sys, torch
sys.path[:0] = [{tests!r}, {root!r}]
import test_addnorm_gpu as T
args = T._inputs(261, 384, torch.bfloat16, seed=4)
T._assert_same(T._run(True, *args, True), T._run(False, *args, True))
print("CAP64_OK")
"""


def test_grid_stride_with_small_block_cap():
    # GENREC_RMS_BWD_CAP is read once per process: 64 blocks x 4 waves is
    # 256 rows, so 261 rows put a second row on the first five waves
    env = dict(os.environ, GENREC_RMS_BWD_CAP="64")
    tests = os.path.dirname(os.path.abspath(__file__))
    code = _CAP_CHILD.format(tests=tests, root=os.path.dirname(tests))
    r = subprocess.run([sys.executable, "-c", code], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CAP64_OK" in r.stdout, r.stderr[-2000:]


@pytest.mark.parametrize("case", ["odd_d", "fp32_y", "eval", "p0", "env"])
def test_fallbacks_compose(case, monkeypatch):
    rows, d, dtype, p, training = 37, 384, torch.bfloat16, P, True
    if case == "odd_d":
        d = 129
    elif case == "fp32_y":
        dtype = torch.float32
    elif case == "eval":
        training = False
    elif case == "p0":
        p = 0.0
    y, res, w, gh, gn = _inputs(rows, d, dtype, seed=5, dtype=dtype)
    calls = _count_kernel_calls(monkeypatch)
    if case == "env":
        monkeypatch.setenv("GENREC_DISABLE_ADDNORM", "1")
    torch.manual_seed(11)
    h, n = ops.dropout_add_rms_norm(y, res, w, p, EPS, True, training)
    torch.manual_seed(11)
    h_ref = ops.dropout_add(y, res, p, training)
    n_ref = ops.rms_norm(h_ref, w, EPS, True)
    assert calls == {"fwd": 0, "bwd": 0}
    assert torch.equal(h, h_ref) and torch.equal(n, n_ref)
    dy, dres, dw = torch.autograd.grad((h, n), (y, res, w),
                                       (gh, gn.to(n.dtype)))
    ref = torch.autograd.grad((h_ref, n_ref), (y, res, w),
                              (gh, gn.to(n.dtype)))
    assert calls == {"fwd": 0, "bwd": 0}
    for a, b in zip((dy, dres, dw), ref):
        assert torch.equal(a, b)


def test_wrapper_rejects_ineligible_inputs():
    y, res, w, _, _ = _inputs(8, 384, torch.bfloat16)
    ext = ops.ext()
    with pytest.raises(RuntimeError, match="bf16 only"):
        ext.dropout_add_rms_norm_fwd(y.detach().float(), res.detach().float(),
                                     w.detach(), P, EPS, True, 1, None)
    yo = torch.zeros(8, 129, device=_dev(), dtype=torch.bfloat16)
    wo = torch.ones(129, device=_dev(), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="unsupported d"):
        ext.dropout_add_rms_norm_fwd(yo, yo, wo, P, EPS, True, 1, None)


# ------------------------------------------------------------------ stack

def _stack():
    from genrec_amd.modules.norms import T5RMSNorm
    from genrec_amd.modules.transformer import TransformerEncoderDecoder

    torch.manual_seed(0)
    m = TransformerEncoderDecoder(
        d_model=128, nhead=2, num_encoder_layers=2, num_decoder_layers=2,
        dim_feedforward=256, dropout=0.1, norm_cls=T5RMSNorm)
    m = m.to(_dev(), torch.bfloat16).train()
    g = torch.Generator(device="cpu").manual_seed(1)
    src = torch.randn(4, 7, 128, generator=g).to(_dev(), torch.bfloat16)
    tgt = torch.randn(4, 4, 128, generator=g).to(_dev(), torch.bfloat16)
    pad = torch.zeros(4, 7, dtype=torch.bool, device=_dev())
    pad[1, 4:] = True
    return m, src, tgt, pad


def _stack_step(m, src, tgt, pad):
    out = m(src, tgt, src_key_padding_mask=pad, memory_key_padding_mask=pad)
    out.float().square().mean().backward()
    return out


def test_stack_switch_on_equals_off(monkeypatch):
    m, src, tgt, pad = _stack()
    results = []
    for disable in ("1", "0"):
        monkeypatch.setenv("GENREC_DISABLE_ADDNORM", disable)
        calls = _count_kernel_calls(monkeypatch)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(21)
        out = _stack_step(m, src, tgt, pad)
        results.append((out.detach().clone(),
                        {k: p.grad.clone() for k, p in m.named_parameters()}))
        # encoder: 2 layers x 2 sublayers - 1; decoder: 2 x 3 - 1
        want = 0 if disable == "1" else 8
        assert calls == {"fwd": want, "bwd": want}
    (out_off, g_off), (out_on, g_on) = results
    assert torch.equal(out_on, out_off)
    assert g_on.keys() == g_off.keys()
    for k in g_off:
        assert torch.equal(g_on[k], g_off[k]), k


def test_stack_graph_capture_replays():
    m, src, tgt, pad = _stack()
    ctr = _seed_counter(_dev())
    keep = ctr.clone()
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                m.zero_grad(set_to_none=True)
                _stack_step(m, src, tgt, pad)
        torch.cuda.current_stream().wait_stream(side)
        m.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = _stack_step(m, src, tgt, pad)
        ctr.copy_(keep)
        graph.replay()
        first = out.clone()
        for _ in range(2):
            ctr.add_(1)
            graph.replay()
        third = out.clone()
        for k, p in m.named_parameters():
            assert torch.isfinite(p.grad).all(), k
        assert torch.isfinite(third).all()
        assert not torch.equal(third, first)    # the masks did move
        ctr.copy_(keep)
        graph.replay()
        assert torch.equal(out, first)
    finally:
        ctr.copy_(keep)
        torch.cuda.synchronize()
