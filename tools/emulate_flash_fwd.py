"""Thread-level emulation of csrc/kernels/attention_flash.hip (forward).

Reproduces the EXACT control flow and index math of the staged kernel —
the 256-thread block (4 waves x 64 lanes), the staging loops (including
the 8x8 butterfly transpose for V^T), frag_load geometry, per-wave
mfma_f32_16x16x32 semantics, the C-fragment epilogue with 16-lane
shuffle reductions, and the running-softmax state — in numpy, then
compares the result against plain softmax attention. An indexing or
lane-mapping bug in the kernel's logic shows up here as a mismatch,
without spending GPU time. (LDS XOR swizzling is omitted: it is a
bijection within each row applied identically by stores and frag loads,
proven separately; tiles are emulated at element granularity.)
In the kernel the per-wave products, the P stash and the row store are the
runtime strip steps of csrc/core/flash_strip.h (strip_mma, strip_stash,
strip_store); `strip` / `row_grp` + `col` here are Strip::row0 / row / col
there, and the staging index math is tile_chunk in mfma_tile.h.

Run: python tools/emulate_flash_fwd.py
"""

import numpy as np

FTILE = 64
FNEG = -1e9


def xpose8x8(vals, g):
    """vals: [8 lanes in the butterfly group][8 elems]; returns transposed
    per-lane arrays — mirrors the device butterfly (validated separately)."""
    vals = [list(v) for v in vals]
    for m in (1, 2, 4):
        nv = [list(v) for v in vals]
        for gg in range(8):
            for e in range(8):
                if (e & m) != (gg & m):
                    nv[gg][e] = vals[gg ^ m][e ^ m]
        vals = nv
    return vals


def frag_load(tile, row0, k0, lane):
    row = row0 + (lane & 15)
    col = k0 + ((lane >> 4) << 3)
    return tile[row, col:col + 8]


def mfma_16x16x32(a_frag_by_lane, b_frag_by_lane, acc_by_lane):
    """Wave-level emulation: reconstruct A[16,32], B[16,32] from the 64
    lanes' fragments, compute D = A @ B^T, redistribute as C fragments
    (row (lane>>4)*4+r, col lane&15)."""
    A = np.zeros((16, 32))
    B = np.zeros((16, 32))
    for lane in range(64):
        r = lane & 15
        kc = (lane >> 4) * 8
        A[r, kc:kc + 8] = a_frag_by_lane[lane]
        B[r, kc:kc + 8] = b_frag_by_lane[lane]
    D = A @ B.T  # [16 rows(i)][16 cols(j)]
    out = [np.array(acc_by_lane[lane], dtype=np.float64).copy()
           for lane in range(64)]
    for lane in range(64):
        col = lane & 15
        row_grp = (lane >> 4) << 2
        for r in range(4):
            out[lane][r] += D[row_grp + r, col]
    return out


def emulate_block(q, k, v, bias, causal, scale, b, h, q0, out, s_saved, ml):
    """One (b,h,q-tile) block of attn_fwd_flash_kernel."""
    Bq, Hh, Lq, D = q.shape
    Lk = k.shape[2]
    qs = np.zeros((FTILE, FTILE))
    ks = np.zeros((FTILE, FTILE))
    vt = np.zeros((FTILE, FTILE))
    ps = np.zeros((FTILE, FTILE))

    # ---- stage Q once (loop: idx = tid; idx < 512; idx += 256)
    for tid in range(256):
        for idx in range(tid, FTILE * (FTILE // 8), 256):
            row = idx // (FTILE // 8)
            d0 = (idx % (FTILE // 8)) * 8
            qi = q0 + row
            val = q[b, h, qi, d0:d0 + 8] if (qi < Lq and d0 < D) else 0.0
            qs[row, d0:d0 + 8] = val

    # per-lane running state: m, l per (wave, lane, r); accO fragments
    m_row = np.full((4, 64, 4), -1e30)
    l_row = np.zeros((4, 64, 4))
    accO = np.zeros((4, 64, 4, 4))  # [wave][lane][f][r]
    nfrag_d = (D + 15) // 16

    for kt0 in range(0, Lk, FTILE):
        # ---- stage K tile + V^T (butterfly) — emulate per wave-iteration
        for w in range(4):
            for it in range(2):  # idx = tid, tid+256
                # gather the 64 lanes' loads for this wave-iteration
                vv_by_lane = {}
                for lane in range(64):
                    tid = w * 64 + lane
                    idx = tid + it * 256
                    row = idx // (FTILE // 8)
                    d0 = (idx % (FTILE // 8)) * 8
                    kj = kt0 + row
                    val = k[b, h, kj, d0:d0 + 8] \
                        if (kj < Lk and d0 < D) else np.zeros(8)
                    ks[row, d0:d0 + 8] = val
                    vv = v[b, h, kj, d0:d0 + 8] \
                        if (kj < Lk and d0 < D) else np.zeros(8)
                    vv_by_lane[lane] = (row, d0, vv)
                # butterfly groups: lanes {8g + c : g=0..7} for each c
                for c in range(8):
                    group = [vv_by_lane[8 * g + c][2] for g in range(8)]
                    t = xpose8x8(group, 0)  # returns full transposed set
                    for g in range(8):
                        row, d0, _ = vv_by_lane[8 * g + c]
                        j0 = row & ~7
                        vt[d0 + g, j0:j0 + 8] = t[g]

        # ---- S = Q K_t^T per wave
        for w in range(4):
            strip = w * 16
            acc = [[np.zeros(4) for _ in range(64)] for _ in range(4)]
            for f in range(4):
                frag_acc = [np.zeros(4) for _ in range(64)]
                for kk in range(0, D, 32):
                    a = [frag_load(qs, strip, kk, ln) for ln in range(64)]
                    bb = [frag_load(ks, f * 16, kk, ln) for ln in range(64)]
                    frag_acc = mfma_16x16x32(a, bb, frag_acc)
                for ln in range(64):
                    acc[f][ln] = frag_acc[ln]

            # ---- epilogue per lane
            s_val = np.zeros((64, 4, 4))
            for ln in range(64):
                col = ln & 15
                row_grp = (ln >> 4) << 2
                for f in range(4):
                    for r in range(4):
                        i = q0 + strip + row_grp + r
                        j = kt0 + f * 16 + col
                        s = acc[f][ln][r]
                        if i < Lq and j < Lk:
                            s *= scale
                            if bias is not None:
                                s += bias[h, i, j]
                            if causal and j > i:
                                s = FNEG
                            s_saved[b, h, i, j] = s
                        else:
                            s = -np.inf
                        s_val[ln, f, r] = s

            # running softmax with 16-lane shuffle reductions
            for r in range(4):
                for grp in range(4):  # 16-lane groups within the wave
                    lanes = range(grp * 16, grp * 16 + 16)
                    tmax = max(max(s_val[ln, f, r] for f in range(4))
                               for ln in lanes)
                    for ln in lanes:
                        m_new = max(m_row[w, ln, r], max(tmax, -1e30))
                        a_resc = np.exp(m_row[w, ln, r] - m_new)
                        m_row[w, ln, r] = m_new
                        l_row[w, ln, r] *= a_resc
                        accO[w, ln, :, r] *= a_resc
                    ssum = 0.0
                    for ln in lanes:
                        for f in range(4):
                            p = 0.0 if s_val[ln, f, r] == -np.inf else \
                                np.exp(s_val[ln, f, r] - m_row[w, ln, r])
                            s_val[ln, f, r] = p
                            ssum += p
                    for ln in lanes:
                        l_row[w, ln, r] += ssum

            # stash P into ps (tile-local columns)
            for ln in range(64):
                col = ln & 15
                row_grp = (ln >> 4) << 2
                for f in range(4):
                    for r in range(4):
                        row = strip + row_grp + r
                        ps[row, f * 16 + col] = s_val[ln, f, r]

            # accO += P V_t
            for f in range(nfrag_d):
                a_prev = [accO[w, ln, f, :].copy() for ln in range(64)]
                for kk in range(0, FTILE, 32):
                    a = [frag_load(ps, strip, kk, ln) for ln in range(64)]
                    bb = [frag_load(vt, f * 16, kk, ln) for ln in range(64)]
                    a_prev = mfma_16x16x32(a, bb, a_prev)
                for ln in range(64):
                    accO[w, ln, f, :] = a_prev[ln]

    # ---- finalize
    for w in range(4):
        strip = w * 16
        for ln in range(64):
            col = ln & 15
            row_grp = (ln >> 4) << 2
            for f in range(nfrag_d):
                for r in range(4):
                    i = q0 + strip + row_grp + r
                    d = f * 16 + col
                    if i < Lq and d < D:
                        l = l_row[w, ln, r]
                        out[b, h, i, d] = accO[w, ln, f, r] / l if l > 0 \
                            else 0.0
            if col == 0:
                for r in range(4):
                    i = q0 + strip + row_grp + r
                    if i < Lq:
                        ml[b, h, i] = (m_row[w, ln, r], l_row[w, ln, r])


def main():
    rng = np.random.default_rng(0)
    B, H, Lq, Lk, D, scale = 1, 2, 100, 128, 64, 0.125
    q = rng.standard_normal((B, H, Lq, D))
    k = rng.standard_normal((B, H, Lk, D))
    v = rng.standard_normal((B, H, Lk, D))
    bias = 0.3 * rng.standard_normal((H, Lq, Lk))
    for causal in (False, True):
        out = np.zeros((B, H, Lq, D))
        s_saved = np.zeros((B, H, Lq, Lk))
        ml = np.zeros((B, H, Lq, 2))
        for b in range(B):
            for h in range(H):
                for q0 in range(0, Lq, FTILE):
                    emulate_block(q, k, v, bias, causal, scale, b, h, q0,
                                  out, s_saved, ml)
        # reference
        s = np.einsum("bhid,bhjd->bhij", q, k) * scale + bias[None]
        if causal:
            ii = np.arange(Lq)[:, None]
            jj = np.arange(Lk)[None, :]
            s = np.where((jj > ii)[None, None], FNEG, s)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        ref = np.einsum("bhij,bhjd->bhid", p, v)
        err = np.abs(out - ref).max()
        err_s = np.abs(s_saved - s).max()
        print(f"causal={causal}: out err {err:.2e}, s_saved err {err_s:.2e}")
        assert err < 1e-10 and err_s < 1e-10
    print("flash forward kernel logic emulated exactly: staging loops, "
          "butterfly V^T, fragment geometry, running softmax all correct")


if __name__ == "__main__":
    main()
