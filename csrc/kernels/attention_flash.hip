// Flash-tiled MFMA attention (bf16, softmax) — Lq/Lk beyond one 64-tile.
//
// Same fragment geometry as attention_mfma.hip, plus a running softmax
// over 64-wide key tiles (forward) and a k-tile-owning backward that
// loops q-tiles, accumulating dK/dV in registers and dQ via fp32 global
// atomics. The tile math (running m/l rescale; single-pass backward via
// the identity dot_i = rowsum(dO * O)) is validated at fragment
// granularity against autograd in tools/sim_flash_tiles.py (~1e-15).
// The strip steps (products, stashes, row stores, the backward's product
// tail) are flash_strip.h's runtime forms: D is a kernel argument here.
//
// DEFAULT for Lk>64 since round 2 (GPU-validated; routes the COBRA
// decoder). Stride-aware on the input side: q/k/v (+dout in backward)
// may be [B,L,H,D]-style transpose views with d innermost.
//
// Backward saves scores S (post-mask) + per-row (m, l) instead of
// normalized P; P is reconstructed as exp(S - m)/l in the epilogue.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../core/attn_host.h"

namespace genrec {

__global__ void __launch_bounds__(256)
attn_fwd_flash_kernel(
    FlashView q, FlashView k, FlashView v,  // [B,H,L,D] views
    const void* __restrict__ bias,          // null | [H,Lq,Lk] | [B,H,Lq,Lk]
    const bool* __restrict__ key_pad,       // null | [B,Lk]
    const float* __restrict__ add_mask,     // null | [Lq,Lk]
    const float* __restrict__ query_mask,   // null | [B,Lq]
    __hip_bfloat16* __restrict__ out,       // [B,H,Lq,D]
    float* __restrict__ s_saved,            // [B,H,Lq,Lk] post-mask scores
    float* __restrict__ ml_saved,           // [B,H,Lq,2] (m, l)
    unsigned char* __restrict__ drop_mask,  // null | [B,H,Lq,Lk]
    const unsigned int* __restrict__ seed_dev,
    int B, int H, int Lq, int Lk, int D,
    float scale, int bias_dim, bool bias_bf16, bool causal,
    float dropout_p, unsigned int seed) {
  if (seed_dev) seed += *seed_dev;
  const float* bias_f = reinterpret_cast<const float*>(bias);
  const __hip_bfloat16* bias_b = reinterpret_cast<const __hip_bfloat16*>(bias);
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int q0 = blockIdx.y * TILE;
  const __hip_bfloat16* qr = q.rows(b, h);
  const __hip_bfloat16* kr = k.rows(b, h);
  const __hip_bfloat16* vr = v.rows(b, h);

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qs = smem;                 // [64][128B] Q rows
  char* ks = qs + TILE * 128;      // [64][128B] K rows (per tile)
  char* vt = ks + TILE * 128;      // [64(d)][128B(j)] V^T (per tile)
  char* ps = vt + TILE * 128;      // [64][128B] P (per tile)

  const int tid = threadIdx.x;
  const Strip w(tid);
  const float inv_keep = dropout_p > 0.f ? 1.0f / (1.0f - dropout_p) : 1.0f;

  // ---- stage Q once
  for (int idx = tid; idx < TILE_CHUNKS; idx += blockDim.x) {
    const TileChunk c = tile_chunk(idx);
    const int qi = q0 + c.row;
    tile_store(qs, c.row, c.d0,
               load8(qr, qi * q.l + c.d0, qi < Lq && c.d0 < D));
  }

  // Running softmax state. Not flash_strip.h's RunningSoftmax: a row whose
  // every score is -inf (an additive mask can do that) saves m = -1e30 here
  // and would save -inf there; every other stored bit is the same.
  float m_row[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
  float l_row[4] = {0.f, 0.f, 0.f, 0.f};
  float4v accO[4] = {};
  const int nfrag_d = (D + 15) / 16;

  for (int kt0 = 0; kt0 < Lk; kt0 += TILE) {
    __syncthreads();  // previous iteration's ps/ks/vt fully consumed
    // ---- stage K tile + V^T tile
    for (int idx = tid; idx < TILE_CHUNKS; idx += blockDim.x) {
      const TileChunk c = tile_chunk(idx);
      const int kj = kt0 + c.row;
      const bool ok = kj < Lk && c.d0 < D;
      tile_store(ks, c.row, c.d0, load8(kr, kj * k.l + c.d0, ok));
      tile_store_tr(vt, c.row, c.d0, w.lane,
                    load8(vr, kj * v.l + c.d0, ok));
    }
    __syncthreads();

    // ---- S = Q K_t^T
    float4v acc[4] = {};
    strip_mma(acc, qs, ks, D, 4, w);

    // ---- epilogue: masks. The kernel's own masks score NEG_BIG, which
    // stays in the softmax; -inf (outside the tensors, or from add_mask)
    // has probability exactly 0.
    float s_val[4][4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i = q0 + w.row + r;
        int j = kt0 + f * 16 + w.col;
        float s = acc[f][r];
        if (i < Lq && j < Lk) {
          s *= scale;
          if (bias_dim) {
            int64_t bi = (bias_dim == 3) ? ((int64_t)h * Lq + i) * Lk + j
                                         : idx4(b, h, i, j, H, Lq, Lk);
            s += bias_bf16 ? to_f32(bias_b[bi]) : bias_f[bi];
          }
          if (causal && j > i) s = NEG_BIG;
          if (key_pad && key_pad[(int64_t)b * Lk + j]) s = NEG_BIG;
          if (add_mask) s += add_mask[(int64_t)i * Lk + j];
          s_saved[idx4(b, h, i, j, H, Lq, Lk)] = s;
        } else {
          s = -INFINITY;
        }
        s_val[f][r] = s;
      }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float tmax = grp16_max(fmaxf(fmaxf(s_val[0][r], s_val[1][r]),
                                   fmaxf(s_val[2][r], s_val[3][r])));
      float m_new = fmaxf(m_row[r], fmaxf(tmax, -1e30f));
      float a = __expf(m_row[r] - m_new);
      float sum = 0.f;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        float p = (s_val[f][r] == -INFINITY) ? 0.f
                                             : __expf(s_val[f][r] - m_new);
        s_val[f][r] = p;  // reuse as unnormalized p
        sum += p;
      }
      l_row[r] = l_row[r] * a + grp16_sum(sum);
      m_row[r] = m_new;
      // rescale accumulated O for this row
#pragma unroll
      for (int f = 0; f < 4; ++f) accO[f][r] *= a;
    }

    // ---- dropout (on the accumulated contribution only) + stash P
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i = q0 + w.row + r;
        int j = kt0 + f * 16 + w.col;
        if (i < Lq && j < Lk && dropout_p > 0.f) {
          unsigned long long gidx = idx4(b, h, i, j, H, Lq, Lk);
          bool keep = (hash_rng(seed, gidx) & 0xFFFFFF) >=
                      (unsigned int)(dropout_p * 16777216.0f);
          drop_mask[gidx] = keep;
          s_val[f][r] = keep ? s_val[f][r] * inv_keep : 0.f;
        }
      }
      strip_stash(ps, f, s_val[f], w);
    }
    __builtin_amdgcn_wave_barrier();

    // ---- accO += P V_t
    strip_mma(accO, ps, vt, TILE, nfrag_d, w);
  }

  // ---- finalize: normalize, query mask, write out + (m, l)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + w.row + r;
    if (i >= Lq) continue;
    const float inv = (l_row[r] > 0.f) ? 1.0f / l_row[r] : 0.f;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      accO[f][r] *= inv;
      if (query_mask) accO[f][r] *= query_mask[(int64_t)b * Lq + i];
    }
    if (w.col == 0) {
      ml_saved[((int64_t)bh * Lq + i) * 2 + 0] = m_row[r];
      ml_saved[((int64_t)bh * Lq + i) * 2 + 1] = l_row[r];
    }
  }
  strip_store(out, bh, q0, Lq, D, accO, w);
}

// Backward: one block per (b, h, k-tile); loops q-tiles. dK/dV accumulate
// in registers across q-tiles; dQ partials go to an fp32 buffer via
// atomicAdd (each (i,d) is touched by n_k_tiles blocks).
__global__ void __launch_bounds__(256)
attn_bwd_flash_kernel(
    FlashView dout, FlashView q, FlashView k, FlashView v,  // [B,H,L,D] views
    const float* __restrict__ s_saved,        // [B,H,Lq,Lk]
    const float* __restrict__ ml_saved,       // [B,H,Lq,2]
    const float* __restrict__ dot_row,        // [B,H,Lq] rowsum(dO*O)
    const float* __restrict__ query_mask,     // null | [B,Lq]
    const unsigned char* __restrict__ drop_mask,
    float* __restrict__ dq_f32,               // [B,H,Lq,D] zero-init
    __hip_bfloat16* __restrict__ dk_out,
    __hip_bfloat16* __restrict__ dv_out,
    float* __restrict__ ds_saved,             // null | [B,H,Lq,Lk]
    int B, int H, int Lq, int Lk, int D,
    float scale, float dropout_p) {
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int kt0 = blockIdx.y * TILE;
  const __hip_bfloat16* dor = dout.rows(b, h);
  const __hip_bfloat16* qr = q.rows(b, h);
  const __hip_bfloat16* kr = k.rows(b, h);
  const __hip_bfloat16* vr = v.rows(b, h);

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* vs = smem;                 // [64][128B] V_t rows (persistent)
  char* kt = vs + TILE * 128;      // [64(d)][128B(j)] K_t^T (persistent)
  char* dos = kt + TILE * 128;     // [64][128B] dO rows (per q-tile)
  char* qt = dos + TILE * 128;     // [64(d)][128B(i)] Q^T (per q-tile)
  char* dot = qt + TILE * 128;     // [64(d)][128B(i)] dO^T (per q-tile)
  char* dsn = dot + TILE * 128;    // [64(i)][128B(j)] dS
  char* dst = dsn + TILE * 128;    // [64(j)][128B(i)] dS^T
  char* adt = dst + TILE * 128;    // [64(j)][128B(i)] A_d^T

  const int tid = threadIdx.x;
  const Strip w(tid);
  const float inv_keep = dropout_p > 0.f ? 1.0f / (1.0f - dropout_p) : 1.0f;

  // ---- stage V_t natural + K_t^T once
  for (int idx = tid; idx < TILE_CHUNKS; idx += blockDim.x) {
    const TileChunk c = tile_chunk(idx);
    const int kj = kt0 + c.row;
    const bool ok = kj < Lk && c.d0 < D;
    short8v vv8 = load8(vr, kj * v.l + c.d0, ok);
    short8v kk8 = load8(kr, kj * k.l + c.d0, ok);
    tile_store(vs, c.row, c.d0, vv8);
    tile_store_tr(kt, c.row, c.d0, w.lane, kk8);
  }

  const int nfrag_d = (D + 15) / 16;
  float4v acck[4] = {};
  float4v accv[4] = {};

  for (int q0 = 0; q0 < Lq; q0 += TILE) {
    __syncthreads();
    // ---- stage dO natural + dO^T + Q^T for this q-tile
    for (int idx = tid; idx < TILE_CHUNKS; idx += blockDim.x) {
      const TileChunk c = tile_chunk(idx);
      const int qi = q0 + c.row;
      const bool ok = qi < Lq && c.d0 < D;
      short8v dd8 = load8(dor, qi * dout.l + c.d0, ok);
      short8v qq8 = load8(qr, qi * q.l + c.d0, ok);
      tile_store(dos, c.row, c.d0, dd8);
      tile_store_tr(dot, c.row, c.d0, w.lane, dd8);
      tile_store_tr(qt, c.row, c.d0, w.lane, qq8);
    }
    __syncthreads();

    // ---- dA = dO V_t^T : C rows = q rows (this wave's strip)
    float4v acc[4] = {};
    strip_mma(acc, dos, vs, D, 4, w);

    // ---- epilogue: reconstruct P, dS = P (M*dA - dot_i); stash tiles
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      short4v ds, ad;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i = q0 + w.row + r;
        int j = kt0 + f * 16 + w.col;
        float dval = 0.f, aval = 0.f;
        if (i < Lq && j < Lk) {
          float m = ml_saved[((int64_t)bh * Lq + i) * 2 + 0];
          float l = ml_saved[((int64_t)bh * Lq + i) * 2 + 1];
          float s = s_saved[idx4(b, h, i, j, H, Lq, Lk)];
          float p = (l > 0.f) ? __expf(s - m) / l : 0.f;
          float mult = 1.f;
          if (query_mask) mult *= query_mask[(int64_t)b * Lq + i];
          if (dropout_p > 0.f) {
            mult *= drop_mask[idx4(b, h, i, j, H, Lq, Lk)] ? inv_keep : 0.f;
          }
          float dp = acc[f][r] * mult;
          dval = p * (dp - dot_row[(int64_t)bh * Lq + i]);
          aval = p * mult;
          if (ds_saved) ds_saved[idx4(b, h, i, j, H, Lq, Lk)] = dval;
        }
        ds[r] = bf16_bits(dval * scale);
        ad[r] = bf16_bits(aval);
      }
      strip_stash(dsn, f, ds, w);
      strip_stash_tr(dst, f, ds, w);
      strip_stash_tr(adt, f, ad, w);
    }

    // dQ rows of this q-tile += (scale*dS) K_t (atomic fp32), then
    // dK_t += (scale*dS)^T Q ; dV_t += A_d^T dO (accumulate over q0)
    strip_bwd_products(
        dsn, kt, dst, qt, adt, dot, nfrag_d, acck, accv, w,
        [&](const float4v (&accq)[4]) {
#pragma unroll
          for (int f = 0; f < 4; ++f) {
            if (f >= nfrag_d) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              int i = q0 + w.row + r;
              int d = f * 16 + w.col;
              if (i < Lq && d < D) {
                atomicAdd(&dq_f32[idx4(b, h, i, d, H, Lq, D)], accq[f][r]);
              }
            }
          }
        });
  }

  // ---- write dK/dV rows of this k-tile
  strip_store(dk_out, bh, kt0, Lk, D, acck, w);
  strip_store(dv_out, bh, kt0, Lk, D, accv, w);
}

// ------------------------------------------------------------------ hosts

std::vector<torch::Tensor> attn_fwd_flash(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> key_pad,
    c10::optional<torch::Tensor> add_mask,
    c10::optional<torch::Tensor> query_mask,
    double scale, bool causal, double dropout_p, int64_t seed,
    c10::optional<torch::Tensor> seed_dev) {
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16);
  const int B = q.size(0), H = q.size(1), Lq = q.size(2), D = q.size(3);
  const int Lk = k.size(2);
  TORCH_CHECK(D <= TILE && D % 32 == 0);
  // stride-aware over [B,H,L,D] views (every [B,L,H,D] transpose view at
  // D % 32 == 0 qualifies). Anything else is copied here, not in the op
  // layer.
  torch::Tensor qn = kernel_readable(q, 3);
  torch::Tensor kn = kernel_readable(k, 3);
  torch::Tensor vn = kernel_readable(v, 3);
  auto out = torch::empty({B, H, Lq, D}, q.options());
  auto opts_f = q.options().dtype(torch::kFloat32);
  auto s_saved = torch::empty({B, H, Lq, Lk}, opts_f);
  auto ml = torch::empty({B, H, Lq, 2}, opts_f);
  torch::Tensor dmask;
  if (dropout_p > 0) {
    dmask = torch::empty({B, H, Lq, Lk}, q.options().dtype(torch::kUInt8));
  } else {
    dmask = torch::empty({0}, q.options().dtype(torch::kUInt8));
  }
  torch::Tensor bias_c, pad_c;
  int bias_dim = 0;
  bool bias_bf16 = false;
  if (bias.has_value()) {
    bias_c = bias->contiguous();
    bias_dim = bias_c.dim();
    bias_bf16 = bias_c.scalar_type() == torch::kBFloat16;
  }
  torch::Tensor am_f, qm_f;
  if (add_mask.has_value()) am_f = add_mask->to(torch::kFloat32).contiguous();
  if (query_mask.has_value())
    qm_f = query_mask->to(torch::kFloat32).contiguous();
  dim3 block(256);
  dim3 grid(B * H, (Lq + TILE - 1) / TILE);
  size_t smem = 4 * TILE * 128;
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(attn_fwd_flash_kernel, grid, block, smem, stream,
      view_bhld(qn), view_bhld(kn), view_bhld(vn),
      bias_dim ? bias_c.data_ptr() : nullptr,
      pad_ptr(key_pad, pad_c),
      add_mask.has_value() ? am_f.data_ptr<float>() : nullptr,
      query_mask.has_value() ? qm_f.data_ptr<float>() : nullptr,
      bf16_ptr(out), s_saved.data_ptr<float>(), ml.data_ptr<float>(),
      dropout_p > 0 ? dmask.data_ptr<unsigned char>() : nullptr,
      seed_dev.has_value()
          ? reinterpret_cast<const unsigned int*>(seed_dev->data_ptr())
          : nullptr,
      B, H, Lq, Lk, D, (float)scale, bias_dim, bias_bf16, causal,
      (float)dropout_p, (unsigned int)seed);
  return {out, s_saved, ml, dmask};
}

std::vector<torch::Tensor> attn_bwd_flash(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor s_saved, torch::Tensor ml,
    torch::Tensor drop_mask, c10::optional<torch::Tensor> query_mask,
    double scale, double dropout_p, bool bias_grad, int64_t bias_dim) {
  const int B = q.size(0), H = q.size(1), Lq = q.size(2), D = q.size(3);
  const int Lk = k.size(2);
  torch::Tensor don = kernel_readable(dout, 3);
  torch::Tensor qn = kernel_readable(q, 3);
  torch::Tensor kn = kernel_readable(k, 3);
  torch::Tensor vn = kernel_readable(v, 3);
  // flash identity: dot_i = rowsum(dO * O) (tools/sim_flash_tiles.py)
  auto dot_row = (don.to(torch::kFloat32) * out.to(torch::kFloat32))
                     .sum(-1).contiguous();
  auto dq_f32 = torch::zeros({B, H, Lq, D},
                             q.options().dtype(torch::kFloat32));
  auto dk = torch::empty({B, H, Lk, D}, k.options());
  auto dv = torch::empty({B, H, Lk, D}, v.options());
  torch::Tensor ds_saved;
  float* ds_ptr = nullptr;
  if (bias_grad) {
    ds_saved = torch::empty({B, H, Lq, Lk},
                            q.options().dtype(torch::kFloat32));
    ds_ptr = ds_saved.data_ptr<float>();
  }
  torch::Tensor qm_f;
  if (query_mask.has_value())
    qm_f = query_mask->to(torch::kFloat32).contiguous();
  dim3 block(256);
  dim3 grid(B * H, (Lk + TILE - 1) / TILE);
  size_t smem = 8 * TILE * 128;
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(attn_bwd_flash_kernel, grid, block, smem, stream,
      view_bhld(don), view_bhld(qn), view_bhld(kn), view_bhld(vn),
      s_saved.data_ptr<float>(), ml.data_ptr<float>(),
      dot_row.data_ptr<float>(),
      query_mask.has_value() ? qm_f.data_ptr<float>() : nullptr,
      dropout_p > 0 ? drop_mask.data_ptr<unsigned char>() : nullptr,
      dq_f32.data_ptr<float>(), bf16_ptr(dk), bf16_ptr(dv), ds_ptr,
      B, H, Lq, Lk, D, (float)scale, (float)dropout_p);
  auto dq = dq_f32.to(torch::kBFloat16);
  torch::Tensor dbias;
  if (bias_grad) {
    dbias = (bias_dim == 3) ? ds_saved.sum(0) : ds_saved;
  } else {
    dbias = torch::empty({0}, q.options().dtype(torch::kFloat32));
  }
  return {dq, dk, dv, dbias};
}

}  // namespace genrec
