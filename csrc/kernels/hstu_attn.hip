// HSTU fused pointwise attention (K4+K5+K6 — SURVEY.md §2.4), gfx950.
//
// The full HSTU signature op in one MFMA kernel: S = Q K^T + position bias
// + temporal bias, causal/key-pad masks at -1e9, SiLU scores (no softmax),
// O = SiLU(S) V. The two bias terms are computed IN the epilogue — the
// T5-style position bucket table is a precomputed [L,L] index (input-
// independent), the temporal bucket is ln2-bucketed |ts_i - ts_j| computed
// per element — so the reference's [B,H,L,L] bias materialization
// (hstu.py:283-409: ~6 large elementwise + 2 gathers per layer) never
// happens.
//
// Backward: dP = dO V^T (MFMA), dS = dP * SiLU'(S), bias-table gradients
// are reduced per-block into LDS histograms (one head per block, <=
// n_pos + n_time floats) and flushed with one global atomicAdd per bucket,
// then dQ/dK/dV run as MFMA in the same launch.
//
// One 64-row tile per (b, h); the strip steps are flash_strip.h's runtime
// forms (D is a kernel argument), shared with attention_flash.hip.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../core/attn_host.h"
#include "../core/hstu_bias.h"

namespace genrec {

__global__ void __launch_bounds__(256)
hstu_attn_fwd_kernel(
    const __hip_bfloat16* __restrict__ q,     // [B,H,L,D]
    const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v,
    const int* __restrict__ pos_bucket,       // [L,L]
    const __hip_bfloat16* __restrict__ pos_table,   // [n_pos, H]
    const __hip_bfloat16* __restrict__ time_table,  // null | [n_time, H]
    const long long* __restrict__ ts,         // null | [B,L]
    const bool* __restrict__ key_pad,         // null | [B,L]
    __hip_bfloat16* __restrict__ out,
    float* __restrict__ s_saved,              // [B,H,L,L] post-mask scores
    int B, int H, int L, int D, int n_time) {
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qs = smem;
  char* ks = qs + TILE * 128;
  char* vt = ks + TILE * 128;
  char* ps = vt + TILE * 128;

  const int tid = threadIdx.x;
  const Strip w(tid);

  for (int idx = tid; idx < TILE_CHUNKS; idx += blockDim.x) {
    const TileChunk c = tile_chunk(idx);
    const bool ok = c.row < L && c.d0 < D;
    const int64_t src = idx4(b, h, c.row, c.d0, H, L, D);
    tile_store(qs, c.row, c.d0, load8(q, src, ok));
    tile_store(ks, c.row, c.d0, load8(k, src, ok));
    // V^T: coalesced natural-row load + in-register 8x8 transpose
    tile_store_tr(vt, c.row, c.d0, w.lane, load8(v, src, ok));
  }
  __syncthreads();

  float4v acc[4] = {};
  strip_mma(acc, qs, ks, D, 4, w);

#pragma unroll
  for (int f = 0; f < 4; ++f) {
    short4v p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = w.row + r;
      int j = f * 16 + w.col;
      float s = acc[f][r];
      float pv = 0.f;
      if (i < L && j < L) {
        s += to_f32(pos_table[(int64_t)pos_bucket[i * L + j] * H + h]);
        if (time_table) {
          int tb = time_bucket(ts[(int64_t)b * L + i],
                               ts[(int64_t)b * L + j], n_time);
          s += to_f32(time_table[(int64_t)tb * H + h]);
        }
        if (j > i) s = NEG_BIG;                                     // causal
        if (key_pad && key_pad[(int64_t)b * L + j]) s = NEG_BIG;    // pad
        s_saved[idx4(b, h, i, j, H, L, L)] = s;
        pv = s * sigmoidf_dev(s);
      }
      p[r] = bf16_bits(pv);
    }
    strip_stash(ps, f, p, w);
  }
  __builtin_amdgcn_wave_barrier();

  float4v acc2[4] = {};
  strip_mma(acc2, ps, vt, TILE, (D + 15) / 16, w);
  strip_store(out, bh, 0, L, D, acc2, w);
}

__global__ void __launch_bounds__(256)
hstu_attn_bwd_kernel(
    const __hip_bfloat16* __restrict__ dout,
    const __hip_bfloat16* __restrict__ q,
    const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v,
    const float* __restrict__ s_saved,        // [B,H,L,L]
    const int* __restrict__ pos_bucket,       // [L,L]
    const long long* __restrict__ ts,         // null | [B,L]
    __hip_bfloat16* __restrict__ dq_out,
    __hip_bfloat16* __restrict__ dk_out,
    __hip_bfloat16* __restrict__ dv_out,
    float* __restrict__ dpos,                 // [n_pos, H] fp32 accum
    float* __restrict__ dtime,                // null | [n_time, H]
    int B, int H, int L, int D, int n_pos, int n_time) {
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* dos = smem;
  char* vs = dos + TILE * 128;
  char* kt = vs + TILE * 128;
  char* qt = kt + TILE * 128;
  char* dot = qt + TILE * 128;
  char* dsn = dot + TILE * 128;
  char* dst = dsn + TILE * 128;
  char* adt = dst + TILE * 128;
  float* hist = reinterpret_cast<float*>(adt + TILE * 128);  // [n_pos+n_time]

  const int tid = threadIdx.x;
  const Strip w(tid);
  const int n_hist = n_pos + n_time;
  for (int i = tid; i < n_hist; i += blockDim.x) hist[i] = 0.f;

  for (int idx = tid; idx < TILE_CHUNKS; idx += blockDim.x) {
    const TileChunk c = tile_chunk(idx);
    const bool ok = c.row < L && c.d0 < D;
    const int64_t src = idx4(b, h, c.row, c.d0, H, L, D);
    short8v dd8 = load8(dout, src, ok);
    short8v vv8 = load8(v, src, ok);
    short8v kk8 = load8(k, src, ok);
    short8v qq8 = load8(q, src, ok);
    tile_store(dos, c.row, c.d0, dd8);
    tile_store(vs, c.row, c.d0, vv8);
    // K^T/Q^T/dO^T: coalesced natural-row b128 loads + in-register 8x8
    // transpose, one b128 LDS store per tensor
    tile_store_tr(kt, c.row, c.d0, w.lane, kk8);
    tile_store_tr(qt, c.row, c.d0, w.lane, qq8);
    tile_store_tr(dot, c.row, c.d0, w.lane, dd8);
  }
  __syncthreads();

  float4v acc[4] = {};
  strip_mma(acc, dos, vs, D, 4, w);

#pragma unroll
  for (int f = 0; f < 4; ++f) {
    short4v ds, ad;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = w.row + r;
      int j = f * 16 + w.col;
      float dsv = 0.f, adv = 0.f;
      if (i < L && j < L) {
        float s = s_saved[idx4(b, h, i, j, H, L, L)];
        float sg = sigmoidf_dev(s);
        dsv = acc[f][r] * sg * (1.f + s * (1.f - sg));
        adv = s * sg;  // A = silu(S)
        // bias-table gradients (dS at masked positions is ~0 since
        // SiLU'(-1e9) == 0 — matching autograd's masked_fill)
        if (dsv != 0.f) {
          atomicAdd(&hist[pos_bucket[i * L + j]], dsv);
          if (dtime) {
            int tb = time_bucket(ts[(int64_t)b * L + i],
                                 ts[(int64_t)b * L + j], n_time);
            atomicAdd(&hist[n_pos + tb], dsv);
          }
        }
      }
      ds[r] = bf16_bits(dsv);
      ad[r] = bf16_bits(adv);
    }
    strip_stash(dsn, f, ds, w);
    strip_stash_tr(dst, f, ds, w);
    strip_stash_tr(adt, f, ad, w);
  }

  float4v ak[4] = {};
  float4v av[4] = {};
  strip_bwd_products(dsn, kt, dst, qt, adt, dot, (D + 15) / 16, ak, av, w,
                     [&](const float4v (&aq)[4]) {
                       strip_store(dq_out, bh, 0, L, D, aq, w);
                     });
  strip_store(dk_out, bh, 0, L, D, ak, w);
  strip_store(dv_out, bh, 0, L, D, av, w);

  // flush bias histograms: one global atomicAdd per bucket per block
  __syncthreads();
  for (int i = tid; i < n_hist; i += blockDim.x) {
    float val = hist[i];
    if (val != 0.f) {
      if (i < n_pos) atomicAdd(&dpos[(int64_t)i * H + h], val);
      else atomicAdd(&dtime[(int64_t)(i - n_pos) * H + h], val);
    }
  }
}

// ------------------------------------------------------------------ hosts

std::vector<torch::Tensor> hstu_attn_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor pos_bucket, torch::Tensor pos_table,
    c10::optional<torch::Tensor> time_table,
    c10::optional<torch::Tensor> timestamps,
    c10::optional<torch::Tensor> key_pad) {
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 && q.dim() == 4);
  const int B = q.size(0), H = q.size(1), L = q.size(2), D = q.size(3);
  TORCH_CHECK(L <= TILE && D % 32 == 0 && D <= TILE);
  TORCH_CHECK(pos_table.scalar_type() == torch::kBFloat16);
  auto out = torch::empty_like(q);
  auto s_saved = torch::empty({B, H, L, L},
                              q.options().dtype(torch::kFloat32));
  auto pb = pos_bucket.to(torch::kInt32).contiguous();
  torch::Tensor ts64, pad_c;
  if (timestamps.has_value())
    ts64 = timestamps->to(torch::kInt64).contiguous();
  int n_time = time_table.has_value() ? time_table->size(0) : 0;
  dim3 block(256);
  dim3 grid(B * H);
  size_t smem = 4 * TILE * 128;
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(hstu_attn_fwd_kernel, grid, block, smem, stream,
      bf16_cptr(q), bf16_cptr(k), bf16_cptr(v), pb.data_ptr<int>(),
      bf16_cptr(pos_table),
      time_table.has_value() ? bf16_cptr(*time_table) : nullptr,
      timestamps.has_value()
          ? reinterpret_cast<const long long*>(ts64.data_ptr())
          : nullptr,
      pad_ptr(key_pad, pad_c), bf16_ptr(out), s_saved.data_ptr<float>(),
      B, H, L, D, n_time);
  return {out, s_saved};
}

std::vector<torch::Tensor> hstu_attn_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor s_saved, torch::Tensor pos_bucket,
    c10::optional<torch::Tensor> timestamps,
    int64_t n_pos, int64_t n_time) {
  const int B = q.size(0), H = q.size(1), L = q.size(2), D = q.size(3);
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  auto dpos = torch::zeros({n_pos, H}, q.options().dtype(torch::kFloat32));
  torch::Tensor dtime;
  float* dtime_ptr = nullptr;
  if (n_time > 0) {
    dtime = torch::zeros({n_time, H}, q.options().dtype(torch::kFloat32));
    dtime_ptr = dtime.data_ptr<float>();
  } else {
    dtime = torch::empty({0}, q.options().dtype(torch::kFloat32));
  }
  auto pb = pos_bucket.to(torch::kInt32).contiguous();
  torch::Tensor ts64;
  if (timestamps.has_value())
    ts64 = timestamps->to(torch::kInt64).contiguous();
  auto dc = dout.contiguous();
  dim3 block(256);
  dim3 grid(B * H);
  size_t smem = 8 * TILE * 128 +
                ((size_t)n_pos + (size_t)n_time) * sizeof(float);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(hstu_attn_bwd_kernel, grid, block, smem, stream,
      bf16_cptr(dc), bf16_cptr(q), bf16_cptr(k), bf16_cptr(v),
      s_saved.data_ptr<float>(), pb.data_ptr<int>(),
      timestamps.has_value()
          ? reinterpret_cast<const long long*>(ts64.data_ptr())
          : nullptr,
      bf16_ptr(dq), bf16_ptr(dk), bf16_ptr(dv),
      dpos.data_ptr<float>(), dtime_ptr,
      B, H, L, D, (int)n_pos, (int)n_time);
  return {dq, dk, dv, dpos, dtime};
}

}  // namespace genrec
