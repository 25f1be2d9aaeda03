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

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../core/mfma_tile.h"

namespace genrec {

__device__ __forceinline__ int time_bucket(long long ti, long long tj,
                                           int n_buckets) {
  long long diff = ti - tj;
  if (diff < 0) diff = -diff;
  if (diff < 1) diff = 1;
  int b = (int)(__logf((float)diff) / 0.693f);
  return min(max(b, 0), n_buckets - 1);
}

template <typename BT>
__global__ void __launch_bounds__(256)
hstu_attn_fwd_kernel(
    const __hip_bfloat16* __restrict__ q,     // [B,H,L,D]
    const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v,
    const int* __restrict__ pos_bucket,       // [L,L]
    const BT* __restrict__ pos_table,         // [n_pos, H]
    const BT* __restrict__ time_table,        // null | [n_time, H]
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
  const int lane = tid & 63;
  const int wid = tid >> 6;

  for (int idx = tid; idx < TILE * (TILE / 8); idx += blockDim.x) {
    int row = idx / (TILE / 8);
    int d0 = (idx % (TILE / 8)) * 8;
    const bool ok = row < L && d0 < D;
    const int64_t src = idx4(b, h, row, d0, H, L, D);
    tile_store(qs, row, d0, load8(q, src, ok));
    tile_store(ks, row, d0, load8(k, src, ok));
    // V^T: coalesced natural-row load + in-register 8x8 transpose
    tile_store_tr(vt, row, d0, lane, load8(v, src, ok));
  }
  __syncthreads();

  const int strip = wid * 16;
  float4v acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    for (int kk = 0; kk < D; kk += 32) {
      acc[f] = mfma_bf16(frag_load(qs, strip, kk, lane),
                         frag_load(ks, f * 16, kk, lane), acc[f]);
    }
  }

  const int col_base = frag_col(lane);
  const int row_grp = frag_row0(lane);
#pragma unroll
  for (int f = 0; f < 4; ++f) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = strip + row_grp + r;
      int j = f * 16 + col_base;
      float s = acc[f][r];
      float p = 0.f;
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
        p = s * sigmoidf_dev(s);
      }
      tile_store(ps, i, j, bf16_bits(p));
    }
  }
  __builtin_amdgcn_wave_barrier();

  float4v acc2[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  const int nfrag_d = (D + 15) / 16;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nfrag_d) break;
    for (int kk = 0; kk < TILE; kk += 32) {
      acc2[f] = mfma_bf16(frag_load(ps, strip, kk, lane),
                          frag_load(vt, f * 16, kk, lane), acc2[f]);
    }
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nfrag_d) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = strip + row_grp + r;
      int d = f * 16 + col_base;
      if (i < L && d < D) {
        out[idx4(b, h, i, d, H, L, D)] = __float2bfloat16(acc2[f][r]);
      }
    }
  }
}

template <typename BT>
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
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int n_hist = n_pos + n_time;
  for (int i = tid; i < n_hist; i += blockDim.x) hist[i] = 0.f;

  for (int idx = tid; idx < TILE * (TILE / 8); idx += blockDim.x) {
    int row = idx / (TILE / 8);
    int d0 = (idx % (TILE / 8)) * 8;
    const bool ok = row < L && d0 < D;
    const int64_t src = idx4(b, h, row, d0, H, L, D);
    short8v dd8 = load8(dout, src, ok);
    short8v vv8 = load8(v, src, ok);
    short8v kk8 = load8(k, src, ok);
    short8v qq8 = load8(q, src, ok);
    tile_store(dos, row, d0, dd8);
    tile_store(vs, row, d0, vv8);
    // K^T/Q^T/dO^T: coalesced natural-row b128 loads + in-register 8x8
    // transpose, one b128 LDS store per tensor
    tile_store_tr(kt, row, d0, lane, kk8);
    tile_store_tr(qt, row, d0, lane, qq8);
    tile_store_tr(dot, row, d0, lane, dd8);
  }
  __syncthreads();

  const int strip = wid * 16;
  float4v acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    for (int kk = 0; kk < D; kk += 32) {
      acc[f] = mfma_bf16(frag_load(dos, strip, kk, lane),
                         frag_load(vs, f * 16, kk, lane), acc[f]);
    }
  }

  const int col_base = frag_col(lane);
  const int row_grp = frag_row0(lane);
  // transposed-tile stores pack a lane's 4 r-values (consecutive columns
  // of row j) into ONE aligned 8-byte ds_write — see attention_mfma.hip
  const int i0 = strip + row_grp;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    short4v dpack, apack;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = i0 + r;
      int j = f * 16 + col_base;
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
      dpack[r] = bf16_bits(dsv);
      apack[r] = bf16_bits(adv);
      tile_store(dsn, i, j, dpack[r]);
    }
    int j = f * 16 + col_base;
    tile_store(dst, j, i0, dpack);
    tile_store(adt, j, i0, apack);
  }
  __builtin_amdgcn_wave_barrier();

  const int nfrag_d = (D + 15) / 16;
  {  // dQ
    float4v a4[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (f >= nfrag_d) break;
      for (int kk = 0; kk < TILE; kk += 32) {
        a4[f] = mfma_bf16(frag_load(dsn, strip, kk, lane),
                          frag_load(kt, f * 16, kk, lane), a4[f]);
      }
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (f >= nfrag_d) break;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i = strip + row_grp + r;
        int d = f * 16 + col_base;
        if (i < L && d < D) {
          dq_out[idx4(b, h, i, d, H, L, D)] = __float2bfloat16(a4[f][r]);
        }
      }
    }
  }
  __syncthreads();

  {  // dK, dV
    float4v ak[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    float4v av[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (f >= nfrag_d) break;
      for (int kk = 0; kk < TILE; kk += 32) {
        ak[f] = mfma_bf16(frag_load(dst, strip, kk, lane),
                          frag_load(qt, f * 16, kk, lane), ak[f]);
        av[f] = mfma_bf16(frag_load(adt, strip, kk, lane),
                          frag_load(dot, f * 16, kk, lane), av[f]);
      }
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (f >= nfrag_d) break;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int j = strip + row_grp + r;
        int d = f * 16 + col_base;
        if (j < L && d < D) {
          dk_out[idx4(b, h, j, d, H, L, D)] = __float2bfloat16(ak[f][r]);
          dv_out[idx4(b, h, j, d, H, L, D)] = __float2bfloat16(av[f][r]);
        }
      }
    }
  }

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
  torch::Tensor ts64;
  if (timestamps.has_value())
    ts64 = timestamps->to(torch::kInt64).contiguous();
  int n_time = time_table.has_value() ? time_table->size(0) : 0;
  dim3 block(256);
  dim3 grid(B * H);
  size_t smem = 4 * TILE * 128;
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL((hstu_attn_fwd_kernel<__hip_bfloat16>), grid, block,
      smem, stream,
      reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),
      reinterpret_cast<const __hip_bfloat16*>(k.data_ptr()),
      reinterpret_cast<const __hip_bfloat16*>(v.data_ptr()),
      pb.data_ptr<int>(),
      reinterpret_cast<const __hip_bfloat16*>(pos_table.data_ptr()),
      time_table.has_value()
          ? reinterpret_cast<const __hip_bfloat16*>(time_table->data_ptr())
          : nullptr,
      timestamps.has_value()
          ? reinterpret_cast<const long long*>(ts64.data_ptr())
          : nullptr,
      key_pad.has_value() ? key_pad->data_ptr<bool>() : nullptr,
      reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),
      s_saved.data_ptr<float>(), B, H, L, D, n_time);
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
  hipLaunchKernelGGL((hstu_attn_bwd_kernel<__hip_bfloat16>), grid, block,
      smem, stream,
      reinterpret_cast<const __hip_bfloat16*>(dc.data_ptr()),
      reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),
      reinterpret_cast<const __hip_bfloat16*>(k.data_ptr()),
      reinterpret_cast<const __hip_bfloat16*>(v.data_ptr()),
      s_saved.data_ptr<float>(), pb.data_ptr<int>(),
      timestamps.has_value()
          ? reinterpret_cast<const long long*>(ts64.data_ptr())
          : nullptr,
      reinterpret_cast<__hip_bfloat16*>(dq.data_ptr()),
      reinterpret_cast<__hip_bfloat16*>(dk.data_ptr()),
      reinterpret_cast<__hip_bfloat16*>(dv.data_ptr()),
      dpos.data_ptr<float>(), dtime_ptr,
      B, H, L, D, (int)n_pos, (int)n_time);
  return {dq, dk, dv, dpos, dtime};
}

}  // namespace genrec
