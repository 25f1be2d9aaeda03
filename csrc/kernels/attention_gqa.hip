// Grouped-query flash attention (bf16, softmax, D in {64,128}) for the
// Qwen2 backbone of LCRec / NoteLLM.
//
// Same fragment geometry as attention_flash.hip (64-row tiles, four waves
// that own 16 query rows each, v_mfma_f32_16x16x32_bf16, XOR-swizzled LDS
// tiles read with 16-byte fragment loads, in-register 8x8 transpose for
// the transposed operands). What a wave does with its 16-row strip of a
// tile (strip products, key columns, masking, running softmax, P stash,
// row store) is core/flash_strip.h, shared with attention_beam.hip; the
// kernels here own staging, barriers and their loops. On top of that,
// what the LLM case needs:
//
//   * query head h reads KV head h / g in-kernel (g = Hq / Hkv); K/V are
//     never expanded
//   * causal masking carries the offset Lk - Lq (prefill, cached decode,
//     chunked decode); K tiles wholly beyond the diagonal are skipped
//   * masking is exact (-inf): a masked key has probability 0, a row with
//     no visible key yields out = 0, lse = 0 and zero gradients
//   * forward saves only out + lse (O(L)); backward recomputes S per tile
//   * backward is two kernels without float atomics, so it is bitwise
//     run-to-run deterministic:
//       - gqa_bwd_dkdv: one block per (b, kv head, K tile); loops the g
//         query heads of the group in fixed order and their Q tiles,
//         accumulating dK/dV in registers
//       - gqa_bwd_dq: one block per (b, q head, Q tile); loops K tiles
//     delta = rowsum(dO * O) comes from a small pre-kernel.
//
// Layouts: q/k/v are [B,H,L,D] views with d innermost (any 8-element
// aligned batch/head/row strides, so [B,L,H,D] transposes and contiguous
// KV caches go through without a copy). out is [B,Lq,Hq,D] contiguous;
// dq/dk/dv are allocated [B,L,H,D] contiguous and returned as [B,H,L,D]
// transpose views, which is the layout the projection GEMMs' grads want.
//
// Variable-length mode (VARLEN = true; gqa_varlen_fwd / gqa_varlen_bwd):
// q/k/v are token-major [T,H,D] views of S packed sequences and cu_seqlens
// [S+1] (int32, device) gives sequence s the tokens [cu[s], cu[s+1]). A
// sequence takes the place of a batch item: blockIdx.x walks (s, head), the
// base pointers move to token cu[s], Lq = Lk = cu[s+1] - cu[s], causal. The
// tile decomposition, loop order and arithmetic of a sequence are those of
// the fixed-length kernel on that sequence alone with B = 1, so the results
// are bit-identical. The grid is sized by the host's max_seqlen; a block
// whose tile starts at or beyond its sequence's length leaves before its
// first barrier. Offsets are clamped to [0,T] and to end >= start, so no
// cu_seqlens content addresses outside the tensors. out is [T,Hq,D], lse
// and delta are [Hq,T], dq/dk/dv are [T,H,D]; all are zero-filled by the
// host, which is what tokens beyond cu[S] and empty sequences keep.

#include <ATen/hip/HIPContext.h>

#include "../core/attn_host.h"

namespace genrec {

namespace {

// GqaSeq / gqa_seq (core/flash_strip.h): the batch item or packed sequence
// a block works on.

// ------------------------------------------------------------------ forward

template <int D, bool VARLEN>
__global__ void __launch_bounds__(256)
gqa_fwd_kernel(FlashView q, FlashView k, FlashView v,
               const bool* __restrict__ key_pad,  // null | [B,Lk]
               __hip_bfloat16* __restrict__ out,  // [B,Lq,Hq,D] | [T,Hq,D]
               float* __restrict__ lse,           // [B,Hq,Lq] | [Hq,T]
               int Hq, int Hkv, int Lq, int Lk, float scale, bool causal,
               const int* __restrict__ cu, int T) {  // VARLEN only
  constexpr int RS = D * 2;
  const int b = blockIdx.x / Hq, h = blockIdx.x % Hq;
  const int hk = h / (Hq / Hkv);
  const int q0 = blockIdx.y * TILE;
  const GqaSeq<VARLEN> sq = gqa_seq<VARLEN>(cu, T, b, Lq, Lk, q0);
  if (!sq.work) return;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qs = smem;               // [64][D]   Q rows
  char* ks = qs + TILE * RS;     // [64][D]   K rows (per tile)
  char* vt = ks + TILE * RS;     // [D][64]   V^T (per tile)
  char* ps = vt + D * 128;       // [64][64]  P (per tile)

  const int tid = threadIdx.x;
  const Strip w(tid);

  gstage<D, true, false>(sq.rows(q, h), q.l, q0, sq.Lq, qs, nullptr, tid);

  RunningSoftmax sm;
  float4v accO[D / 16] = {};

  const CausalMask visible(q0, sq.Lq, sq.Lk, causal, w);
  const int kt_end = visible.kt_end(q0, sq.Lk);
  const __hip_bfloat16* kb = sq.rows(k, hk);
  const __hip_bfloat16* vb = sq.rows(v, hk);
  const bool* pad = key_pad ? key_pad + (int64_t)b * sq.Lk : nullptr;

  for (int kt0 = 0; kt0 < kt_end; kt0 += TILE) {
    __syncthreads();  // previous iteration's ks/vt fully consumed
    gstage<D, true, false>(kb, k.l, kt0, sq.Lk, ks, nullptr, tid);
    gstage<D, false, true>(vb, v.l, kt0, sq.Lk, nullptr, vt, tid);
    __syncthreads();
    flash_fwd_tile<D>(qs, ks, vt, ps, kt0, sq.Lk, pad, visible, scale, sm, accO,
                      w);
  }

  float inv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) inv[r] = sm.inv(r);
  strip_store<D>(out, sq.tok0(sq.Lq), Hq, h, q0, sq.Lq, accO, w, inv);
  if (w.col == 0) {
    const int64_t rowb = sq.rowb(h, Hq, T);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = q0 + w.row + r;
      if (i < sq.Lq) lse[rowb + i] = sm.lse(r);
    }
  }
}

// ------------------------------------------------- delta = rowsum(dO * O)

template <int D>
__global__ void __launch_bounds__(256)
gqa_delta_kernel(FlashView dout,                          // [B,Lq,Hq,D] view
                 const __hip_bfloat16* __restrict__ out,  // [B,Lq,Hq,D]
                 float* __restrict__ delta,               // [B,Hq,Lq]
                 int Hq, int Lq, int64_t n_rows) {
  constexpr int GRP = D / 8;  // lanes per row
  const int64_t row = (int64_t)blockIdx.x * (256 / GRP) + threadIdx.x / GRP;
  const int c = (threadIdx.x % GRP) * 8;
  float acc = 0.f;
  if (row < n_rows) {
    int i = row % Lq;
    int64_t bh = row / Lq;
    int h = bh % Hq;
    int64_t b = bh / Hq;
    short8v a = *reinterpret_cast<const short8v*>(
        &dout.p[b * dout.b + (int64_t)h * dout.h + (int64_t)i * dout.l + c]);
    short8v o = *reinterpret_cast<const short8v*>(
        &out[((b * Lq + i) * Hq + h) * D + c]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      acc += __uint_as_float(((unsigned int)(unsigned short)a[e]) << 16) *
             __uint_as_float(((unsigned int)(unsigned short)o[e]) << 16);
    }
  }
#pragma unroll
  for (int o = 1; o < GRP; o <<= 1) acc += __shfl_xor(acc, o, 64);
  if (row < n_rows && c == 0) delta[row] = acc;
}

// ------------------------ backward: what both kernels do after S and dP

// lse and delta of the lane's four rows of the Q tile at q0 (0 beyond Lq)
struct GqaRowStats {
  float lse[4], dl[4];
};
__device__ __forceinline__ GqaRowStats gqa_row_stats(
    const float* __restrict__ lse, const float* __restrict__ delta,
    int64_t rowb, int q0, int Lq, const Strip& w) {
  GqaRowStats st;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int i = q0 + w.row + r;
    st.lse[r] = i < Lq ? lse[rowb + i] : 0.f;
    st.dl[r] = i < Lq ? delta[rowb + i] : 0.f;
  }
  return st;
}

// P and scale*dS of fragment f of a strip, from the strip's S = Q K_t^T
// (acc) and dP = dO V_t^T (accp) accumulators. p = exp(s - lse) for visible
// keys, exactly 0 for masked ones. The softmax Jacobian carries p (1 - p): a
// probability that rounds to 1 (a row with one visible key, e.g. row 0 of
// every prefill) has dS = 0, where dP - delta would leave the rounding
// difference between the MFMA dot product and the delta pre-kernel's sum.
__device__ __forceinline__ void gqa_p_ds(int f, const float4v (&acc)[4],
                                         const float4v (&accp)[4],
                                         const KeyCols& kc,
                                         const CausalMask& visible,
                                         const GqaRowStats& st, float scale,
                                         float (&p)[4], float (&ds)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float s = __fmul_rn(acc[f][r], scale);  // as forward: no fma
    p[r] = visible(kc, f, r) ? __expf(s - st.lse[r]) : 0.f;
    ds[r] = (p[r] == 1.0f) ? 0.f : p[r] * (accp[f][r] - st.dl[r]) * scale;
  }
}

// ------------------------------------------------------- backward: dK, dV

template <int D, bool VARLEN>
__global__ void __launch_bounds__(256)
gqa_bwd_dkdv_kernel(FlashView dout, FlashView q, FlashView k, FlashView v,
                    const float* __restrict__ lse,    // [B,Hq,Lq]
                    const float* __restrict__ delta,  // [B,Hq,Lq]
                    const bool* __restrict__ key_pad,
                    __hip_bfloat16* __restrict__ dk,  // [B,Lk,Hkv,D]
                    __hip_bfloat16* __restrict__ dv,  // [B,Lk,Hkv,D]
                    int Hq, int Hkv, int Lq, int Lk, float scale, bool causal,
                    const int* __restrict__ cu, int T) {  // VARLEN only
  constexpr int RS = D * 2;
  const int b = blockIdx.x / Hkv, hk = blockIdx.x % Hkv;
  const int grp = Hq / Hkv;
  const int kt0 = blockIdx.y * TILE;
  const GqaSeq<VARLEN> sq = gqa_seq<VARLEN>(cu, T, b, Lq, Lk, kt0);
  if (!sq.work) return;
  const int off = sq.Lk - sq.Lq;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ks = smem;                // [64][D]  K_t rows (persistent)
  char* vs = ks + TILE * RS;      // [64][D]  V_t rows (persistent)
  char* qs = vs + TILE * RS;      // [64][D]  Q rows (per q-tile)
  char* dos = qs + TILE * RS;     // [64][D]  dO rows (per q-tile)
  char* qt = dos + TILE * RS;     // [D][64]  Q^T
  char* dot = qt + D * 128;       // [D][64]  dO^T
  char* dst = dot + D * 128;      // [64 j][64 i]  (scale*dS)^T
  char* pt = dst + TILE * 128;    // [64 j][64 i]  P^T

  const int tid = threadIdx.x;
  const Strip w(tid);

  gstage<D, true, false>(sq.rows(k, hk), k.l, kt0, sq.Lk, ks, nullptr, tid);
  gstage<D, true, false>(sq.rows(v, hk), v.l, kt0, sq.Lk, vs, nullptr, tid);

  const KeyCols kc = key_cols(
      kt0, sq.Lk, key_pad ? key_pad + (int64_t)b * sq.Lk : nullptr, w);

  float4v acck[D / 16] = {}, accv[D / 16] = {};

  // Q tiles whose every row sits before this K tile see none of it
  int q_begin = 0;
  if (causal && kt0 - off > 0) q_begin = ((kt0 - off) / TILE) * TILE;

  for (int hh = 0; hh < grp; ++hh) {
    const int h = hk * grp + hh;
    const __hip_bfloat16* qb = sq.rows(q, h);
    const __hip_bfloat16* dob = sq.rows(dout, h);
    const int64_t rowb = sq.rowb(h, Hq, T);
    for (int q0 = q_begin; q0 < sq.Lq; q0 += TILE) {
      __syncthreads();  // previous tile's qs/dos/qt/dot/dst/pt consumed
      gstage<D, true, true>(qb, q.l, q0, sq.Lq, qs, qt, tid);
      gstage<D, true, true>(dob, dout.l, q0, sq.Lq, dos, dot, tid);
      __syncthreads();

      const GqaRowStats st = gqa_row_stats(lse, delta, rowb, q0, sq.Lq, w);
      const CausalMask visible(q0, sq.Lq, sq.Lk, causal, w);

      // ---- S = Q K_t^T, dP = dO V_t^T (rows = this wave's q strip)
      float4v acc[4] = {}, accp[4] = {};
      strip_mma2<D, 4, RS>(acc, qs, ks, accp, dos, vs, w);

      // ---- P^T and (scale*dS)^T tiles: the lane's 4 rows are 4 adjacent
      // columns of the transposed image, one 8-byte store each
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        float p[4], ds[4];
        gqa_p_ds(f, acc, accp, kc, visible, st, scale, p, ds);
        short4v ppack, dpack;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ppack[r] = bf16_bits(p[r]);
          dpack[r] = bf16_bits(ds[r]);
        }
        tile_store(pt, f * 16 + w.col, w.row, ppack);
        tile_store(dst, f * 16 + w.col, w.row, dpack);
      }
      __syncthreads();  // pt/dst complete across waves

      // ---- dK_t += (scale*dS)^T Q ; dV_t += P^T dO (rows = k strip)
      strip_mma2<TILE, D / 16, 128>(acck, dst, qt, accv, pt, dot, w);
    }
  }

  strip_store<D>(dk, sq.tok0(sq.Lk), Hkv, hk, kt0, sq.Lk, acck, w);
  strip_store<D>(dv, sq.tok0(sq.Lk), Hkv, hk, kt0, sq.Lk, accv, w);
}

// ----------------------------------------------------------- backward: dQ

template <int D, bool VARLEN>
__global__ void __launch_bounds__(256)
gqa_bwd_dq_kernel(FlashView dout, FlashView q, FlashView k, FlashView v,
                  const float* __restrict__ lse,
                  const float* __restrict__ delta,
                  const bool* __restrict__ key_pad,
                  __hip_bfloat16* __restrict__ dq,  // [B,Lq,Hq,D]
                  int Hq, int Hkv, int Lq, int Lk, float scale, bool causal,
                  const int* __restrict__ cu, int T) {  // VARLEN only
  constexpr int RS = D * 2;
  const int b = blockIdx.x / Hq, h = blockIdx.x % Hq;
  const int hk = h / (Hq / Hkv);
  const int q0 = blockIdx.y * TILE;
  const GqaSeq<VARLEN> sq = gqa_seq<VARLEN>(cu, T, b, Lq, Lk, q0);
  if (!sq.work) return;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qs = smem;                // [64][D]  Q rows (persistent)
  char* dos = qs + TILE * RS;     // [64][D]  dO rows (persistent)
  char* ks = dos + TILE * RS;     // [64][D]  K_t rows (per tile)
  char* vs = ks + TILE * RS;      // [64][D]  V_t rows (per tile)
  char* kt = vs + TILE * RS;      // [D][64]  K_t^T
  char* dsn = kt + D * 128;       // [64 i][64 j]  scale*dS

  const int tid = threadIdx.x;
  const Strip w(tid);

  gstage<D, true, false>(sq.rows(q, h), q.l, q0, sq.Lq, qs, nullptr, tid);
  gstage<D, true, false>(sq.rows(dout, h), dout.l, q0, sq.Lq, dos, nullptr,
                         tid);

  const GqaRowStats st =
      gqa_row_stats(lse, delta, sq.rowb(h, Hq, T), q0, sq.Lq, w);

  float4v accq[D / 16] = {};

  const CausalMask visible(q0, sq.Lq, sq.Lk, causal, w);
  const int kt_end = visible.kt_end(q0, sq.Lk);
  const __hip_bfloat16* kb = sq.rows(k, hk);
  const __hip_bfloat16* vb = sq.rows(v, hk);
  const bool* pad = key_pad ? key_pad + (int64_t)b * sq.Lk : nullptr;

  for (int kt0 = 0; kt0 < kt_end; kt0 += TILE) {
    __syncthreads();  // previous tile's ks/vs/kt consumed
    gstage<D, true, true>(kb, k.l, kt0, sq.Lk, ks, kt, tid);
    gstage<D, true, false>(vb, v.l, kt0, sq.Lk, vs, nullptr, tid);
    __syncthreads();

    float4v acc[4] = {}, accp[4] = {};
    strip_mma2<D, 4, RS>(acc, qs, ks, accp, dos, vs, w);

    // ---- dQ += (scale*dS) K_t through the wave's rows of dsn
    const KeyCols kc = key_cols(kt0, sq.Lk, pad, w);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      float p[4], ds[4];
      gqa_p_ds(f, acc, accp, kc, visible, st, scale, p, ds);
      strip_stash(dsn, f, ds, w);
    }
    __builtin_amdgcn_wave_barrier();
    strip_mma<TILE, D / 16, 128, 128>(accq, dsn, kt, w);
    __builtin_amdgcn_wave_barrier();
  }

  strip_store<D>(dq, sq.tok0(sq.Lq), Hq, h, q0, sq.Lq, accq, w);
}

// ------------------------------------------------------------------ hosts

struct GqaShape {
  int B, Hq, Hkv, Lq, Lk, D;
};

GqaShape gqa_check(const torch::Tensor& q, const torch::Tensor& k,
                   const torch::Tensor& v,
                   const c10::optional<torch::Tensor>& key_pad) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda(),
              "gqa_attn: q/k/v must be GPU tensors");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
                  k.scalar_type() == torch::kBFloat16 &&
                  v.scalar_type() == torch::kBFloat16,
              "gqa_attn: q/k/v must be bfloat16");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4,
              "gqa_attn: q/k/v must be [B,H,L,D]");
  GqaShape s;
  s.B = q.size(0); s.Hq = q.size(1); s.Lq = q.size(2); s.D = q.size(3);
  s.Hkv = k.size(1); s.Lk = k.size(2);
  TORCH_CHECK(s.D == 64 || s.D == 128,
              "gqa_attn: head dim must be 64 or 128, got ", s.D);
  TORCH_CHECK(k.size(0) == s.B && k.size(3) == s.D && v.sizes() == k.sizes(),
              "gqa_attn: k/v must be [B,Hkv,Lk,D] matching q");
  TORCH_CHECK(s.Hkv >= 1 && s.Hq % s.Hkv == 0,
              "gqa_attn: Hq (", s.Hq, ") must be a multiple of Hkv (", s.Hkv,
              ")");
  TORCH_CHECK(s.B >= 1 && s.Lq >= 1 && s.Lk >= 1,
              "gqa_attn: empty batch or sequence");
  TORCH_CHECK((int64_t)(s.Lq + TILE - 1) / TILE <= 65535 &&
                  (int64_t)(s.Lk + TILE - 1) / TILE <= 65535,
              "gqa_attn: sequence too long");
  if (key_pad.has_value()) {
    TORCH_CHECK(key_pad->is_cuda() &&
                    key_pad->scalar_type() == torch::kBool &&
                    key_pad->dim() == 2 && key_pad->size(0) == s.B &&
                    key_pad->size(1) == s.Lk,
                "gqa_attn: key_pad must be a bool [B,Lk] GPU tensor");
  }
  return s;
}

// Kernels at or above 64 KiB of dynamic LDS raise their limit once.
template <typename K>
void gqa_allow_lds(K kernel, size_t smem, bool* done) {
  if (smem >= 64 * 1024 && !*done) {
    C10_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    *done = true;
  }
}

constexpr int kMaxDev = 64;

// q/k/v as the kernels take them: [B,H,L,D], or packed [T,H,D] when VARLEN
template <bool VARLEN>
FlashView gqa_view(const torch::Tensor& t) {
  return VARLEN ? view_thd(t) : view_bhld(t);
}

// s.B counts sequences and s.Lq = s.Lk = max_seqlen when VARLEN; cu/T are
// then the device offsets and the token count, else null/0.
template <int D, bool VARLEN>
void gqa_launch_fwd(const GqaShape& s, const torch::Tensor& q,
                    const torch::Tensor& k, const torch::Tensor& v,
                    const bool* kp, torch::Tensor& out, torch::Tensor& lse,
                    float scale, bool causal, const int* cu = nullptr,
                    int T = 0) {
  dim3 grid(s.B * s.Hq, (s.Lq + TILE - 1) / TILE);
  size_t smem = 2 * TILE * D * 2 + D * 128 + TILE * 128;
  static bool done[kMaxDev] = {};
  gqa_allow_lds(gqa_fwd_kernel<D, VARLEN>, smem,
                &done[q.get_device() % kMaxDev]);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL((gqa_fwd_kernel<D, VARLEN>), grid, dim3(256), smem,
      stream, gqa_view<VARLEN>(q), gqa_view<VARLEN>(k), gqa_view<VARLEN>(v),
      kp, bf16_ptr(out), lse.data_ptr<float>(), s.Hq, s.Hkv, s.Lq, s.Lk,
      scale, causal, cu, T);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

template <int D, bool VARLEN>
void gqa_launch_bwd(const GqaShape& s, const torch::Tensor& dout,
                    const torch::Tensor& q, const torch::Tensor& k,
                    const torch::Tensor& v, const torch::Tensor& out,
                    const torch::Tensor& lse, const bool* kp,
                    torch::Tensor& delta, torch::Tensor& dq,
                    torch::Tensor& dk, torch::Tensor& dv, float scale,
                    bool causal, const int* cu = nullptr, int T = 0) {
  auto stream = at::cuda::getCurrentHIPStream();
  const int dev = q.get_device() % kMaxDev;
  // dout arrives as [B,Lq,Hq,D] | [T,Hq,D]
  const FlashView dov = VARLEN ? view_thd(dout) : view_blhd(dout),
                  qv = gqa_view<VARLEN>(q), kv = gqa_view<VARLEN>(k),
                  vv = gqa_view<VARLEN>(v);
  {
    // packed sequences: the [T,Hq,D] rows are one batch item of T rows
    // (delta is per row, so sequence boundaries do not matter to it)
    constexpr int rows_per_block = 256 / (D / 8);
    const int dl_L = VARLEN ? T : s.Lq;
    int64_t n_rows = (int64_t)(VARLEN ? 1 : s.B) * s.Hq * dl_L;
    dim3 grid((unsigned int)((n_rows + rows_per_block - 1) / rows_per_block));
    hipLaunchKernelGGL(gqa_delta_kernel<D>, grid, dim3(256), 0, stream, dov,
        bf16_cptr(out), delta.data_ptr<float>(), s.Hq, dl_L, n_rows);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  {
    dim3 grid(s.B * s.Hkv, (s.Lk + TILE - 1) / TILE);
    size_t smem = 4 * TILE * D * 2 + 2 * D * 128 + 2 * TILE * 128;
    static bool done[kMaxDev] = {};
    gqa_allow_lds(gqa_bwd_dkdv_kernel<D, VARLEN>, smem, &done[dev]);
    hipLaunchKernelGGL((gqa_bwd_dkdv_kernel<D, VARLEN>), grid, dim3(256),
        smem, stream, dov, qv, kv, vv, lse.data_ptr<float>(),
        delta.data_ptr<float>(), kp, bf16_ptr(dk), bf16_ptr(dv),
        s.Hq, s.Hkv, s.Lq, s.Lk, scale, causal, cu, T);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  {
    dim3 grid(s.B * s.Hq, (s.Lq + TILE - 1) / TILE);
    size_t smem = 4 * TILE * D * 2 + D * 128 + TILE * 128;
    static bool done[kMaxDev] = {};
    gqa_allow_lds(gqa_bwd_dq_kernel<D, VARLEN>, smem, &done[dev]);
    hipLaunchKernelGGL((gqa_bwd_dq_kernel<D, VARLEN>), grid, dim3(256), smem,
        stream, dov, qv, kv, vv, lse.data_ptr<float>(),
        delta.data_ptr<float>(), kp, bf16_ptr(dq),
        s.Hq, s.Hkv, s.Lq, s.Lk, scale, causal, cu, T);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
}

// ---- packed sequences

// s.B = number of sequences, s.Lq = s.Lk = max_seqlen; returns T
int gqa_varlen_check(const torch::Tensor& q, const torch::Tensor& k,
                     const torch::Tensor& v, const torch::Tensor& cu,
                     int64_t max_seqlen, GqaShape* s) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda() && cu.is_cuda(),
              "gqa_varlen: q/k/v/cu_seqlens must be GPU tensors");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
                  k.scalar_type() == torch::kBFloat16 &&
                  v.scalar_type() == torch::kBFloat16,
              "gqa_varlen: q/k/v must be bfloat16");
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3,
              "gqa_varlen: q/k/v must be [T,H,D]");
  TORCH_CHECK(cu.scalar_type() == torch::kInt32 && cu.dim() == 1 &&
                  cu.size(0) >= 1 && cu.is_contiguous(),
              "gqa_varlen: cu_seqlens must be a contiguous int32 [S+1] "
              "tensor");
  const int64_t T = q.size(0);
  s->B = (int)(cu.size(0) - 1);
  s->Hq = q.size(1); s->D = q.size(2); s->Hkv = k.size(1);
  TORCH_CHECK(s->D == 64 || s->D == 128,
              "gqa_varlen: head dim must be 64 or 128, got ", s->D);
  TORCH_CHECK(k.size(0) == T && k.size(2) == s->D && v.sizes() == k.sizes(),
              "gqa_varlen: k/v must be [T,Hkv,D] matching q");
  TORCH_CHECK(s->Hkv >= 1 && s->Hq % s->Hkv == 0,
              "gqa_varlen: Hq (", s->Hq, ") must be a multiple of Hkv (",
              s->Hkv, ")");
  TORCH_CHECK(T < (int64_t)1 << 31, "gqa_varlen: too many tokens");
  TORCH_CHECK(max_seqlen >= 0 && (max_seqlen + TILE - 1) / TILE <= 65535,
              "gqa_varlen: max_seqlen out of range");
  TORCH_CHECK((int64_t)s->B * s->Hq < (int64_t)1 << 31,
              "gqa_varlen: too many sequences");
  s->Lq = s->Lk = (int)max_seqlen;
  return (int)T;
}

}  // namespace

std::vector<torch::Tensor> gqa_attn_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    c10::optional<torch::Tensor> key_pad, double scale, bool causal) {
  GqaShape s = gqa_check(q, k, v, key_pad);
  // [B,H,L,D]: batch, head and row strides
  torch::Tensor qn = kernel_readable(q, 3), kn = kernel_readable(k, 3),
                vn = kernel_readable(v, 3);
  torch::Tensor kpc;
  const bool* kp = pad_ptr(key_pad, kpc);
  auto out = torch::empty({s.B, s.Lq, s.Hq, s.D}, q.options());
  auto lse = torch::empty({s.B, s.Hq, s.Lq},
                          q.options().dtype(torch::kFloat32));
  dispatch_head_dim(s.D, [&](auto d) {
    gqa_launch_fwd<decltype(d)::value, false>(s, qn, kn, vn, kp, out, lse,
                                              (float)scale, causal);
  });
  return {out, lse};
}

std::vector<torch::Tensor> gqa_attn_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse,
    c10::optional<torch::Tensor> key_pad, double scale, bool causal) {
  GqaShape s = gqa_check(q, k, v, key_pad);
  TORCH_CHECK(dout.is_cuda() && dout.scalar_type() == torch::kBFloat16 &&
                  dout.dim() == 4 && dout.size(0) == s.B &&
                  dout.size(1) == s.Lq && dout.size(2) == s.Hq &&
                  dout.size(3) == s.D,
              "gqa_attn_bwd: dout must be bf16 [B,Lq,Hq,D]");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 &&
                  out.sizes() == dout.sizes() && out.is_contiguous(),
              "gqa_attn_bwd: out must be the contiguous forward output");
  TORCH_CHECK(lse.scalar_type() == torch::kFloat32 && lse.is_contiguous() &&
                  lse.dim() == 3 && lse.size(0) == s.B &&
                  lse.size(1) == s.Hq && lse.size(2) == s.Lq,
              "gqa_attn_bwd: lse must be the fp32 [B,Hq,Lq] forward lse");
  torch::Tensor don = kernel_readable(dout, 3), qn = kernel_readable(q, 3),
                kn = kernel_readable(k, 3), vn = kernel_readable(v, 3);
  torch::Tensor kpc;
  const bool* kp = pad_ptr(key_pad, kpc);
  auto delta = torch::empty({s.B, s.Hq, s.Lq}, lse.options());
  // [B,L,H,D] storage, handed back as [B,H,L,D] views: the grads of the
  // q/k/v projections' .view().transpose(1,2) are then contiguous
  auto dq = torch::empty({s.B, s.Lq, s.Hq, s.D}, q.options());
  auto dk = torch::empty({s.B, s.Lk, s.Hkv, s.D}, k.options());
  auto dv = torch::empty({s.B, s.Lk, s.Hkv, s.D}, v.options());
  dispatch_head_dim(s.D, [&](auto d) {
    gqa_launch_bwd<decltype(d)::value, false>(s, don, qn, kn, vn, out, lse,
                                              kp, delta, dq, dk, dv,
                                              (float)scale, causal);
  });
  return {dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)};
}

std::vector<torch::Tensor> gqa_varlen_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor cu_seqlens, int64_t max_seqlen, double scale) {
  GqaShape s;
  const int T = gqa_varlen_check(q, k, v, cu_seqlens, max_seqlen, &s);
  // [T,H,D]: token and head strides
  torch::Tensor qn = kernel_readable(q, 2), kn = kernel_readable(k, 2),
                vn = kernel_readable(v, 2);
  // zeros: tokens of no sequence (beyond cu[S]) are never written
  auto out = torch::zeros({T, s.Hq, s.D}, q.options());
  auto lse = torch::zeros({s.Hq, T}, q.options().dtype(torch::kFloat32));
  if (T == 0 || s.B == 0 || max_seqlen == 0) return {out, lse};
  const int* cu = cu_seqlens.data_ptr<int>();
  dispatch_head_dim(s.D, [&](auto d) {
    gqa_launch_fwd<decltype(d)::value, true>(s, qn, kn, vn, nullptr, out, lse,
                                             (float)scale, true, cu, T);
  });
  return {out, lse};
}

std::vector<torch::Tensor> gqa_varlen_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, torch::Tensor cu_seqlens,
    int64_t max_seqlen, double scale) {
  GqaShape s;
  const int T = gqa_varlen_check(q, k, v, cu_seqlens, max_seqlen, &s);
  TORCH_CHECK(dout.is_cuda() && dout.scalar_type() == torch::kBFloat16 &&
                  dout.dim() == 3 && dout.size(0) == T &&
                  dout.size(1) == s.Hq && dout.size(2) == s.D,
              "gqa_varlen_bwd: dout must be bf16 [T,Hq,D]");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 &&
                  out.sizes() == dout.sizes() && out.is_contiguous(),
              "gqa_varlen_bwd: out must be the contiguous forward output");
  TORCH_CHECK(lse.scalar_type() == torch::kFloat32 && lse.is_contiguous() &&
                  lse.dim() == 2 && lse.size(0) == s.Hq && lse.size(1) == T,
              "gqa_varlen_bwd: lse must be the fp32 [Hq,T] forward lse");
  torch::Tensor don = kernel_readable(dout, 2), qn = kernel_readable(q, 2),
                kn = kernel_readable(k, 2), vn = kernel_readable(v, 2);
  auto dq = torch::zeros({T, s.Hq, s.D}, q.options());
  auto dk = torch::zeros({T, s.Hkv, s.D}, k.options());
  auto dv = torch::zeros({T, s.Hkv, s.D}, v.options());
  if (T == 0 || s.B == 0 || max_seqlen == 0) return {dq, dk, dv};
  auto delta = torch::empty({s.Hq, T}, lse.options());
  const int* cu = cu_seqlens.data_ptr<int>();
  dispatch_head_dim(s.D, [&](auto d) {
    gqa_launch_bwd<decltype(d)::value, true>(s, don, qn, kn, vn, out, lse,
                                             nullptr, delta, dq, dk, dv,
                                             (float)scale, true, cu, T);
  });
  return {dq, dk, dv};
}

}  // namespace genrec
