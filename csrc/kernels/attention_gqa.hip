// Grouped-query flash attention (bf16, softmax, D in {64,128}) for the
// Qwen2 backbone of LCRec / NoteLLM.
//
// Same fragment geometry as attention_flash.hip (64-row tiles, four waves
// that own 16 query rows each, v_mfma_f32_16x16x32_bf16, XOR-swizzled LDS
// tiles read with 16-byte fragment loads, in-register 8x8 transpose for
// the transposed operands), with what the LLM case needs on top:
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

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../core/mfma_tile.h"

namespace genrec {

namespace {

// Token range of packed sequence s, clamped so that it lies inside [0,T].
__device__ __forceinline__ void gqa_seq_range(const int* __restrict__ cu,
                                              int s, int T, int* start,
                                              int* len) {
  const int a = min(max(cu[s], 0), T);
  const int e = min(max(cu[s + 1], a), T);
  *start = a;
  *len = e - a;
}

// ------------------------------------------------------------------ forward

template <int D, bool VARLEN>
__global__ void __launch_bounds__(256)
gqa_fwd_kernel(const __hip_bfloat16* __restrict__ q,
               const __hip_bfloat16* __restrict__ k,
               const __hip_bfloat16* __restrict__ v,
               const bool* __restrict__ key_pad,  // null | [B,Lk]
               __hip_bfloat16* __restrict__ out,  // [B,Lq,Hq,D] | [T,Hq,D]
               float* __restrict__ lse,           // [B,Hq,Lq] | [Hq,T]
               int Hq, int Hkv, int Lq, int Lk, float scale, bool causal,
               int64_t q_sb, int64_t q_sh, int64_t q_sl,
               int64_t k_sb, int64_t k_sh, int64_t k_sl,
               int64_t v_sb, int64_t v_sh, int64_t v_sl,
               const int* __restrict__ cu, int T) {  // VARLEN only
  constexpr int RS = D * 2;
  const int b = blockIdx.x / Hq, h = blockIdx.x % Hq;
  const int hk = h / (Hq / Hkv);
  const int q0 = blockIdx.y * TILE;
  int64_t tok0, rowb;  // first out row of b; first lse entry of (b, h)
  if constexpr (VARLEN) {
    int start;
    gqa_seq_range(cu, b, T, &start, &Lq);
    Lk = Lq;
    if (q0 >= Lq) return;  // uniform per block, before any barrier
    q_sb = k_sb = v_sb = 0;  // the sequence's base is its first token
    q += (int64_t)start * q_sl;
    k += (int64_t)start * k_sl;
    v += (int64_t)start * v_sl;
    tok0 = start;
    rowb = (int64_t)h * T + start;
  } else {
    tok0 = (int64_t)b * Lq;
    rowb = ((int64_t)b * Hq + h) * Lq;
  }
  const int off = Lk - Lq;  // query row i sits at absolute position i + off

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qs = smem;               // [64][D]   Q rows
  char* ks = qs + TILE * RS;     // [64][D]   K rows (per tile)
  char* vt = ks + TILE * RS;     // [D][64]   V^T (per tile)
  char* ps = vt + D * 128;       // [64][64]  P (per tile)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col_base = frag_col(lane);
  const int row_grp = frag_row0(lane);
  const int strip = wid * 16;

  gstage<D, true, false>(q + (int64_t)b * q_sb + (int64_t)h * q_sh, q_sl, q0,
                         Lq, qs, nullptr, tid);

  float m_row[4], l_row[4];
  float4v accO[D / 16];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_row[r] = -INFINITY; l_row[r] = 0.f; }
#pragma unroll
  for (int f = 0; f < D / 16; ++f) accO[f] = float4v{0, 0, 0, 0};

  // K tiles wholly beyond the diagonal of this Q tile are skipped
  int kt_end = Lk;
  if (causal) kt_end = min(Lk, q0 + TILE + off);
  const __hip_bfloat16* kb = k + (int64_t)b * k_sb + (int64_t)hk * k_sh;
  const __hip_bfloat16* vb = v + (int64_t)b * v_sb + (int64_t)hk * v_sh;

  for (int kt0 = 0; kt0 < kt_end; kt0 += TILE) {
    __syncthreads();  // previous iteration's ks/vt fully consumed
    gstage<D, true, false>(kb, k_sl, kt0, Lk, ks, nullptr, tid);
    gstage<D, false, true>(vb, v_sl, kt0, Lk, nullptr, vt, tid);
    __syncthreads();

    // ---- S = Q K_t^T
    float4v acc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      acc[f] = float4v{0, 0, 0, 0};
#pragma unroll
      for (int kk = 0; kk < D; kk += 32) {
        acc[f] = mfma_bf16(frag_load(qs, strip, kk, lane, RS),
                           frag_load(ks, f * 16, kk, lane, RS), acc[f]);
      }
    }

    // ---- exact masking (-inf)
    float s_val[4][4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      int j = kt0 + f * 16 + col_base;
      bool jok = j < Lk;
      if (jok && key_pad) jok = !key_pad[(int64_t)b * Lk + j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i = q0 + strip + row_grp + r;
        bool ok = jok && i < Lq && !(causal && j > i + off);
        s_val[f][r] = ok ? __fmul_rn(acc[f][r], scale) : -INFINITY;
      }
    }

    // ---- running softmax; a row whose keys so far are all masked keeps
    // m = -inf, l = 0 and contributes nothing (no exp(-inf - -inf))
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float tmax = grp16_max(fmaxf(fmaxf(s_val[0][r], s_val[1][r]),
                                   fmaxf(s_val[2][r], s_val[3][r])));
      float m_new = fmaxf(m_row[r], tmax);
      bool dead = (m_new == -INFINITY);
      float a = (dead || m_row[r] == -INFINITY) ? (dead ? 1.f : 0.f)
                                                : __expf(m_row[r] - m_new);
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
#pragma unroll
      for (int f = 0; f < D / 16; ++f) accO[f][r] *= a;
    }

    // ---- stash P (this wave's 16 rows only)
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        tile_store(ps, strip + row_grp + r, f * 16 + col_base,
                   bf16_bits(s_val[f][r]));
      }
    }
    __builtin_amdgcn_wave_barrier();

    // ---- accO += P V_t
#pragma unroll
    for (int f = 0; f < D / 16; ++f) {
#pragma unroll
      for (int kk = 0; kk < TILE; kk += 32) {
        accO[f] = mfma_bf16(frag_load(ps, strip, kk, lane),
                            frag_load(vt, f * 16, kk, lane), accO[f]);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

  // ---- finalize
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int i = q0 + strip + row_grp + r;
    if (i >= Lq) continue;
    float inv = (l_row[r] > 0.f) ? 1.0f / l_row[r] : 0.f;
    int64_t ob = ((tok0 + i) * Hq + h) * D;
#pragma unroll
    for (int f = 0; f < D / 16; ++f) {
      out[ob + f * 16 + col_base] = __float2bfloat16(accO[f][r] * inv);
    }
    if (col_base == 0) {
      lse[rowb + i] =
          (l_row[r] > 0.f) ? m_row[r] + __logf(l_row[r]) : 0.f;
    }
  }
}

// ------------------------------------------------- delta = rowsum(dO * O)

template <int D>
__global__ void __launch_bounds__(256)
gqa_delta_kernel(const __hip_bfloat16* __restrict__ dout,  // [B,Lq,Hq,D] view
                 const __hip_bfloat16* __restrict__ out,   // [B,Lq,Hq,D]
                 float* __restrict__ delta,                // [B,Hq,Lq]
                 int Hq, int Lq, int64_t n_rows,
                 int64_t do_sb, int64_t do_sh, int64_t do_sl) {
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
        &dout[b * do_sb + (int64_t)h * do_sh + (int64_t)i * do_sl + c]);
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

// Recompute P and dS for one 16x64 strip from the S and dP accumulators.
// p = exp(s - lse) for visible keys, exactly 0 for masked ones. The
// softmax Jacobian carries p (1 - p): a probability that rounds to 1 (a row
// with one visible key, e.g. row 0 of every prefill) has dS = 0, where
// dP - delta would leave the rounding difference between the MFMA dot
// product and the delta pre-kernel's sum.
#define GQA_P_DS(f, r, p_out, ds_out)                                      \
  {                                                                        \
    int i_ = q0 + strip + row_grp + (r);                                   \
    bool ok_ = jok[f] && i_ < Lq && !(causal && jcol[f] > i_ + off);       \
    float s_ = __fmul_rn(acc[f][r], scale); /* as forward: no fma */       \
    float p_ = ok_ ? __expf(s_ - lse_r[r]) : 0.f;                          \
    p_out = p_;                                                            \
    ds_out = (p_ == 1.0f) ? 0.f : p_ * (accp[f][r] - dl_r[r]) * scale;     \
  }

// ------------------------------------------------------- backward: dK, dV

template <int D, bool VARLEN>
__global__ void __launch_bounds__(256)
gqa_bwd_dkdv_kernel(const __hip_bfloat16* __restrict__ dout,
                    const __hip_bfloat16* __restrict__ q,
                    const __hip_bfloat16* __restrict__ k,
                    const __hip_bfloat16* __restrict__ v,
                    const float* __restrict__ lse,    // [B,Hq,Lq]
                    const float* __restrict__ delta,  // [B,Hq,Lq]
                    const bool* __restrict__ key_pad,
                    __hip_bfloat16* __restrict__ dk,  // [B,Lk,Hkv,D]
                    __hip_bfloat16* __restrict__ dv,  // [B,Lk,Hkv,D]
                    int Hq, int Hkv, int Lq, int Lk, float scale, bool causal,
                    int64_t do_sb, int64_t do_sh, int64_t do_sl,
                    int64_t q_sb, int64_t q_sh, int64_t q_sl,
                    int64_t k_sb, int64_t k_sh, int64_t k_sl,
                    int64_t v_sb, int64_t v_sh, int64_t v_sl,
                    const int* __restrict__ cu, int T) {  // VARLEN only
  constexpr int RS = D * 2;
  const int b = blockIdx.x / Hkv, hk = blockIdx.x % Hkv;
  const int grp = Hq / Hkv;
  const int kt0 = blockIdx.y * TILE;
  int64_t tok0 = (int64_t)b * Lk;  // first dk/dv row of b
  int start = 0;
  if constexpr (VARLEN) {
    gqa_seq_range(cu, b, T, &start, &Lq);
    Lk = Lq;
    if (kt0 >= Lk) return;  // uniform per block, before any barrier
    do_sb = q_sb = k_sb = v_sb = 0;
    dout += (int64_t)start * do_sl;
    q += (int64_t)start * q_sl;
    k += (int64_t)start * k_sl;
    v += (int64_t)start * v_sl;
    tok0 = start;
  }
  const int off = Lk - Lq;

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
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col_base = frag_col(lane);
  const int row_grp = frag_row0(lane);
  const int strip = wid * 16;
  const int i0g = strip + row_grp;  // 8-byte aligned store base

  gstage<D, true, false>(k + (int64_t)b * k_sb + (int64_t)hk * k_sh, k_sl,
                         kt0, Lk, ks, nullptr, tid);
  gstage<D, true, false>(v + (int64_t)b * v_sb + (int64_t)hk * v_sh, v_sl,
                         kt0, Lk, vs, nullptr, tid);

  int jcol[4];
  bool jok[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    jcol[f] = kt0 + f * 16 + col_base;
    jok[f] = jcol[f] < Lk;
    if (jok[f] && key_pad) jok[f] = !key_pad[(int64_t)b * Lk + jcol[f]];
  }

  float4v acck[D / 16], accv[D / 16];
#pragma unroll
  for (int f = 0; f < D / 16; ++f) {
    acck[f] = float4v{0, 0, 0, 0};
    accv[f] = float4v{0, 0, 0, 0};
  }

  // Q tiles whose every row sits before this K tile see none of it
  int q_begin = 0;
  if (causal && kt0 - off > 0) q_begin = ((kt0 - off) / TILE) * TILE;

  for (int hh = 0; hh < grp; ++hh) {
    const int h = hk * grp + hh;
    const __hip_bfloat16* qb = q + (int64_t)b * q_sb + (int64_t)h * q_sh;
    const __hip_bfloat16* dob = dout + (int64_t)b * do_sb + (int64_t)h * do_sh;
    const int64_t rowb =
        VARLEN ? (int64_t)h * T + start : ((int64_t)b * Hq + h) * Lq;
    for (int q0 = q_begin; q0 < Lq; q0 += TILE) {
      __syncthreads();  // previous tile's qs/dos/qt/dot/dst/pt consumed
      gstage<D, true, true>(qb, q_sl, q0, Lq, qs, qt, tid);
      gstage<D, true, true>(dob, do_sl, q0, Lq, dos, dot, tid);
      __syncthreads();

      float lse_r[4], dl_r[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i = q0 + strip + row_grp + r;
        lse_r[r] = i < Lq ? lse[rowb + i] : 0.f;
        dl_r[r] = i < Lq ? delta[rowb + i] : 0.f;
      }

      // ---- S = Q K_t^T, dP = dO V_t^T (rows = this wave's q strip)
      float4v acc[4], accp[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        acc[f] = float4v{0, 0, 0, 0};
        accp[f] = float4v{0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < D; kk += 32) {
          acc[f] = mfma_bf16(frag_load(qs, strip, kk, lane, RS),
                             frag_load(ks, f * 16, kk, lane, RS), acc[f]);
          accp[f] = mfma_bf16(frag_load(dos, strip, kk, lane, RS),
                              frag_load(vs, f * 16, kk, lane, RS), accp[f]);
        }
      }

      // ---- P^T and (scale*dS)^T tiles
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        short4v ppack, dpack;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float pv, dsv;
          GQA_P_DS(f, r, pv, dsv);
          ppack[r] = bf16_bits(pv);
          dpack[r] = bf16_bits(dsv);
        }
        int jl = f * 16 + col_base;
        tile_store(pt, jl, i0g, ppack);
        tile_store(dst, jl, i0g, dpack);
      }
      __syncthreads();  // pt/dst complete across waves

      // ---- dK_t += (scale*dS)^T Q ; dV_t += P^T dO (rows = k strip)
#pragma unroll
      for (int f = 0; f < D / 16; ++f) {
#pragma unroll
        for (int kk = 0; kk < TILE; kk += 32) {
          acck[f] = mfma_bf16(frag_load(dst, strip, kk, lane),
                              frag_load(qt, f * 16, kk, lane), acck[f]);
          accv[f] = mfma_bf16(frag_load(pt, strip, kk, lane),
                              frag_load(dot, f * 16, kk, lane), accv[f]);
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int j = kt0 + strip + row_grp + r;
    if (j >= Lk) continue;
    int64_t ob = ((tok0 + j) * Hkv + hk) * D;
#pragma unroll
    for (int f = 0; f < D / 16; ++f) {
      dk[ob + f * 16 + col_base] = __float2bfloat16(acck[f][r]);
      dv[ob + f * 16 + col_base] = __float2bfloat16(accv[f][r]);
    }
  }
}

// ----------------------------------------------------------- backward: dQ

template <int D, bool VARLEN>
__global__ void __launch_bounds__(256)
gqa_bwd_dq_kernel(const __hip_bfloat16* __restrict__ dout,
                  const __hip_bfloat16* __restrict__ q,
                  const __hip_bfloat16* __restrict__ k,
                  const __hip_bfloat16* __restrict__ v,
                  const float* __restrict__ lse,
                  const float* __restrict__ delta,
                  const bool* __restrict__ key_pad,
                  __hip_bfloat16* __restrict__ dq,  // [B,Lq,Hq,D]
                  int Hq, int Hkv, int Lq, int Lk, float scale, bool causal,
                  int64_t do_sb, int64_t do_sh, int64_t do_sl,
                  int64_t q_sb, int64_t q_sh, int64_t q_sl,
                  int64_t k_sb, int64_t k_sh, int64_t k_sl,
                  int64_t v_sb, int64_t v_sh, int64_t v_sl,
                  const int* __restrict__ cu, int T) {  // VARLEN only
  constexpr int RS = D * 2;
  const int b = blockIdx.x / Hq, h = blockIdx.x % Hq;
  const int hk = h / (Hq / Hkv);
  const int q0 = blockIdx.y * TILE;
  int64_t tok0, rowb;  // first dq row of b; first lse/delta entry of (b, h)
  if constexpr (VARLEN) {
    int start;
    gqa_seq_range(cu, b, T, &start, &Lq);
    Lk = Lq;
    if (q0 >= Lq) return;  // uniform per block, before any barrier
    do_sb = q_sb = k_sb = v_sb = 0;
    dout += (int64_t)start * do_sl;
    q += (int64_t)start * q_sl;
    k += (int64_t)start * k_sl;
    v += (int64_t)start * v_sl;
    tok0 = start;
    rowb = (int64_t)h * T + start;
  } else {
    tok0 = (int64_t)b * Lq;
    rowb = ((int64_t)b * Hq + h) * Lq;
  }
  const int off = Lk - Lq;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qs = smem;                // [64][D]  Q rows (persistent)
  char* dos = qs + TILE * RS;     // [64][D]  dO rows (persistent)
  char* ks = dos + TILE * RS;     // [64][D]  K_t rows (per tile)
  char* vs = ks + TILE * RS;      // [64][D]  V_t rows (per tile)
  char* kt = vs + TILE * RS;      // [D][64]  K_t^T
  char* dsn = kt + D * 128;       // [64 i][64 j]  scale*dS

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col_base = frag_col(lane);
  const int row_grp = frag_row0(lane);
  const int strip = wid * 16;

  gstage<D, true, false>(q + (int64_t)b * q_sb + (int64_t)h * q_sh, q_sl, q0,
                         Lq, qs, nullptr, tid);
  gstage<D, true, false>(dout + (int64_t)b * do_sb + (int64_t)h * do_sh,
                         do_sl, q0, Lq, dos, nullptr, tid);

  float lse_r[4], dl_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int i = q0 + strip + row_grp + r;
    lse_r[r] = i < Lq ? lse[rowb + i] : 0.f;
    dl_r[r] = i < Lq ? delta[rowb + i] : 0.f;
  }

  float4v accq[D / 16];
#pragma unroll
  for (int f = 0; f < D / 16; ++f) accq[f] = float4v{0, 0, 0, 0};

  int kt_end = Lk;
  if (causal) kt_end = min(Lk, q0 + TILE + off);
  const __hip_bfloat16* kb = k + (int64_t)b * k_sb + (int64_t)hk * k_sh;
  const __hip_bfloat16* vb = v + (int64_t)b * v_sb + (int64_t)hk * v_sh;

  for (int kt0 = 0; kt0 < kt_end; kt0 += TILE) {
    __syncthreads();  // previous tile's ks/vs/kt consumed
    gstage<D, true, true>(kb, k_sl, kt0, Lk, ks, kt, tid);
    gstage<D, true, false>(vb, v_sl, kt0, Lk, vs, nullptr, tid);
    __syncthreads();

    int jcol[4];
    bool jok[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      jcol[f] = kt0 + f * 16 + col_base;
      jok[f] = jcol[f] < Lk;
      if (jok[f] && key_pad) jok[f] = !key_pad[(int64_t)b * Lk + jcol[f]];
    }

    float4v acc[4], accp[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      acc[f] = float4v{0, 0, 0, 0};
      accp[f] = float4v{0, 0, 0, 0};
#pragma unroll
      for (int kk = 0; kk < D; kk += 32) {
        acc[f] = mfma_bf16(frag_load(qs, strip, kk, lane, RS),
                           frag_load(ks, f * 16, kk, lane, RS), acc[f]);
        accp[f] = mfma_bf16(frag_load(dos, strip, kk, lane, RS),
                            frag_load(vs, f * 16, kk, lane, RS), accp[f]);
      }
    }

    // ---- scale*dS rows of this wave's strip
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pv, dsv;
        GQA_P_DS(f, r, pv, dsv);
        (void)pv;
        tile_store(dsn, strip + row_grp + r, f * 16 + col_base,
                   bf16_bits(dsv));
      }
    }
    __builtin_amdgcn_wave_barrier();

    // ---- dQ += (scale*dS) K_t
#pragma unroll
    for (int f = 0; f < D / 16; ++f) {
#pragma unroll
      for (int kk = 0; kk < TILE; kk += 32) {
        accq[f] = mfma_bf16(frag_load(dsn, strip, kk, lane),
                            frag_load(kt, f * 16, kk, lane), accq[f]);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int i = q0 + strip + row_grp + r;
    if (i >= Lq) continue;
    int64_t ob = ((tok0 + i) * Hq + h) * D;
#pragma unroll
    for (int f = 0; f < D / 16; ++f) {
      dq[ob + f * 16 + col_base] = __float2bfloat16(accq[f][r]);
    }
  }
}

#undef GQA_P_DS

// ------------------------------------------------------------------ hosts

bool gqa_ok_strides(const torch::Tensor& t) {
  return t.stride(3) == 1 && t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
         t.stride(2) % 8 == 0 &&
         reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

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

// batch / head / row strides of one operand as the kernels take them
struct GqaStrides {
  int64_t b, h, l;
};
// [B,H,L,D] view
GqaStrides gqa_bhld(const torch::Tensor& t) {
  return {t.stride(0), t.stride(1), t.stride(2)};
}
// [B,L,H,D] view (dout)
GqaStrides gqa_blhd(const torch::Tensor& t) {
  return {t.stride(0), t.stride(2), t.stride(1)};
}
// token-major [T,H,D] view of packed sequences: no batch stride
GqaStrides gqa_thd(const torch::Tensor& t) {
  return {0, t.stride(1), t.stride(0)};
}

const __hip_bfloat16* gqa_cptr(const torch::Tensor& t) {
  return reinterpret_cast<const __hip_bfloat16*>(t.data_ptr());
}
__hip_bfloat16* gqa_ptr(torch::Tensor& t) {
  return reinterpret_cast<__hip_bfloat16*>(t.data_ptr());
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
  const GqaStrides qs = VARLEN ? gqa_thd(q) : gqa_bhld(q),
                   ks = VARLEN ? gqa_thd(k) : gqa_bhld(k),
                   vs = VARLEN ? gqa_thd(v) : gqa_bhld(v);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL((gqa_fwd_kernel<D, VARLEN>), grid, dim3(256), smem,
      stream, gqa_cptr(q), gqa_cptr(k), gqa_cptr(v), kp, gqa_ptr(out),
      lse.data_ptr<float>(), s.Hq, s.Hkv, s.Lq, s.Lk, scale, causal,
      qs.b, qs.h, qs.l, ks.b, ks.h, ks.l, vs.b, vs.h, vs.l, cu, T);
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
  const __hip_bfloat16* dop = gqa_cptr(dout);
  const __hip_bfloat16* qp = gqa_cptr(q);
  const __hip_bfloat16* kp16 = gqa_cptr(k);
  const __hip_bfloat16* vp = gqa_cptr(v);
  const GqaStrides ds = VARLEN ? gqa_thd(dout) : gqa_blhd(dout),
                   qs = VARLEN ? gqa_thd(q) : gqa_bhld(q),
                   ks = VARLEN ? gqa_thd(k) : gqa_bhld(k),
                   vs = VARLEN ? gqa_thd(v) : gqa_bhld(v);
  {
    // packed sequences: the [T,Hq,D] rows are one batch item of T rows
    // (delta is per row, so sequence boundaries do not matter to it)
    constexpr int rows_per_block = 256 / (D / 8);
    const int dl_L = VARLEN ? T : s.Lq;
    int64_t n_rows = (int64_t)(VARLEN ? 1 : s.B) * s.Hq * dl_L;
    dim3 grid((unsigned int)((n_rows + rows_per_block - 1) / rows_per_block));
    hipLaunchKernelGGL(gqa_delta_kernel<D>, grid, dim3(256), 0, stream, dop,
        gqa_cptr(out), delta.data_ptr<float>(), s.Hq, dl_L, n_rows, ds.b,
        ds.h, ds.l);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  {
    dim3 grid(s.B * s.Hkv, (s.Lk + TILE - 1) / TILE);
    size_t smem = 4 * TILE * D * 2 + 2 * D * 128 + 2 * TILE * 128;
    static bool done[kMaxDev] = {};
    gqa_allow_lds(gqa_bwd_dkdv_kernel<D, VARLEN>, smem, &done[dev]);
    hipLaunchKernelGGL((gqa_bwd_dkdv_kernel<D, VARLEN>), grid, dim3(256),
        smem, stream, dop, qp, kp16, vp, lse.data_ptr<float>(),
        delta.data_ptr<float>(), kp, gqa_ptr(dk), gqa_ptr(dv),
        s.Hq, s.Hkv, s.Lq, s.Lk, scale, causal, ds.b, ds.h, ds.l,
        qs.b, qs.h, qs.l, ks.b, ks.h, ks.l, vs.b, vs.h, vs.l, cu, T);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  {
    dim3 grid(s.B * s.Hq, (s.Lq + TILE - 1) / TILE);
    size_t smem = 4 * TILE * D * 2 + D * 128 + TILE * 128;
    static bool done[kMaxDev] = {};
    gqa_allow_lds(gqa_bwd_dq_kernel<D, VARLEN>, smem, &done[dev]);
    hipLaunchKernelGGL((gqa_bwd_dq_kernel<D, VARLEN>), grid, dim3(256), smem,
        stream, dop, qp, kp16, vp, lse.data_ptr<float>(),
        delta.data_ptr<float>(), kp, gqa_ptr(dq),
        s.Hq, s.Hkv, s.Lq, s.Lk, scale, causal, ds.b, ds.h, ds.l,
        qs.b, qs.h, qs.l, ks.b, ks.h, ks.l, vs.b, vs.h, vs.l, cu, T);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
}

// ---- packed sequences

bool gqa_ok_strides_thd(const torch::Tensor& t) {
  return t.stride(2) == 1 && t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
         reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

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
  torch::Tensor qn = gqa_ok_strides(q) ? q : q.contiguous();
  torch::Tensor kn = gqa_ok_strides(k) ? k : k.contiguous();
  torch::Tensor vn = gqa_ok_strides(v) ? v : v.contiguous();
  torch::Tensor kpc;
  const bool* kp = nullptr;
  if (key_pad.has_value()) {
    kpc = key_pad->contiguous();
    kp = kpc.data_ptr<bool>();
  }
  auto out = torch::empty({s.B, s.Lq, s.Hq, s.D}, q.options());
  auto lse = torch::empty({s.B, s.Hq, s.Lq},
                          q.options().dtype(torch::kFloat32));
  if (s.D == 64) {
    gqa_launch_fwd<64, false>(s, qn, kn, vn, kp, out, lse, (float)scale, causal);
  } else {
    gqa_launch_fwd<128, false>(s, qn, kn, vn, kp, out, lse, (float)scale, causal);
  }
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
  torch::Tensor don = gqa_ok_strides(dout) ? dout : dout.contiguous();
  torch::Tensor qn = gqa_ok_strides(q) ? q : q.contiguous();
  torch::Tensor kn = gqa_ok_strides(k) ? k : k.contiguous();
  torch::Tensor vn = gqa_ok_strides(v) ? v : v.contiguous();
  torch::Tensor kpc;
  const bool* kp = nullptr;
  if (key_pad.has_value()) {
    kpc = key_pad->contiguous();
    kp = kpc.data_ptr<bool>();
  }
  auto delta = torch::empty({s.B, s.Hq, s.Lq}, lse.options());
  // [B,L,H,D] storage, handed back as [B,H,L,D] views: the grads of the
  // q/k/v projections' .view().transpose(1,2) are then contiguous
  auto dq = torch::empty({s.B, s.Lq, s.Hq, s.D}, q.options());
  auto dk = torch::empty({s.B, s.Lk, s.Hkv, s.D}, k.options());
  auto dv = torch::empty({s.B, s.Lk, s.Hkv, s.D}, v.options());
  if (s.D == 64) {
    gqa_launch_bwd<64, false>(s, don, qn, kn, vn, out, lse, kp, delta, dq, dk, dv,
                       (float)scale, causal);
  } else {
    gqa_launch_bwd<128, false>(s, don, qn, kn, vn, out, lse, kp, delta, dq, dk, dv,
                        (float)scale, causal);
  }
  return {dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)};
}

std::vector<torch::Tensor> gqa_varlen_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor cu_seqlens, int64_t max_seqlen, double scale) {
  GqaShape s;
  const int T = gqa_varlen_check(q, k, v, cu_seqlens, max_seqlen, &s);
  torch::Tensor qn = gqa_ok_strides_thd(q) ? q : q.contiguous();
  torch::Tensor kn = gqa_ok_strides_thd(k) ? k : k.contiguous();
  torch::Tensor vn = gqa_ok_strides_thd(v) ? v : v.contiguous();
  // zeros: tokens of no sequence (beyond cu[S]) are never written
  auto out = torch::zeros({T, s.Hq, s.D}, q.options());
  auto lse = torch::zeros({s.Hq, T}, q.options().dtype(torch::kFloat32));
  if (T == 0 || s.B == 0 || max_seqlen == 0) return {out, lse};
  const int* cu = cu_seqlens.data_ptr<int>();
  if (s.D == 64) {
    gqa_launch_fwd<64, true>(s, qn, kn, vn, nullptr, out, lse, (float)scale,
                             true, cu, T);
  } else {
    gqa_launch_fwd<128, true>(s, qn, kn, vn, nullptr, out, lse, (float)scale,
                              true, cu, T);
  }
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
  torch::Tensor don = gqa_ok_strides_thd(dout) ? dout : dout.contiguous();
  torch::Tensor qn = gqa_ok_strides_thd(q) ? q : q.contiguous();
  torch::Tensor kn = gqa_ok_strides_thd(k) ? k : k.contiguous();
  torch::Tensor vn = gqa_ok_strides_thd(v) ? v : v.contiguous();
  auto dq = torch::zeros({T, s.Hq, s.D}, q.options());
  auto dk = torch::zeros({T, s.Hkv, s.D}, k.options());
  auto dv = torch::zeros({T, s.Hkv, s.D}, v.options());
  if (T == 0 || s.B == 0 || max_seqlen == 0) return {dq, dk, dv};
  auto delta = torch::empty({s.Hq, T}, lse.options());
  const int* cu = cu_seqlens.data_ptr<int>();
  if (s.D == 64) {
    gqa_launch_bwd<64, true>(s, don, qn, kn, vn, out, lse, nullptr, delta, dq,
                             dk, dv, (float)scale, true, cu, T);
  } else {
    gqa_launch_bwd<128, true>(s, don, qn, kn, vn, out, lse, nullptr, delta,
                              dq, dk, dv, (float)scale, true, cu, T);
  }
  return {dq, dk, dv};
}

}  // namespace genrec
