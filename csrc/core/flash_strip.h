// Strip-level steps of a flash-attention tile, one level above mfma_tile.h
// (attention_gqa, attention_beam, attention_flash, hstu_attn,
// hstu_attn_flash).
//
// A block of four waves works on 64-row tiles; a wave owns a strip of 16
// tile rows and holds, per 16-column fragment f, the C fragment
// acc[f][r] = element (row + r, f*16 + col) of its strip (Strip below).
// What a wave does with its strip is written here once: the strip x tile
// MFMA products, the key-validity columns of a K tile, exact (-inf)
// masking, the guarded running softmax, the P stash, the row store of a
// finished strip, and the stashes and products of a backward tile. The head
// dim D and every row stride are compile-time for attention_gqa and
// attention_beam; attention_flash, hstu_attn and hstu_attn_flash take D (32
// or 64) as a kernel argument and use the runtime forms, all on [4]
// accumulators and 128-byte rows. Staging, barriers and what a kernel
// iterates over stay with the kernel.
//
// Bit-stability: every accumulator here is summed in one fixed order (f
// outer, kk inner; the reductions as written), so two kernels that call
// the same step on the same data get the same bits.
#pragma once

#include "mfma_tile.h"

namespace genrec {

// One bf16 operand as a kernel takes it: base pointer plus batch / head /
// row strides in elements, d innermost (stride 1).
struct FlashView {
  const __hip_bfloat16* p;
  int64_t b, h, l;
  // row 0 of batch item bi, head hi
  __device__ __forceinline__ const __hip_bfloat16* rows(int bi, int hi) const {
    return p + (int64_t)bi * b + (int64_t)hi * h;
  }
};

// The batch item (fixed-length) or packed sequence (VARLEN) a block works
// on, and where its rows sit in the operands and outputs.
template <bool VARLEN>
struct GqaSeq {
  int Lq, Lk;  // lengths of this item
  int b;
  int start;   // first token of the sequence in the packed tensors
  bool work;   // false: the block's tile lies beyond the sequence
  // first row of the item in a [B,L,H,D] | [T,H,D] tensor
  __device__ __forceinline__ int64_t tok0(int L) const {
    return VARLEN ? (int64_t)start : (int64_t)b * L;
  }
  // first lse / delta entry of head h ([B,Hq,Lq] | [Hq,T])
  __device__ __forceinline__ int64_t rowb(int h, int Hq, int T) const {
    return VARLEN ? (int64_t)h * T + start : ((int64_t)b * Hq + h) * Lq;
  }
  // row 0 of head h of the item in operand x
  __device__ __forceinline__ const __hip_bfloat16* rows(const FlashView& x,
                                                        int h) const {
    return x.p + (VARLEN ? (int64_t)start * x.l : (int64_t)b * x.b) +
           (int64_t)h * x.h;
  }
};

// tile0: first row of the block's Q (or K) tile. VARLEN reads the token
// range of sequence b, clamped so that it lies inside [0,T]; work is
// uniform per block, so a kernel may return on it before its first barrier.
template <bool VARLEN>
__device__ __forceinline__ GqaSeq<VARLEN> gqa_seq(const int* __restrict__ cu,
                                                  int T, int b, int Lq, int Lk,
                                                  int tile0) {
  if constexpr (VARLEN) {
    const int a = min(max(cu[b], 0), T);
    const int e = min(max(cu[b + 1], a), T);
    return {e - a, e - a, b, a, tile0 < e - a};
  } else {
    return {Lq, Lk, b, 0, true};
  }
}

// Where a lane sits in its wave's strip.
struct Strip {
  int lane;
  int row0;  // first tile row of the strip
  int col;   // the lane's C-fragment column (within a 16-column fragment)
  int row;   // tile row of the lane's C-fragment register r is row + r
  __device__ __forceinline__ explicit Strip(int tid)
      : lane(tid & 63),
        row0((tid >> 6) * 16),
        col(frag_col(lane)),
        row(row0 + frag_row0(lane)) {}
};

// acc[f] += A[strip rows, 0..K) . B[rows f*16.., 0..K)^T for f < NF; a and b
// are swizzled tiles with RSA / RSB bytes per row.
template <int K, int NF, int RSA, int RSB>
__device__ __forceinline__ void strip_mma(float4v (&acc)[NF], const char* a,
                                          const char* b, const Strip& w) {
#pragma unroll
  for (int f = 0; f < NF; ++f) {
#pragma unroll
    for (int kk = 0; kk < K; kk += 32) {
      acc[f] = mfma_bf16(frag_load(a, w.row0, kk, w.lane, RSA),
                         frag_load(b, f * 16, kk, w.lane, RSB), acc[f]);
    }
  }
}

// Runtime form: K extent and live fragment count nf = (D + 15) / 16 as
// arguments, 128-byte rows.
__device__ __forceinline__ void strip_mma(float4v (&acc)[4], const char* a,
                                          const char* b, int K, int nf,
                                          const Strip& w) {
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nf) break;
    for (int kk = 0; kk < K; kk += 32) {
      acc[f] = mfma_bf16(frag_load(a, w.row0, kk, w.lane),
                         frag_load(b, f * 16, kk, w.lane), acc[f]);
    }
  }
}

// Two strip products with the two MFMAs of one (f, kk) step issued back to
// back, so each hides the other's operand loads. Per accumulator the
// summation order is strip_mma's.
template <int K, int NF, int RS>
__device__ __forceinline__ void strip_mma2(float4v (&acc1)[NF], const char* a1,
                                           const char* b1,
                                           float4v (&acc2)[NF], const char* a2,
                                           const char* b2, const Strip& w) {
#pragma unroll
  for (int f = 0; f < NF; ++f) {
#pragma unroll
    for (int kk = 0; kk < K; kk += 32) {
      acc1[f] = mfma_bf16(frag_load(a1, w.row0, kk, w.lane, RS),
                          frag_load(b1, f * 16, kk, w.lane, RS), acc1[f]);
      acc2[f] = mfma_bf16(frag_load(a2, w.row0, kk, w.lane, RS),
                          frag_load(b2, f * 16, kk, w.lane, RS), acc2[f]);
    }
  }
}

// Runtime form, as strip_mma's.
__device__ __forceinline__ void strip_mma2(float4v (&acc1)[4], const char* a1,
                                           const char* b1,
                                           float4v (&acc2)[4], const char* a2,
                                           const char* b2, int K, int nf,
                                           const Strip& w) {
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nf) break;
    for (int kk = 0; kk < K; kk += 32) {
      acc1[f] = mfma_bf16(frag_load(a1, w.row0, kk, w.lane),
                          frag_load(b1, f * 16, kk, w.lane), acc1[f]);
      acc2[f] = mfma_bf16(frag_load(a2, w.row0, kk, w.lane),
                          frag_load(b2, f * 16, kk, w.lane), acc2[f]);
    }
  }
}

// The lane's four key columns of the K tile at kt0: absolute index, and
// whether the key exists and is not padded. pad is null or the [Lk] pad row
// of this batch item.
struct KeyCols {
  int j[4];
  bool ok[4];
};
__device__ __forceinline__ KeyCols key_cols(int kt0, int Lk,
                                            const bool* __restrict__ pad,
                                            const Strip& w) {
  KeyCols kc;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    kc.j[f] = kt0 + f * 16 + w.col;
    kc.ok[f] = kc.j[f] < Lk;
    if (kc.ok[f] && pad) kc.ok[f] = !pad[kc.j[f]];
  }
  return kc;
}

// Which (query row, key) pairs are visible. KeyMask: every valid key, for
// queries that all sit behind the keys. CausalMask: the strip of the Q tile
// at q0, rows beyond Lq see nothing, and with causal set query row i sits
// at absolute position i + off.
struct KeyMask {
  __device__ __forceinline__ bool operator()(const KeyCols& kc, int f,
                                             int) const {
    return kc.ok[f];
  }
};
struct CausalMask {
  int i0, Lq, off;  // i0: absolute query row of the lane's register 0
  bool causal;
  __device__ __forceinline__ CausalMask(int q0, int Lq, int Lk, bool causal,
                                        const Strip& w)
      : i0(q0 + w.row), Lq(Lq), off(Lk - Lq), causal(causal) {}
  __device__ __forceinline__ bool operator()(const KeyCols& kc, int f,
                                             int r) const {
    const int i = i0 + r;
    return kc.ok[f] && i < Lq && !(causal && kc.j[f] > i + off);
  }
  // end of the keys the Q tile at q0 can see: K tiles wholly beyond its
  // diagonal are skipped
  __device__ __forceinline__ int kt_end(int q0, int Lk) const {
    return causal ? min(Lk, q0 + TILE + off) : Lk;
  }
};

// Running softmax of the lane's four strip rows over the K tiles seen so far.
struct RunningSoftmax {
  float m[4], l[4];
  __device__ __forceinline__ RunningSoftmax() {
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
  }

  // s: the masked scores of one K tile (-inf = masked); comes back as the
  // unnormalised p. Rescales accO to the new maximum. A row whose keys so
  // far are all masked keeps m = -inf, l = 0 and contributes nothing (no
  // exp(-inf - -inf)).
  template <int NF>
  __device__ __forceinline__ void step(float (&s)[4][4],
                                       float4v (&accO)[NF]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float tmax = grp16_max(fmaxf(fmaxf(s[0][r], s[1][r]),
                                   fmaxf(s[2][r], s[3][r])));
      float m_new = fmaxf(m[r], tmax);
      bool dead = (m_new == -INFINITY);
      float a = (dead || m[r] == -INFINITY) ? (dead ? 1.f : 0.f)
                                            : __expf(m[r] - m_new);
      float sum = 0.f;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        float p = (s[f][r] == -INFINITY) ? 0.f : __expf(s[f][r] - m_new);
        s[f][r] = p;
        sum += p;
      }
      l[r] = l[r] * a + grp16_sum(sum);
      m[r] = m_new;
#pragma unroll
      for (int f = 0; f < NF; ++f) accO[f][r] *= a;
    }
  }

  // normalised finish: out = accO * inv, lse; both 0 for a row that saw no key
  __device__ __forceinline__ float inv(int r) const {
    return (l[r] > 0.f) ? 1.0f / l[r] : 0.f;
  }
  __device__ __forceinline__ float lse(int r) const {
    return (l[r] > 0.f) ? m[r] + __logf(l[r]) : 0.f;
  }
  // raw finish (split-KV): the partial is (m, l, accO) as they stand; an
  // empty one has nothing in accO worth storing
  __device__ __forceinline__ bool empty(int r) const {
    return m[r] == -INFINITY;
  }
};

// Row-major stash of fragment f of the wave's strip as bf16 into a [64][64]
// tile: x[r] is element (row + r, f*16 + col). The strip is read back by the
// same wave as an A operand, so a wave barrier suffices.
__device__ __forceinline__ void strip_stash(char* tile, int f,
                                            const float (&x)[4],
                                            const Strip& w) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    tile_store(tile, w.row + r, f * 16 + w.col, bf16_bits(x[r]));
  }
}

// The backward stashes take the fragment as packed bf16 bits, which an
// epilogue converts element by element (four floats held across its
// branches cost registers). Row-major as above, and transposed: the lane's
// four values are consecutive columns row..row+3 of tile row f*16 + col,
// one 8-byte store. Other waves read the transposed tile, behind a block
// barrier.
__device__ __forceinline__ void strip_stash(char* tile, int f, short4v x,
                                            const Strip& w) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    tile_store(tile, w.row + r, f * 16 + w.col, (short)x[r]);
  }
}
__device__ __forceinline__ void strip_stash_tr(char* tile, int f, short4v x,
                                               const Strip& w) {
  tile_store(tile, f * 16 + w.col, w.row, x);
}

// Product tail of a backward tile once the epilogue has stashed dS into dsn
// (row-major) and dst (transposed) and A into adt (transposed):
// dQ strip = dS K from the wave's own dsn rows and the staged kt = K^T, handed
// to dq_done (atomics or a store); then, behind the block barrier that
// completes dst / adt, dK += dS^T Q and dV += A^T dO, paired, from the
// staged qt = Q^T and dot = dO^T.
template <typename DqDone>
__device__ __forceinline__ void strip_bwd_products(
    const char* dsn, const char* kt, const char* dst, const char* qt,
    const char* adt, const char* dot, int nf, float4v (&acck)[4],
    float4v (&accv)[4], const Strip& w, DqDone&& dq_done) {
  __builtin_amdgcn_wave_barrier();
  float4v accq[4] = {};
  strip_mma(accq, dsn, kt, TILE, nf, w);
  dq_done(accq);
  __syncthreads();
  strip_mma2(acck, dst, qt, accv, adt, dot, TILE, nf, w);
}

// The K tile at kt0 of a flash forward for the wave's strip: S = Q K_t^T
// from the staged qs [64][D] and ks [64][D], exact masking (keys at or
// beyond Lk, pad keys, and what visible hides), the running-softmax step,
// and accO += P V_t through the wave's rows of ps [64][64] and vt [D][64].
template <int D, typename Mask>
__device__ __forceinline__ void flash_fwd_tile(
    const char* qs, const char* ks, const char* vt, char* ps, int kt0, int Lk,
    const bool* __restrict__ pad, const Mask& visible, float scale,
    RunningSoftmax& sm, float4v (&accO)[D / 16], const Strip& w) {
  float4v acc[4] = {};
  strip_mma<D, 4, D * 2, D * 2>(acc, qs, ks, w);

  const KeyCols kc = key_cols(kt0, Lk, pad, w);
  float s[4][4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[f][r] = visible(kc, f, r) ? __fmul_rn(acc[f][r], scale) : -INFINITY;
    }
  }
  sm.step(s, accO);

#pragma unroll
  for (int f = 0; f < 4; ++f) strip_stash(ps, f, s[f], w);
  __builtin_amdgcn_wave_barrier();
  strip_mma<TILE, D / 16, 128, 128>(accO, ps, vt, w);
  __builtin_amdgcn_wave_barrier();
}

// Store the live rows of a finished strip as bf16 into a [rows, H, D]
// tensor: tile row t of the tile at i0 goes to row tok0 + i0 + t, head h,
// while i0 + t < L. mul, when given, scales register row r by mul[r].
template <int D>
__device__ __forceinline__ void strip_store(__hip_bfloat16* __restrict__ dst,
                                            int64_t tok0, int H, int h,
                                            int i0, int L,
                                            const float4v (&acc)[D / 16],
                                            const Strip& w,
                                            const float* mul = nullptr) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + w.row + r;
    if (i >= L) continue;
    const int64_t ob = ((tok0 + i) * H + h) * D;
#pragma unroll
    for (int f = 0; f < D / 16; ++f) {
      const float x = mul ? acc[f][r] * mul[r] : acc[f][r];
      dst[ob + f * 16 + w.col] = __float2bfloat16(x);
    }
  }
}

// Runtime form: the live rows of a strip into a contiguous [B,H,L,D] tensor
// (bh = b * H + h), columns below D of acc[4].
__device__ __forceinline__ void strip_store(__hip_bfloat16* __restrict__ dst,
                                            int bh, int i0, int L, int D,
                                            const float4v (&acc)[4],
                                            const Strip& w) {
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int d = f * 16 + w.col;
    if (d >= D) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + w.row + r;
      if (i >= L) continue;
      dst[((int64_t)bh * L + i) * D + d] = __float2bfloat16(acc[f][r]);
    }
  }
}

}  // namespace genrec
