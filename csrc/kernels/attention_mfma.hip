// MFMA fused attention (bf16) — gfx950 matrix-core path for K1/K4/K13.
//
// LDS images: every tile is staged ONCE, natural row-major, from coalesced
// 16-byte global loads. A tile that some product needs by columns is a
// dual-use image (mfma_tile.h): ds_read_b128 row reads (frag_load) and
// ds_read_b64_tr_b16 transposed reads (frag_load_tr) of the same bytes are
// both bank-conflict-free, so no transposed copy is built and no
// cross-lane shuffle runs before the first MFMA.
//
// Forward: one 256-thread workgroup (4 waves) per (batch, head); tiles Q,
// K (row reads), V and P^T (dual-use), 32 KiB. Each wave owns a 16-row
// q-strip: S = Q K^T runs as 4 column-fragments x (D/32) K-steps of
// v_mfma_f32_16x16x32_bf16; scale/bias/masks/softmax(or SiLU) are applied
// on the accumulator fragments in-register (the C/D layout places row
// (lane>>4)*4+reg, col lane&15 — a row reduction is an fmax/fadd over the
// 4 column fragments followed by shuffle-xor over the 16-lane group).
// A lane's four P values of one key column go to the P^T image [j][i] as
// ONE 8-byte store; O = P V then reads both operands by columns (A from
// P^T, B from V). Scores never touch HBM; P is saved fp32 for backward.
// The bias / key-padding / additive-mask loads are issued with the tile
// loads, ahead of the staging barrier.
//
// Backward: attn_bwd_ds_kernel stages dO, V, K, Q (dual-use, 6 tiles with
// dS^T and A_d^T: 48.5 KiB, 3 workgroups per CU), computes dP = dO V^T by
// row reads, applies the dropout/query-mask multiplier and the softmax
// Jacobian (or SiLU') in-register, stores dS^T and A_d^T packed, and
// finishes dQ = dS K (A: dS^T by columns, B: K by columns), dK = dS^T Q
// (A: dS^T by rows, B: Q by columns), dV = A_d^T dO (A: A_d^T by rows,
// B: dO by columns) as MFMA in the SAME launch (no extra batched GEMMs,
// no extra global round-trips). P, the dropout mask and the query mask
// are loaded with the tiles, ahead of the staging barrier. All global
// tensors are stride-parameterized so [B,L,H,D] transpose views flow
// in/out without permute copies.
//
// Every MFMA sees the operands, in the k order, that the earlier
// shuffle-transposed images gave it: results are bitwise unchanged.
//
// Calls with Lq <= 16 (softmax, dense bias) run the small-query variants
// further down — one wave per (batch, head), no workgroup barrier — which
// give the same bits; the hosts pick through smallq_applies().

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../core/mfma_tile.h"

namespace genrec {

torch::Tensor colsum(torch::Tensor x);  // fused_elementwise.hip

// A lane's share of the softmax-Jacobian row dot over two column fragments,
// a0*b0 + a1*b1. The compiler contracts that sum into one fma and is free
// to pick either product for it; the 64-row and the small-query backward
// must round alike, so the contraction is written out: the second product
// is rounded, the first fused.
__device__ __forceinline__ float jac_dot2(float a0, float b0, float a1,
                                          float b1) {
  return __builtin_fmaf(a0, b0, a1 * b1);
}

// 32 KiB of LDS lets 5 workgroups (5 waves/SIMD) share a CU; the second
// launch bound keeps the register budget (<= 96) from lowering that.
template <bool IS_SILU>
__global__ void __launch_bounds__(256, 5)
attn_fwd_mfma_kernel(
    const __hip_bfloat16* __restrict__ q,   // [B,H,Lq,D]
    const __hip_bfloat16* __restrict__ k,   // [B,H,Lk,D]
    const __hip_bfloat16* __restrict__ v,   // [B,H,Lk,D]
    const void* __restrict__ bias,          // null | [H,Lq,Lk] | [B,H,Lq,Lk]
                                            // | table [H*nb] (bucket mode)
    const int* __restrict__ bias_bucket,    // null | [Lq,Lk] table indices
    const bool* __restrict__ key_pad,       // null | [B,Lk]
    const float* __restrict__ add_mask,     // null | [Lq,Lk]
    const float* __restrict__ query_mask,   // null | [B,Lq]
    __hip_bfloat16* __restrict__ out,       // [B,H,Lq,D]
    float* __restrict__ p_saved,            // [B,H,Lq,Lk]
    unsigned char* __restrict__ drop_mask,
    const unsigned int* __restrict__ seed_dev,
    int B, int H, int Lq, int Lk, int D, int n_buckets,
    int64_t q_sb, int64_t q_sh, int64_t q_sl,
    int64_t k_sb, int64_t k_sh, int64_t k_sl,
    int64_t v_sb, int64_t v_sh, int64_t v_sl,
    int64_t o_sb, int64_t o_sh, int64_t o_sl,
    float scale, int bias_dim, bool bias_bf16, bool causal,
    float dropout_p, unsigned int seed, int q_tile) {
  if (seed_dev) seed += *seed_dev;
  const float* bias_f = reinterpret_cast<const float*>(bias);
  const __hip_bfloat16* bias_b = reinterpret_cast<const __hip_bfloat16*>(bias);
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int q0 = blockIdx.y * q_tile;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qs = smem;                 // [64(i)][128B(d)] Q, row reads
  char* ks = qs + TILE * 128;      // [64(j)][128B(d)] K, row reads
  char* vs = ks + TILE * 128;      // [64(j)][128B(d)] V, dual-use image
  char* pt = vs + TILE * 128;      // [64(j)][128B(i)] P^T, dual-use image

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // wave-uniform by construction; readfirstlane lets the compiler see it,
  // so the branches around the transposed reads are scalar (EXEC all ones)
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int strip = wid * 16;            // this wave's q rows [strip, strip+16)
  const int col_base = frag_col(lane);
  const int row_grp = frag_row0(lane);   // rows row_grp..row_grp+3 (in strip)

  // ---- stage: coalesced global rows -> swizzled LDS rows (zero-padded).
  // The 256 threads copy two 8-element (16 B) chunks of each tile;
  // row-major walk. V stays natural: the PV B operand reads it by columns
  // (frag_load_tr).
  constexpr int NCH = TILE * (TILE / 8) / 256;
  short8v qq8[NCH], kk8[NCH], vv8[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    int idx = tid + c * 256;
    int row = idx / (TILE / 8);
    int d0 = (idx % (TILE / 8)) * 8;
    int qi = q0 + row;
    qq8[c] = load8(q, (int64_t)b * q_sb + h * q_sh + qi * q_sl + d0,
                   qi < Lq && d0 < D);
    kk8[c] = load8(k, (int64_t)b * k_sb + h * k_sh + row * k_sl + d0,
                   row < Lk && d0 < D);
    vv8[c] = load8(v, (int64_t)b * v_sb + h * v_sh + row * v_sl + d0,
                   row < Lk && d0 < D);
  }

  // ---- epilogue inputs (bias / key padding / additive mask) depend only
  // on indices: issue them behind the tile loads and ahead of the staging
  // barrier so one global-latency wait covers both
  float bias_v[4][4], am_v[4][4];
  bool kp_v[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    int j = f * 16 + col_base;          // key col
    kp_v[f] = (key_pad && j < Lk) ? key_pad[(int64_t)b * Lk + j] : false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = q0 + strip + row_grp + r;   // global q row
      bool ok = (i < Lq) && (j < Lk);
      float bv = 0.f, av = 0.f;
      if (ok) {
        if (bias_dim) {
          int64_t bi = (bias_dim == 3) ? ((int64_t)h * Lq + i) * Lk + j
                                       : idx4(b, h, i, j, H, Lq, Lk);
          bv = bias_bf16 ? to_f32(bias_b[bi]) : bias_f[bi];
        } else if (bias_bucket) {
          // in-kernel rel-bias table gather (HSTU-style): no
          // materialized [H,Lq,Lk] bias tensor traffic
          bv = bias_f[h * n_buckets + bias_bucket[(int64_t)i * Lk + j]];
        }
        if (add_mask) av = add_mask[(int64_t)i * Lk + j];
      }
      bias_v[f][r] = bv;
      am_v[f][r] = av;
    }
  }

#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    int idx = tid + c * 256;
    int row = idx / (TILE / 8);
    int d0 = (idx % (TILE / 8)) * 8;
    tile_store(qs, row, d0, qq8[c]);
    tile_store(ks, row, d0, kk8[c]);
    tile_store<true>(vs, row, d0, vv8[c]);
  }
  __syncthreads();

  const float inv_keep = dropout_p > 0.f ? 1.0f / (1.0f - dropout_p) : 1.0f;

  // ---- S = Q K^T : 4 column fragments
  float4v acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                    {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    for (int kk = 0; kk < D; kk += 32) {
      short8v a = frag_load(qs, strip, kk, lane);
      short8v bfr = frag_load(ks, f * 16, kk, lane);
      acc[f] = mfma_bf16(a, bfr, acc[f]);
    }
  }

  // ---- epilogue on fragments: scale + bias + masks
  float s_val[4][4];                     // [fragment][reg]
#pragma unroll
  for (int f = 0; f < 4; ++f) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = q0 + strip + row_grp + r;   // global q row
      int j = f * 16 + col_base;          // key col
      float s = acc[f][r];
      bool ok = (i < Lq) && (j < Lk);
      if (ok) {
        s *= scale;
        if (bias_dim || bias_bucket) s += bias_v[f][r];
        if (causal && j > i) s = NEG_BIG;
        if (kp_v[f]) s = NEG_BIG;
        if (add_mask) s += am_v[f][r];
      } else {
        s = -INFINITY;
      }
      s_val[f][r] = s;
    }
  }

  float p_val[4][4];
  if (IS_SILU) {
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = s_val[f][r];
        p_val[f][r] = (s == -INFINITY) ? 0.f : s * sigmoidf_dev(s);
      }
  } else {
    // row softmax: combine 4 col fragments per reg, reduce over 16-lane grp
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m = grp16_max(fmaxf(fmaxf(s_val[0][r], s_val[1][r]),
                                fmaxf(s_val[2][r], s_val[3][r])));
      float sum = 0.f;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        float e = (s_val[f][r] == -INFINITY) ? 0.f
                                             : __expf(s_val[f][r] - m);
        p_val[f][r] = e;
        sum += e;
      }
      sum = grp16_sum(sum);
      float inv = (sum > 0.f) ? 1.0f / sum : 0.f;
#pragma unroll
      for (int f = 0; f < 4; ++f) p_val[f][r] *= inv;
    }
  }

  // ---- save P/S, apply post-softmax query mask + dropout, stash P^T in
  // LDS: a lane's 4 r-values are consecutive i of one key column j, so they
  // pack into ONE aligned 8-byte store at pt[j][i0..i0+3]
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    short4v ppack;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = q0 + strip + row_grp + r;
      int j = f * 16 + col_base;
      float p = p_val[f][r];
      if (i < Lq && j < Lk) {
        p_saved[idx4(b, h, i, j, H, Lq, Lk)] = IS_SILU ? s_val[f][r] : p;
        if (query_mask) p *= query_mask[(int64_t)b * Lq + i];
        if (dropout_p > 0.f) {
          unsigned long long gidx = idx4(b, h, i, j, H, Lq, Lk);
          bool keep = (hash_rng(seed, gidx) & 0xFFFFFF) >=
                      (unsigned int)(dropout_p * 16777216.0f);
          drop_mask[gidx] = keep;
          p = keep ? p * inv_keep : 0.f;
        }
      } else {
        p = 0.f;
      }
      ppack[r] = bf16_bits(p);
    }
    tile_store<true>(pt, f * 16 + col_base, strip + row_grp, ppack);
  }
  // wave-local: this wave only reads its own strip's 16 i-columns back
  __builtin_amdgcn_wave_barrier();

  // ---- O = P V : A = P^T columns (m=i, k=j), B = V columns (k=j, n=d),
  // both by transposed reads (wave-uniform control flow only: EXEC all ones)
  float4v acc2[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                     {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const int nfrag_d = (D + 15) / 16;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nfrag_d) break;
    for (int kk = 0; kk < TILE; kk += 32) {
      short8v a = frag_load_tr(pt, kk, strip, lane);
      short8v bfr = frag_load_tr(vs, kk, f * 16, lane);
      acc2[f] = mfma_bf16(a, bfr, acc2[f]);
    }
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nfrag_d) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = q0 + strip + row_grp + r;
      int d = f * 16 + col_base;
      if (i < Lq && d < D) {
        out[(int64_t)b * o_sb + h * o_sh + i * o_sl + d] =
            __float2bfloat16(acc2[f][r]);
      }
    }
  }
}

// ---- backward dS kernel: dP = dO V^T (MFMA), then Jacobian in-register,
// then dQ/dK/dV MFMA in the same launch.
//
// 8-wave occupancy layout (round 2): 512 threads; wave pair p = wid>>1
// owns q/j-strip [16p, 16p+16) and half = wid&1 computes dP column
// fragments {2*half, 2*half+1}. The softmax-Jacobian row dot becomes
// cross-wave: each half reduces its 2-fragment partial over the 16-lane
// group and writes it to a per-half LDS slot (dotbuf[2][64], 512 B — no
// atomics: every slot has exactly one writer); one barrier later both
// halves read the summed dot. dS^T/A_d^T stores stay disjoint per half
// (different column fragments -> different j rows of the transposed
// tiles), and dQ/dK/dV split their OUTPUT d-fragments across the halves
// with full k-loops. Six tiles + 512 B of LDS: 3 blocks/CU, 24 resident
// waves (64-70 VGPRs allow more). The launch is exactly 512 threads: each
// stages one 16-byte chunk of each of the four input tiles.
template <bool IS_SILU>
__global__ void __launch_bounds__(512)
attn_bwd_ds_kernel(
    const __hip_bfloat16* __restrict__ dout,  // [B,H,Lq,D]
    const __hip_bfloat16* __restrict__ q,     // [B,H,Lq,D]
    const __hip_bfloat16* __restrict__ k,     // [B,H,Lk,D]
    const __hip_bfloat16* __restrict__ v,     // [B,H,Lk,D]
    const float* __restrict__ p_saved,        // [B,H,Lq,Lk] (P or S)
    const float* __restrict__ query_mask,     // null | [B,Lq]
    const unsigned char* __restrict__ drop_mask,
    __hip_bfloat16* __restrict__ dq_out,      // [B,H,Lq,D]
    __hip_bfloat16* __restrict__ dk_out,      // [B,H,Lk,D]
    __hip_bfloat16* __restrict__ dv_out,      // [B,H,Lk,D]
    __hip_bfloat16* __restrict__ ds_saved,    // null | [B,H,Lq,Lk] bias grad
                                              // (bf16: halves the HBM
                                              // round-trip; summed fp32)
    const int* __restrict__ bias_bucket,      // null | [Lq,Lk]
    float* __restrict__ dtab_partial,         // null | [B*H, n_buckets]
    int n_buckets,
    int B, int H, int Lq, int Lk, int D,
    int64_t do_sb, int64_t do_sh, int64_t do_sl,
    int64_t q_sb, int64_t q_sh, int64_t q_sl,
    int64_t k_sb, int64_t k_sh, int64_t k_sl,
    int64_t v_sb, int64_t v_sh, int64_t v_sl,
    int64_t dq_sb, int64_t dq_sh, int64_t dq_sl,
    int64_t dk_sb, int64_t dk_sh, int64_t dk_sl,
    int64_t dv_sb, int64_t dv_sh, int64_t dv_sl,
    float scale, float dropout_p) {
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // Every tile is a natural row-major dual-use image, staged once: dP
  // reads dO and V by rows, dQ/dK/dV read K, Q and dO by columns.
  char* dos = smem;                 // [64(i)][128B(d)] dO (A for dP, B for dV)
  char* vs = dos + TILE * 128;      // [64(j)][128B(d)] V (B for dP)
  char* ks = vs + TILE * 128;       // [64(j)][128B(d)] K (B for dQ)
  char* qs = ks + TILE * 128;       // [64(i)][128B(d)] Q (B for dK)
  char* dst = qs + TILE * 128;      // [64(j)][128B(i)] dS^T (A for dQ, dK)
  char* adt = dst + TILE * 128;     // [64(j)][128B(i)] A_d^T (A for dV)
  float* dotbuf = reinterpret_cast<float*>(adt + TILE * 128);  // [2][64]
  float* tab_lds = dotbuf + 2 * TILE;  // [n_buckets] table-grad partials

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7, scalar
  const int pair = wid >> 1;         // strip owner
  const int half = wid & 1;          // fragment split
  const int fbase = half * 2;
  const int strip = pair * 16;
  const int col_base = frag_col(lane);
  const int row_grp = frag_row0(lane);

  if (dtab_partial && tid < n_buckets) tab_lds[tid] = 0.f;

  // stage: the 512 threads hold one 8-element chunk of each tile
  short8v dd8, vv8, kk8, qq8;
  const int st_row = tid / (TILE / 8);
  const int st_d0 = (tid % (TILE / 8)) * 8;
  {
    const int row = st_row, d0 = st_d0;
    const bool q_ok = row < Lq && d0 < D, k_ok = row < Lk && d0 < D;
    dd8 = load8(dout, (int64_t)b * do_sb + h * do_sh + row * do_sl + d0, q_ok);
    vv8 = load8(v, (int64_t)b * v_sb + h * v_sh + row * v_sl + d0, k_ok);
    kk8 = load8(k, (int64_t)b * k_sb + h * k_sh + row * k_sl + d0, k_ok);
    qq8 = load8(q, (int64_t)b * q_sb + h * q_sh + row * q_sl + d0, q_ok);
  }

  // P (or S), the dropout mask and the query mask depend only on indices:
  // issue them behind the tile loads and ahead of the staging barrier so
  // one global-latency wait covers both instead of a second one after the
  // dP MFMAs
  float pv[2][4], qm_v[4];
  unsigned char dm_v[2][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int i = strip + row_grp + r;
    qm_v[r] = (!IS_SILU && query_mask && i < Lq)
                  ? query_mask[(int64_t)b * Lq + i] : 1.f;
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) {
      int j = (fbase + fi) * 16 + col_base;
      bool ok = (i < Lq) && (j < Lk);
      pv[fi][r] = ok ? p_saved[idx4(b, h, i, j, H, Lq, Lk)] : 0.f;
      dm_v[fi][r] = (!IS_SILU && dropout_p > 0.f && ok)
                        ? drop_mask[idx4(b, h, i, j, H, Lq, Lk)] : 0;
    }
  }

  tile_store<true>(dos, st_row, st_d0, dd8);
  tile_store<true>(vs, st_row, st_d0, vv8);
  tile_store<true>(ks, st_row, st_d0, kk8);
  tile_store<true>(qs, st_row, st_d0, qq8);
  __syncthreads();

  const float inv_keep = dropout_p > 0.f ? 1.0f / (1.0f - dropout_p) : 1.0f;

  // dP = dO V^T : A = dO strip rows (k=d), B = V rows (n=j, k=d).
  // This half computes column fragments fbase and fbase+1 only.
  float4v acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int fi = 0; fi < 2; ++fi) {
    for (int kk = 0; kk < D; kk += 32) {
      short8v a = frag_load<true>(dos, strip, kk, lane);
      short8v bfr = frag_load<true>(vs, (fbase + fi) * 16, kk, lane);
      acc[fi] = mfma_bf16(a, bfr, acc[fi]);
    }
  }

  float da[2][4], ad[2][4];
#pragma unroll
  for (int fi = 0; fi < 2; ++fi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = strip + row_grp + r;
      int j = (fbase + fi) * 16 + col_base;
      bool ok = (i < Lq) && (j < Lk);
      float p = pv[fi][r];    // P (softmax) or S (silu)
      float m = 1.f;
      if (!IS_SILU && ok) {
        if (query_mask) m *= qm_v[r];
        if (dropout_p > 0.f) m *= dm_v[fi][r] ? inv_keep : 0.f;
      }
      da[fi][r] = ok ? acc[fi][r] * (IS_SILU ? 1.f : m) : 0.f;
      ad[fi][r] = IS_SILU ? (ok ? p * sigmoidf_dev(p) : 0.f) : p * m;
    }
  }

  float ds[2][4];
  if (IS_SILU) {
#pragma unroll
    for (int fi = 0; fi < 2; ++fi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = pv[fi][r];
        float sg = sigmoidf_dev(s);
        ds[fi][r] = da[fi][r] * sg * (1.f + s * (1.f - sg));
      }
  } else {
    // Jacobian row dot across both halves: reduce this half's 32-column
    // partial in-wave, publish to dotbuf[half], barrier, read the sum.
    float part[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      part[r] = grp16_sum(jac_dot2(da[0][r], pv[0][r], da[1][r], pv[1][r]));
    if (col_base == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        dotbuf[half * TILE + strip + row_grp + r] = part[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float dot_r = dotbuf[strip + row_grp + r] +
                    dotbuf[TILE + strip + row_grp + r];
#pragma unroll
      for (int fi = 0; fi < 2; ++fi)
        ds[fi][r] = pv[fi][r] * (da[fi][r] - dot_r);
    }
  }

  // stash dS^T and A_d^T in LDS; optional global dS. A lane's 4 r-values
  // land on consecutive columns of row j, so they pack into ONE aligned
  // 8-byte ds_write (4x fewer LDS stores than per-element bf16 scatter ->
  // fewer bank conflict cycles; rocprofv3 SQ_LDS_BANK_CONFLICT was
  // dominated by these stores). dQ reads dS^T by columns, so there is no
  // natural dS image. Halves write disjoint j rows / column fragments.
  const int i0 = strip + row_grp;  // multiple of 4 -> byte i0*2 is 8B-aligned
#pragma unroll
  for (int fi = 0; fi < 2; ++fi) {
    short4v dpack, apack;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = i0 + r;
      int j = (fbase + fi) * 16 + col_base;
      float dval = (i < Lq && j < Lk) ? ds[fi][r] : 0.f;
      float aval = (i < Lq && j < Lk) ? ad[fi][r] : 0.f;
      dpack[r] = bf16_bits(dval * scale);
      apack[r] = bf16_bits(aval);
      if (ds_saved && i < Lq && j < Lk) {
        ds_saved[idx4(b, h, i, j, H, Lq, Lk)] = __float2bfloat16(dval);
      }
      if (dtab_partial && i < Lq && j < Lk) {
        // LDS-privatized table-grad accumulation (32-entry histogram)
        atomicAdd(&tab_lds[bias_bucket[(int64_t)i * Lk + j]], dval);
      }
    }
    int j = (fbase + fi) * 16 + col_base;
    tile_store<true>(dst, j, i0, dpack);
    tile_store<true>(adt, j, i0, apack);
  }
  // dQ's A-operand (this strip's i columns of dS^T) mixes both halves'
  // j rows, and dK/dV read all pairs' dS^T/A_d^T columns: one workgroup
  // barrier covers every consumer below.
  __syncthreads();
  if (dtab_partial && tid < n_buckets) {
    // one partial row per (b,h) block; reduced deterministically on the
    // host via colsum over [B, H*nb]
    dtab_partial[(int64_t)bh * n_buckets + tid] = tab_lds[tid];
  }

  const int nfrag_d = (D + 15) / 16;
  {  // dQ[strip rows] = (scale*dS) @ K : output d-fragments split by half
    float4v accq[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) {
      if (fbase + fi >= nfrag_d) break;
      for (int kk = 0; kk < TILE; kk += 32) {
        short8v a = frag_load_tr(dst, kk, strip, lane);
        short8v bfr = frag_load_tr(ks, kk, (fbase + fi) * 16, lane);
        accq[fi] = mfma_bf16(a, bfr, accq[fi]);
      }
    }
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) {
      if (fbase + fi >= nfrag_d) break;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i = strip + row_grp + r;
        int d = (fbase + fi) * 16 + col_base;
        if (i < Lq && d < D) {
          dq_out[(int64_t)b * dq_sb + h * dq_sh + i * dq_sl + d] =
              __float2bfloat16(accq[fi][r]);
        }
      }
    }
  }

  {  // dK[j strip] = (scale*dS)^T @ Q ; dV[j strip] = A_d^T @ dO
    float4v acck[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float4v accv[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) {
      if (fbase + fi >= nfrag_d) break;
      for (int kk = 0; kk < TILE; kk += 32) {
        short8v a1 = frag_load<true>(dst, strip, kk, lane);
        short8v b1 = frag_load_tr(qs, kk, (fbase + fi) * 16, lane);
        acck[fi] = mfma_bf16(a1, b1, acck[fi]);
        short8v a2 = frag_load<true>(adt, strip, kk, lane);
        short8v b2 = frag_load_tr(dos, kk, (fbase + fi) * 16, lane);
        accv[fi] = mfma_bf16(a2, b2, accv[fi]);
      }
    }
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) {
      if (fbase + fi >= nfrag_d) break;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int j = strip + row_grp + r;
        int d = (fbase + fi) * 16 + col_base;
        if (j < Lk && d < D) {
          dk_out[(int64_t)b * dk_sb + h * dk_sh + j * dk_sl + d] =
              __float2bfloat16(acck[fi][r]);
          dv_out[(int64_t)b * dv_sb + h * dv_sh + j * dv_sl + d] =
              __float2bfloat16(accv[fi][r]);
        }
      }
    }
  }
}

// ---- small-query variants (Lq <= 16, softmax, dense bias) --------------
//
// The decoder-side calls of a T5 step have a handful of query rows: in the
// 64-row kernels above three of four strips hold no row, yet every block
// stages full tiles and meets at workgroup barriers. Here ONE wave owns a
// (batch, head): q strip 0 is the only strip, the wave's LDS images are
// private to it, and nothing but program order (LDS operations of a wave
// complete in issue order) stands between a store and the read of another
// lane — no __syncthreads. A workgroup packs SQ_HEADS such waves; a wave
// past the last head returns at once, which nothing else waits on.
//
// Only image rows that can hold data exist: K/V/P^T/dS^T have
// round32(Lk) rows (a transposed read spans a 32-row k step), Q and dO
// have 16 (forward, row reads) or 32 (backward, transposed reads). Column
// fragments with f*16 >= Lk and k steps that are all padding are skipped:
// the kernels are instances by NF = ceil(Lk / 16), so a dead fragment's
// loads, softmax terms and stores are not in the code at all.
// A skipped fragment is all -inf / all zero in the 64-row kernels and a
// skipped k step adds +0 to an accumulator that cannot be -0, every other
// MFMA sees the same operands in the same order, and the element-wise
// code is the same text: all outputs equal the 64-row kernels' bit for bit.
constexpr int SQ_HEADS = 2;   // heads (= waves) per workgroup
constexpr int SQ_LQ = 16;     // largest Lq of the small-query path
// The backward takes one key strip only. Its strip loop is serial in the
// one wave: at Lk = 61 (four strips) it measured slower than the 64-row
// backward, 24.1 against 21.0 us, so only the one-strip instance is built.
constexpr int SQ_BWD_LK = 16;

static inline int sq_rows32(int L) { return (L + 31) & ~31; }
// LDS bytes of one head: Q[16] + K[kr] (P^T overlays it) + V[kr]
static inline size_t sq_fwd_lds(int Lk) {
  return (size_t)(16 + 2 * sq_rows32(Lk)) * 128;
}
// dO[32] + Q[32] + K[kr] + V[kr] (A_d^T, then dS^T overlay V)
static inline size_t sq_bwd_lds(int Lk) {
  return (size_t)(64 + 2 * sq_rows32(Lk)) * 128;
}

// orders this wave's LDS stores and reads of other lanes' data: no
// instruction, it only keeps the compiler from moving them across
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int NF>   // live key column fragments: ceil(Lk / 16)
__global__ void __launch_bounds__(64 * SQ_HEADS)
attn_fwd_smallq_kernel(
    const __hip_bfloat16* __restrict__ q,   // [B,H,Lq,D]
    const __hip_bfloat16* __restrict__ k,   // [B,H,Lk,D]
    const __hip_bfloat16* __restrict__ v,   // [B,H,Lk,D]
    const void* __restrict__ bias,          // null | [H,Lq,Lk] | [B,H,Lq,Lk]
    const bool* __restrict__ key_pad,       // null | [B,Lk]
    const float* __restrict__ add_mask,     // null | [Lq,Lk]
    const float* __restrict__ query_mask,   // null | [B,Lq]
    __hip_bfloat16* __restrict__ out,       // [B,H,Lq,D]
    float* __restrict__ p_saved,            // [B,H,Lq,Lk]
    unsigned char* __restrict__ drop_mask,
    const unsigned int* __restrict__ seed_dev,
    int B, int H, int Lq, int Lk, int D,
    int64_t q_sb, int64_t q_sh, int64_t q_sl,
    int64_t k_sb, int64_t k_sh, int64_t k_sl,
    int64_t v_sb, int64_t v_sh, int64_t v_sl,
    int64_t o_sb, int64_t o_sh, int64_t o_sl,
    float scale, int bias_dim, bool bias_bf16, bool causal,
    float dropout_p, unsigned int seed) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bh = blockIdx.x * SQ_HEADS + wid;
  if (bh >= B * H) return;              // wave-uniform; no barrier below
  if (seed_dev) seed += *seed_dev;
  const float* bias_f = reinterpret_cast<const float*>(bias);
  const __hip_bfloat16* bias_b = reinterpret_cast<const __hip_bfloat16*>(bias);
  const int b = bh / H, h = bh % H;
  constexpr int nf = NF;
  constexpr int kr = (NF + 1) / 2 * 32;  // rows of the K / V / P^T images

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qs = smem + (size_t)wid * (16 + 2 * kr) * 128;  // [16(i)][128B(d)]
  char* ks = qs + 16 * 128;             // [kr(j)][128B(d)] K, row reads
  char* vs = ks + kr * 128;             // [kr(j)][128B(d)] V, dual-use image
  char* pt = ks;                        // [kr(j)][128B(i)] P^T once S is done

  const int col_base = frag_col(lane);
  const int row_grp = frag_row0(lane);

  // ---- stage: the 64 lanes copy 8 rows x 8 chunks per step
  const int st_row = lane >> 3;
  const int st_d0 = (lane & 7) * 8;
  short8v qq8[2], kk8[kr / 8], vv8[kr / 8];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    int row = c * 8 + st_row;
    qq8[c] = load8(q, (int64_t)b * q_sb + h * q_sh + row * q_sl + st_d0,
                   row < Lq && st_d0 < D);
  }
#pragma unroll
  for (int c = 0; c < kr / 8; ++c) {
    int row = c * 8 + st_row;
    kk8[c] = load8(k, (int64_t)b * k_sb + h * k_sh + row * k_sl + st_d0,
                   row < Lk && st_d0 < D);
    vv8[c] = load8(v, (int64_t)b * v_sb + h * v_sh + row * v_sl + st_d0,
                   row < Lk && st_d0 < D);
  }

  // ---- epilogue inputs, issued behind the tile loads
  float bias_v[4][4], am_v[4][4];
  bool kp_v[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    int j = f * 16 + col_base;          // key col
    kp_v[f] = (key_pad && f < nf && j < Lk) ? key_pad[(int64_t)b * Lk + j] : false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = row_grp + r;              // q row
      bool ok = (f < nf) && (i < Lq) && (j < Lk);
      float bv = 0.f, av = 0.f;
      if (ok) {
        if (bias_dim) {
          int64_t bi = (bias_dim == 3) ? ((int64_t)h * Lq + i) * Lk + j
                                       : idx4(b, h, i, j, H, Lq, Lk);
          bv = bias_bf16 ? to_f32(bias_b[bi]) : bias_f[bi];
        }
        if (add_mask) av = add_mask[(int64_t)i * Lk + j];
      }
      bias_v[f][r] = bv;
      am_v[f][r] = av;
    }
  }

#pragma unroll
  for (int c = 0; c < 2; ++c)
    tile_store(qs, c * 8 + st_row, st_d0, qq8[c]);
#pragma unroll
  for (int c = 0; c < kr / 8; ++c) {
    if (c * 8 < nf * 16) tile_store(ks, c * 8 + st_row, st_d0, kk8[c]);
    tile_store<true>(vs, c * 8 + st_row, st_d0, vv8[c]);
  }
  wave_lds_sync();

  const float inv_keep = dropout_p > 0.f ? 1.0f / (1.0f - dropout_p) : 1.0f;

  // ---- S = Q K^T : the live column fragments
  float4v acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                    {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nf) break;
    for (int kk = 0; kk < D; kk += 32) {
      short8v a = frag_load(qs, 0, kk, lane);
      short8v bfr = frag_load(ks, f * 16, kk, lane);
      acc[f] = mfma_bf16(a, bfr, acc[f]);
    }
  }

  // ---- epilogue on fragments: scale + bias + masks
  float s_val[4][4];                     // [fragment][reg]
#pragma unroll
  for (int f = 0; f < 4; ++f) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = row_grp + r;                // q row
      int j = f * 16 + col_base;          // key col
      float s = acc[f][r];
      bool ok = (f < nf) && (i < Lq) && (j < Lk);
      if (ok) {
        s *= scale;
        if (bias_dim) s += bias_v[f][r];
        if (causal && j > i) s = NEG_BIG;
        if (kp_v[f]) s = NEG_BIG;
        if (add_mask) s += am_v[f][r];
      } else {
        s = -INFINITY;
      }
      s_val[f][r] = s;
    }
  }

  // row softmax: combine 4 col fragments per reg, reduce over 16-lane grp
  float p_val[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float m = grp16_max(fmaxf(fmaxf(s_val[0][r], s_val[1][r]),
                              fmaxf(s_val[2][r], s_val[3][r])));
    float sum = 0.f;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      float e = (s_val[f][r] == -INFINITY) ? 0.f
                                           : __expf(s_val[f][r] - m);
      p_val[f][r] = e;
      sum += e;
    }
    sum = grp16_sum(sum);
    float inv = (sum > 0.f) ? 1.0f / sum : 0.f;
#pragma unroll
    for (int f = 0; f < 4; ++f) p_val[f][r] *= inv;
  }

  // K is dead: P^T takes its place (every S read precedes in program order)
  wave_lds_sync();

  // ---- save P, apply post-softmax query mask + dropout, stash P^T
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f * 16 >= kr) break;
    short4v ppack;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = row_grp + r;
      int j = f * 16 + col_base;
      float p = p_val[f][r];
      if (f < nf && i < Lq && j < Lk) {
        p_saved[idx4(b, h, i, j, H, Lq, Lk)] = p;
        if (query_mask) p *= query_mask[(int64_t)b * Lq + i];
        if (dropout_p > 0.f) {
          unsigned long long gidx = idx4(b, h, i, j, H, Lq, Lk);
          bool keep = (hash_rng(seed, gidx) & 0xFFFFFF) >=
                      (unsigned int)(dropout_p * 16777216.0f);
          drop_mask[gidx] = keep;
          p = keep ? p * inv_keep : 0.f;
        }
      } else {
        p = 0.f;
      }
      ppack[r] = bf16_bits(p);
    }
    tile_store<true>(pt, f * 16 + col_base, row_grp, ppack);
  }
  wave_lds_sync();

  // ---- O = P V over the live 32-row k steps (uniform control flow only)
  float4v acc2[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                     {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const int nfrag_d = (D + 15) / 16;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nfrag_d) break;
    for (int kk = 0; kk < kr; kk += 32) {
      short8v a = frag_load_tr(pt, kk, 0, lane);
      short8v bfr = frag_load_tr(vs, kk, f * 16, lane);
      acc2[f] = mfma_bf16(a, bfr, acc2[f]);
    }
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nfrag_d) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = row_grp + r;
      int d = f * 16 + col_base;
      if (i < Lq && d < D) {
        out[(int64_t)b * o_sb + h * o_sh + i * o_sl + d] =
            __float2bfloat16(acc2[f][r]);
      }
    }
  }
}

// Backward of the above: one wave per (batch, head) loops over the live key
// strips for dK/dV. The Jacobian row dot keeps the 64-row kernel's order,
// (fragments 0+1 group-reduced) + (fragments 2+3 group-reduced). V is dead
// after dP, so A_d^T (for dV) and then dS^T (for dQ, dK) take its place in
// turn: 16 KiB per head up to Lk = 32, 24 KiB up to 64. The host launches
// the one-strip instance only (SQ_BWD_LK).
template <int NF>   // live key fragments / key strips: ceil(Lk / 16)
__global__ void __launch_bounds__(64 * SQ_HEADS)
attn_bwd_smallq_kernel(
    const __hip_bfloat16* __restrict__ dout,  // [B,H,Lq,D]
    const __hip_bfloat16* __restrict__ q,     // [B,H,Lq,D]
    const __hip_bfloat16* __restrict__ k,     // [B,H,Lk,D]
    const __hip_bfloat16* __restrict__ v,     // [B,H,Lk,D]
    const float* __restrict__ p_saved,        // [B,H,Lq,Lk]
    const float* __restrict__ query_mask,     // null | [B,Lq]
    const unsigned char* __restrict__ drop_mask,
    __hip_bfloat16* __restrict__ dq_out,      // [B,H,Lq,D]
    __hip_bfloat16* __restrict__ dk_out,      // [B,H,Lk,D]
    __hip_bfloat16* __restrict__ dv_out,      // [B,H,Lk,D]
    __hip_bfloat16* __restrict__ ds_saved,    // null | [B,H,Lq,Lk] bias grad
    int B, int H, int Lq, int Lk, int D,
    int64_t do_sb, int64_t do_sh, int64_t do_sl,
    int64_t q_sb, int64_t q_sh, int64_t q_sl,
    int64_t k_sb, int64_t k_sh, int64_t k_sl,
    int64_t v_sb, int64_t v_sh, int64_t v_sl,
    int64_t dq_sb, int64_t dq_sh, int64_t dq_sl,
    int64_t dk_sb, int64_t dk_sh, int64_t dk_sl,
    int64_t dv_sb, int64_t dv_sh, int64_t dv_sl,
    float scale, float dropout_p) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bh = blockIdx.x * SQ_HEADS + wid;
  if (bh >= B * H) return;              // wave-uniform; no barrier below
  const int b = bh / H, h = bh % H;
  constexpr int nf = NF;
  constexpr int kr = (NF + 1) / 2 * 32;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // dual-use images; dO and Q carry 32 rows (rows >= Lq zero) because dV
  // and dK read them by columns over one 32-row k step
  char* dos = smem + (size_t)wid * (64 + 2 * kr) * 128;  // [32(i)][128B(d)]
  char* qs = dos + 32 * 128;            // [32(i)][128B(d)] Q (B for dK)
  char* ks = qs + 32 * 128;             // [kr(j)][128B(d)] K (B for dQ)
  char* vs = ks + kr * 128;             // [kr(j)][128B(d)] V (B for dP)
  char* adt = vs;                       // [kr(j)][128B(i)] A_d^T, after dP
  char* dst = vs;                       // [kr(j)][128B(i)] dS^T, after dV

  const int col_base = frag_col(lane);
  const int row_grp = frag_row0(lane);

  const int st_row = lane >> 3;
  const int st_d0 = (lane & 7) * 8;
  short8v dd8[2], qq8[2], kk8[kr / 8], vv8[kr / 8];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    int row = c * 8 + st_row;
    const bool q_ok = row < Lq && st_d0 < D;
    dd8[c] = load8(dout, (int64_t)b * do_sb + h * do_sh + row * do_sl + st_d0,
                   q_ok);
    qq8[c] = load8(q, (int64_t)b * q_sb + h * q_sh + row * q_sl + st_d0,
                   q_ok);
  }
#pragma unroll
  for (int c = 0; c < kr / 8; ++c) {
    int row = c * 8 + st_row;
    const bool k_ok = row < Lk && st_d0 < D;
    vv8[c] = load8(v, (int64_t)b * v_sb + h * v_sh + row * v_sl + st_d0,
                   k_ok);
    kk8[c] = load8(k, (int64_t)b * k_sb + h * k_sh + row * k_sl + st_d0,
                   k_ok);
  }

  // P, the dropout mask and the query mask, issued behind the tile loads
  float pv[4][4], qm_v[4];
  unsigned char dm_v[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int i = row_grp + r;
    qm_v[r] = (query_mask && i < Lq) ? query_mask[(int64_t)b * Lq + i] : 1.f;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      int j = f * 16 + col_base;
      bool ok = (f < nf) && (i < Lq) && (j < Lk);
      pv[f][r] = ok ? p_saved[idx4(b, h, i, j, H, Lq, Lk)] : 0.f;
      dm_v[f][r] = (dropout_p > 0.f && ok)
                       ? drop_mask[idx4(b, h, i, j, H, Lq, Lk)] : 0;
    }
  }

#pragma unroll
  for (int c = 0; c < 2; ++c) {
    tile_store<true>(dos, c * 8 + st_row, st_d0, dd8[c]);
    tile_store<true>(qs, c * 8 + st_row, st_d0, qq8[c]);
    tile_store<true>(dos, 16 + c * 8 + st_row, st_d0, short8v{});
    tile_store<true>(qs, 16 + c * 8 + st_row, st_d0, short8v{});
  }
#pragma unroll
  for (int c = 0; c < kr / 8; ++c) {
    if (c * 8 < nf * 16) tile_store<true>(vs, c * 8 + st_row, st_d0, vv8[c]);
    tile_store<true>(ks, c * 8 + st_row, st_d0, kk8[c]);
  }
  wave_lds_sync();

  const float inv_keep = dropout_p > 0.f ? 1.0f / (1.0f - dropout_p) : 1.0f;

  // dP = dO V^T : A = dO rows (k=d), B = V rows (n=j, k=d)
  float4v acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                    {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nf) break;
    for (int kk = 0; kk < D; kk += 32) {
      short8v a = frag_load<true>(dos, 0, kk, lane);
      short8v bfr = frag_load<true>(vs, f * 16, kk, lane);
      acc[f] = mfma_bf16(a, bfr, acc[f]);
    }
  }

  float da[4][4], ad[4][4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = row_grp + r;
      int j = f * 16 + col_base;
      bool ok = (f < nf) && (i < Lq) && (j < Lk);
      float p = pv[f][r];
      float m = 1.f;
      if (ok) {
        if (query_mask) m *= qm_v[r];
        if (dropout_p > 0.f) m *= dm_v[f][r] ? inv_keep : 0.f;
      }
      da[f][r] = ok ? acc[f][r] * m : 0.f;
      ad[f][r] = p * m;
    }
  }

  float ds[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float part0 = grp16_sum(jac_dot2(da[0][r], pv[0][r], da[1][r], pv[1][r]));
    float part1 = grp16_sum(jac_dot2(da[2][r], pv[2][r], da[3][r], pv[3][r]));
    float dot_r = part0 + part1;
#pragma unroll
    for (int f = 0; f < 4; ++f)
      ds[f][r] = pv[f][r] * (da[f][r] - dot_r);
  }

  // V is dead: A_d^T takes its place. i columns 16..31 of the k step that
  // dV and dK read by rows hold no query: zero.
  wave_lds_sync();
  const short4v zero4 = {0, 0, 0, 0};
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f * 16 >= kr) break;
    short4v apack;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = row_grp + r;
      int j = f * 16 + col_base;
      float aval = (f < nf && i < Lq && j < Lk) ? ad[f][r] : 0.f;
      apack[r] = bf16_bits(aval);
    }
    int j = f * 16 + col_base;
    tile_store<true>(adt, j, row_grp, apack);
    tile_store<true>(adt, j, 16 + row_grp, zero4);
  }
  wave_lds_sync();

  const int nfrag_d = (D + 15) / 16;
  // dV[j strip] = A_d^T @ dO : one k step (i < 32)
  for (int js = 0; js < nf; ++js) {
    float4v accv[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                       {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    short8v a2 = frag_load<true>(adt, js * 16, 0, lane);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (f >= nfrag_d) break;
      short8v b2 = frag_load_tr(dos, 0, f * 16, lane);
      accv[f] = mfma_bf16(a2, b2, accv[f]);
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (f >= nfrag_d) break;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int j = js * 16 + row_grp + r;
        int d = f * 16 + col_base;
        if (j < Lk && d < D) {
          dv_out[(int64_t)b * dv_sb + h * dv_sh + j * dv_sl + d] =
              __float2bfloat16(accv[f][r]);
        }
      }
    }
  }

  // A_d^T is dead: dS^T takes its place
  wave_lds_sync();
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f * 16 >= kr) break;
    short4v dpack;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i = row_grp + r;
      int j = f * 16 + col_base;
      float dval = (f < nf && i < Lq && j < Lk) ? ds[f][r] : 0.f;
      dpack[r] = bf16_bits(dval * scale);
      if (ds_saved && f < nf && i < Lq && j < Lk) {
        ds_saved[idx4(b, h, i, j, H, Lq, Lk)] = __float2bfloat16(dval);
      }
    }
    int j = f * 16 + col_base;
    tile_store<true>(dst, j, row_grp, dpack);
    tile_store<true>(dst, j, 16 + row_grp, zero4);
  }
  wave_lds_sync();

  {  // dQ = (scale*dS) @ K over the live 32-row k steps
    float4v accq[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                       {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (f >= nfrag_d) break;
      for (int kk = 0; kk < kr; kk += 32) {
        short8v a = frag_load_tr(dst, kk, 0, lane);
        short8v bfr = frag_load_tr(ks, kk, f * 16, lane);
        accq[f] = mfma_bf16(a, bfr, accq[f]);
      }
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (f >= nfrag_d) break;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i = row_grp + r;
        int d = f * 16 + col_base;
        if (i < Lq && d < D) {
          dq_out[(int64_t)b * dq_sb + h * dq_sh + i * dq_sl + d] =
              __float2bfloat16(accq[f][r]);
        }
      }
    }
  }

  // dK[j strip] = (scale*dS)^T @ Q : one k step (i < 32)
  for (int js = 0; js < nf; ++js) {
    float4v acck[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                       {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    short8v a1 = frag_load<true>(dst, js * 16, 0, lane);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (f >= nfrag_d) break;
      short8v b1 = frag_load_tr(qs, 0, f * 16, lane);
      acck[f] = mfma_bf16(a1, b1, acck[f]);
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (f >= nfrag_d) break;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int j = js * 16 + row_grp + r;
        int d = f * 16 + col_base;
        if (j < Lk && d < D) {
          dk_out[(int64_t)b * dk_sb + h * dk_sh + j * dk_sl + d] =
              __float2bfloat16(acck[f][r]);
        }
      }
    }
  }
}

// Batch-reduce of the bf16 bias-grad buffer: out[h,i,j] = sum_b ds[b,h,i,j]
// in fp32 — replaces an ATen sum(0) that cost ~11.7 us/layer (BACKLOG r1
// item 2b). Two stages keep enough resident waves; fixed-order loops:
// deterministic.
constexpr int BS_CH = 16;

__global__ void batch_sum1_kernel(const __hip_bfloat16* __restrict__ in,
                                  float* __restrict__ tmp,
                                  int B, int64_t inner) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (int64_t)BS_CH * inner) return;
  int64_t j = tid % inner;
  int chunk = (int)(tid / inner);
  float acc = 0.f;
  for (int b = chunk; b < B; b += BS_CH)
    acc += to_f32(in[(int64_t)b * inner + j]);
  tmp[(int64_t)chunk * inner + j] = acc;
}

__global__ void batch_sum2_kernel(const float* __restrict__ tmp,
                                  float* __restrict__ out, int64_t inner) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= inner) return;
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < BS_CH; ++r) acc += tmp[(int64_t)r * inner + j];
  out[j] = acc;
}

// ------------------------------------------------------------------ hosts

// The one dispatch predicate of attn_fwd_mfma and attn_bwd_mfma. The
// environment knob GENREC_ATTN_SMALLQ=0 (read on every call) keeps every
// shape on the 64-row kernels, for A/B runs and the parity test.
static bool smallq_applies(int64_t Lq, int64_t Lk, int64_t D, int64_t act,
                           bool table_mode, bool backward) {
  if (Lq < 1 || Lq > SQ_LQ || Lk < 1 || Lk > (backward ? SQ_BWD_LK : TILE) ||
      D > TILE || D % 32 != 0 || act != 0 || table_mode)
    return false;
  const char* knob = std::getenv("GENREC_ATTN_SMALLQ");
  return !(knob && knob[0] == '0' && knob[1] == '\0');
}

std::string attn_mfma_path(int64_t Lq, int64_t Lk, int64_t D, int64_t act,
                           bool table_mode, bool backward) {
  return smallq_applies(Lq, Lk, D, act, table_mode, backward) ? "smallq"
                                                              : "tile64";
}

std::vector<torch::Tensor> attn_fwd_mfma(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> key_pad,
    c10::optional<torch::Tensor> add_mask,
    c10::optional<torch::Tensor> query_mask,
    double scale, bool causal, int64_t act, double dropout_p, int64_t seed,
    c10::optional<torch::Tensor> seed_dev,
    c10::optional<torch::Tensor> bias_bucket) {
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16);
  const int B = q.size(0), H = q.size(1), Lq = q.size(2), D = q.size(3);
  const int Lk = k.size(2);
  TORCH_CHECK(Lk <= TILE && D <= TILE && D % 32 == 0);
  // q/k/v may be transpose views (e.g. [B,L,H,D] -> [B,H,L,D]); only the
  // D axis must be unit-stride. Saves the .contiguous() copies around
  // every attention call.
  TORCH_CHECK(q.stride(3) == 1 && k.stride(3) == 1 && v.stride(3) == 1,
              "attn_fwd_mfma: innermost (D) stride must be 1");
  auto out = torch::empty_like(q);
  auto p_saved = torch::empty({B, H, Lq, Lk},
                              q.options().dtype(torch::kFloat32));
  torch::Tensor dmask;
  if (dropout_p > 0) {
    dmask = torch::empty({B, H, Lq, Lk}, q.options().dtype(torch::kUInt8));
  } else {
    dmask = torch::empty({0}, q.options().dtype(torch::kUInt8));
  }
  torch::Tensor bias_c, bucket_c;
  int bias_dim = 0;
  bool bias_bf16 = false;
  int n_buckets = 0;
  if (bias_bucket.has_value()) {
    // bucket mode: `bias` is the fp32 table [H*nb] (flattened rel-bias
    // embedding weight), `bias_bucket` the [Lq,Lk] int32 index map
    TORCH_CHECK(bias.has_value() &&
                bias->scalar_type() == torch::kFloat32);
    bias_c = bias->contiguous();
    bucket_c = bias_bucket->to(torch::kInt32).contiguous();
    n_buckets = (int)(bias_c.numel() / H);
  } else if (bias.has_value()) {
    TORCH_CHECK(bias->scalar_type() == torch::kFloat32 ||
                bias->scalar_type() == torch::kBFloat16);
    bias_c = bias->contiguous();
    bias_dim = bias_c.dim();
    bias_bf16 = bias_c.scalar_type() == torch::kBFloat16;
  }
  torch::Tensor am_f, qm_f;
  if (add_mask.has_value()) am_f = add_mask->to(torch::kFloat32).contiguous();
  if (query_mask.has_value())
    qm_f = query_mask->to(torch::kFloat32).contiguous();

  auto stream = at::cuda::getCurrentHIPStream();

  if (smallq_applies(Lq, Lk, D, act, bias_bucket.has_value(), false)) {
    dim3 sq_block(64 * SQ_HEADS);
    dim3 sq_grid((B * H + SQ_HEADS - 1) / SQ_HEADS);
    auto kern = attn_fwd_smallq_kernel<1>;   // instance by live fragments
    if (Lk > 48) kern = attn_fwd_smallq_kernel<4>;
    else if (Lk > 32) kern = attn_fwd_smallq_kernel<3>;
    else if (Lk > 16) kern = attn_fwd_smallq_kernel<2>;
    hipLaunchKernelGGL(kern, sq_grid, sq_block,
        SQ_HEADS * sq_fwd_lds(Lk), stream,
        reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(k.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(v.data_ptr()),
        bias_dim ? bias_c.data_ptr() : nullptr,
        key_pad.has_value() ? key_pad->data_ptr<bool>() : nullptr,
        add_mask.has_value() ? am_f.data_ptr<float>() : nullptr,
        query_mask.has_value() ? qm_f.data_ptr<float>() : nullptr,
        reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),
        p_saved.data_ptr<float>(),
        dropout_p > 0 ? dmask.data_ptr<unsigned char>() : nullptr,
        seed_dev.has_value()
            ? reinterpret_cast<const unsigned int*>(seed_dev->data_ptr())
            : nullptr,
        B, H, Lq, Lk, D,
        q.stride(0), q.stride(1), q.stride(2),
        k.stride(0), k.stride(1), k.stride(2),
        v.stride(0), v.stride(1), v.stride(2),
        out.stride(0), out.stride(1), out.stride(2),
        (float)scale, bias_dim, bias_bf16, causal,
        (float)dropout_p, (unsigned int)seed);
    return {out, p_saved, dmask};
  }

  const int q_tile = TILE;
  dim3 block(256);
  dim3 grid(B * H, (Lq + q_tile - 1) / q_tile);
  size_t smem = 4 * TILE * 128;

#define LAUNCH_FWD_MFMA(SILU)                                                  \
  hipLaunchKernelGGL((attn_fwd_mfma_kernel<SILU>), grid, block, smem, stream,  \
      reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),                   \
      reinterpret_cast<const __hip_bfloat16*>(k.data_ptr()),                   \
      reinterpret_cast<const __hip_bfloat16*>(v.data_ptr()),                   \
      (bias_dim || n_buckets) ? bias_c.data_ptr() : nullptr,                   \
      n_buckets ? bucket_c.data_ptr<int>() : nullptr,                          \
      key_pad.has_value() ? key_pad->data_ptr<bool>() : nullptr,               \
      add_mask.has_value() ? am_f.data_ptr<float>() : nullptr,                 \
      query_mask.has_value() ? qm_f.data_ptr<float>() : nullptr,               \
      reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),                       \
      p_saved.data_ptr<float>(),                                               \
      dropout_p > 0 ? dmask.data_ptr<unsigned char>() : nullptr,               \
      seed_dev.has_value()                                                     \
          ? reinterpret_cast<const unsigned int*>(seed_dev->data_ptr())        \
          : nullptr,                                                           \
      B, H, Lq, Lk, D, n_buckets,                                              \
      q.stride(0), q.stride(1), q.stride(2),                                   \
      k.stride(0), k.stride(1), k.stride(2),                                   \
      v.stride(0), v.stride(1), v.stride(2),                                   \
      out.stride(0), out.stride(1), out.stride(2),                             \
      (float)scale, bias_dim, bias_bf16, causal,                               \
      (float)dropout_p, (unsigned int)seed, q_tile)

  if (act == 0) LAUNCH_FWD_MFMA(false);
  else LAUNCH_FWD_MFMA(true);
#undef LAUNCH_FWD_MFMA
  return {out, p_saved, dmask};
}

std::vector<torch::Tensor> attn_bwd_mfma(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor p_saved, torch::Tensor drop_mask,
    c10::optional<torch::Tensor> query_mask,
    double scale, int64_t act, double dropout_p, int64_t seed,
    bool bias_grad, int64_t bias_dim,
    c10::optional<torch::Tensor> bias_bucket, int64_t n_buckets,
    c10::optional<torch::Tensor> dqkv_out,
    c10::optional<torch::Tensor> dkv_out, int64_t dk_col, int64_t dv_col) {
  (void)seed;
  const int B = q.size(0), H = q.size(1), Lq = q.size(2), D = q.size(3);
  const int Lk = k.size(2);
  TORCH_CHECK(Lq <= TILE && Lk <= TILE && D % 32 == 0);
  TORCH_CHECK(dout.stride(3) == 1 && q.stride(3) == 1 && k.stride(3) == 1 &&
                  v.stride(3) == 1,
              "attn_bwd_mfma: innermost (D) stride must be 1");
  TORCH_CHECK(!(dqkv_out.has_value() && dkv_out.has_value()),
              "attn_bwd_mfma: dqkv_out and dkv_out are mutually exclusive");
  torch::Tensor dq, dk, dv;
  if (dkv_out.has_value()) {
    // packed cross-attention gradient: dk and dv are [B,H,Lk,D] views of
    // two H*D-wide column blocks (at element columns dk_col and dv_col) of
    // one [B,Lk,W] buffer that several calls share — each call fills its
    // own blocks, so the K/V projections of all decoder layers get their
    // output gradient as one tensor. dq stays a fresh tensor; Lq != Lk is
    // fine. The kernels store dK/dV element by element through the
    // strides, so a row stride of W and a column offset need no alignment
    // beyond the element's own.
    const int64_t HD = (int64_t)H * D;
    TORCH_CHECK(dkv_out->scalar_type() == torch::kBFloat16,
                "attn_bwd_mfma: dkv_out must be bf16");
    TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
                    k.scalar_type() == torch::kBFloat16 &&
                    v.scalar_type() == torch::kBFloat16,
                "attn_bwd_mfma: dkv_out needs bf16 q/k/v");
    TORCH_CHECK(dkv_out->is_contiguous() && dkv_out->dim() == 3,
                "attn_bwd_mfma: dkv_out must be a contiguous [B, Lk, W] "
                "tensor");
    TORCH_CHECK(dkv_out->device() == q.device(),
                "attn_bwd_mfma: dkv_out must be on the device of q");
    TORCH_CHECK(k.size(0) == B && k.size(1) == H && k.size(3) == D &&
                    v.sizes() == k.sizes(),
                "attn_bwd_mfma: k/v must be [B, H, Lk, D]");
    const int64_t W = dkv_out->size(2);
    TORCH_CHECK(dkv_out->size(0) == B && dkv_out->size(1) == Lk &&
                    W >= 2 * HD && W % HD == 0,
                "attn_bwd_mfma: dkv_out must be [B, Lk, n_blocks*H*D] with "
                "n_blocks >= 2");
    TORCH_CHECK(dk_col >= 0 && dv_col >= 0 && dk_col % HD == 0 &&
                    dv_col % HD == 0 && dk_col + HD <= W &&
                    dv_col + HD <= W && dk_col != dv_col,
                "attn_bwd_mfma: dk_col/dv_col must be distinct multiples of "
                "H*D inside dkv_out's last dimension");
    auto blocks = dkv_out->view({B, Lk, W / HD, H, D});
    dq = torch::empty_like(q);
    dk = blocks.select(2, dk_col / HD).transpose(1, 2);
    dv = blocks.select(2, dv_col / HD).transpose(1, 2);
  } else if (dqkv_out.has_value()) {
    // packed self-attention gradient: dq/dk/dv are [B,H,L,D] views of the
    // three column blocks of one [B,L,3*H*D] buffer, which is the layout
    // the fused qkv projection's backward reads — the kernels write
    // through the strides, so no concatenation follows
    TORCH_CHECK(Lq == Lk, "attn_bwd_mfma: dqkv_out needs Lq == Lk");
    TORCH_CHECK(dqkv_out->scalar_type() == torch::kBFloat16 &&
                    dqkv_out->is_contiguous() && dqkv_out->dim() == 3 &&
                    dqkv_out->size(0) == B && dqkv_out->size(1) == Lq &&
                    dqkv_out->size(2) == (int64_t)3 * H * D &&
                    dqkv_out->device() == q.device(),
                "attn_bwd_mfma: dqkv_out must be contiguous bf16 "
                "[B, L, 3*H*D]");
    auto parts = dqkv_out->view({B, Lq, 3, H, D});
    dq = parts.select(2, 0).transpose(1, 2);
    dk = parts.select(2, 1).transpose(1, 2);
    dv = parts.select(2, 2).transpose(1, 2);
  } else {
    dq = torch::empty_like(q);
    dk = torch::empty_like(k);
    dv = torch::empty_like(v);
  }
  torch::Tensor ds_saved, bucket_c, dtab_partial;
  __hip_bfloat16* ds_ptr = nullptr;
  const bool table_mode = bias_grad && bias_bucket.has_value();
  if (table_mode) {
    bucket_c = bias_bucket->to(torch::kInt32).contiguous();
    dtab_partial = torch::empty({(int64_t)B * H, n_buckets},
                                q.options().dtype(torch::kFloat32));
  } else if (bias_grad) {
    ds_saved = torch::empty({B, H, Lq, Lk},
                            q.options().dtype(torch::kBFloat16));
    ds_ptr = reinterpret_cast<__hip_bfloat16*>(ds_saved.data_ptr());
  }
  torch::Tensor qm_f;
  if (query_mask.has_value())
    qm_f = query_mask->to(torch::kFloat32).contiguous();
  auto stream = at::cuda::getCurrentHIPStream();
  const bool smallq =
      smallq_applies(Lq, Lk, D, act, bias_bucket.has_value(), true);
  dim3 block(512);  // 8 waves: pairs own strips, halves split fragments
  dim3 grid(B * H);
  size_t smem = 6 * TILE * 128 + 2 * TILE * sizeof(float)
      + (table_mode ? (size_t)n_buckets * sizeof(float) : 0);

  if (smallq) {
    dim3 sq_block(64 * SQ_HEADS);
    dim3 sq_grid((B * H + SQ_HEADS - 1) / SQ_HEADS);
    static_assert(SQ_BWD_LK == 16, "one key strip: instance <1>");
    hipLaunchKernelGGL(attn_bwd_smallq_kernel<1>, sq_grid, sq_block,
        SQ_HEADS * sq_bwd_lds(Lk), stream,
        reinterpret_cast<const __hip_bfloat16*>(dout.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(k.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(v.data_ptr()),
        p_saved.data_ptr<float>(),
        query_mask.has_value() ? qm_f.data_ptr<float>() : nullptr,
        dropout_p > 0 ? drop_mask.data_ptr<unsigned char>() : nullptr,
        reinterpret_cast<__hip_bfloat16*>(dq.data_ptr()),
        reinterpret_cast<__hip_bfloat16*>(dk.data_ptr()),
        reinterpret_cast<__hip_bfloat16*>(dv.data_ptr()), ds_ptr,
        B, H, Lq, Lk, D,
        dout.stride(0), dout.stride(1), dout.stride(2),
        q.stride(0), q.stride(1), q.stride(2),
        k.stride(0), k.stride(1), k.stride(2),
        v.stride(0), v.stride(1), v.stride(2),
        dq.stride(0), dq.stride(1), dq.stride(2),
        dk.stride(0), dk.stride(1), dk.stride(2),
        dv.stride(0), dv.stride(1), dv.stride(2),
        (float)scale, (float)dropout_p);
  }

#define LAUNCH_BWD_DS(SILU)                                                    \
  hipLaunchKernelGGL((attn_bwd_ds_kernel<SILU>), grid, block, smem, stream,    \
      reinterpret_cast<const __hip_bfloat16*>(dout.data_ptr()),                \
      reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),                   \
      reinterpret_cast<const __hip_bfloat16*>(k.data_ptr()),                   \
      reinterpret_cast<const __hip_bfloat16*>(v.data_ptr()),                   \
      p_saved.data_ptr<float>(),                                               \
      query_mask.has_value() ? qm_f.data_ptr<float>() : nullptr,               \
      dropout_p > 0 ? drop_mask.data_ptr<unsigned char>() : nullptr,           \
      reinterpret_cast<__hip_bfloat16*>(dq.data_ptr()),                        \
      reinterpret_cast<__hip_bfloat16*>(dk.data_ptr()),                        \
      reinterpret_cast<__hip_bfloat16*>(dv.data_ptr()), ds_ptr,                \
      table_mode ? bucket_c.data_ptr<int>() : nullptr,                         \
      table_mode ? dtab_partial.data_ptr<float>() : nullptr,                   \
      (int)n_buckets,                                                          \
      B, H, Lq, Lk, D,                                                         \
      dout.stride(0), dout.stride(1), dout.stride(2),                          \
      q.stride(0), q.stride(1), q.stride(2),                                   \
      k.stride(0), k.stride(1), k.stride(2),                                   \
      v.stride(0), v.stride(1), v.stride(2),                                   \
      dq.stride(0), dq.stride(1), dq.stride(2),                                \
      dk.stride(0), dk.stride(1), dk.stride(2),                                \
      dv.stride(0), dv.stride(1), dv.stride(2),                                \
      (float)scale, (float)dropout_p)

  if (!smallq) {
    if (act == 0) LAUNCH_BWD_DS(false);
    else LAUNCH_BWD_DS(true);
  }
#undef LAUNCH_BWD_DS

  torch::Tensor dbias;
  if (table_mode) {
    // deterministic reduce of the per-block table-grad partials:
    // [B*H, nb] -> view [B, H*nb] -> replay-safe colsum -> [H*nb]
    dbias = colsum(dtab_partial.view({B, (int64_t)H * n_buckets}));
  } else if (bias_grad) {
    if (bias_dim == 3) {  // bf16 per-element grads, fp32 batch reduce
      const int64_t inner = (int64_t)H * Lq * Lk;
      dbias = torch::empty({H, Lq, Lk},
                           q.options().dtype(torch::kFloat32));
      auto tmp = torch::empty({16, inner},
                              q.options().dtype(torch::kFloat32));
      dim3 rblock(256);
      dim3 rgrid1((unsigned)((16 * inner + 255) / 256));
      hipLaunchKernelGGL(batch_sum1_kernel, rgrid1, rblock, 0, stream,
          reinterpret_cast<const __hip_bfloat16*>(ds_saved.data_ptr()),
          tmp.data_ptr<float>(), B, inner);
      dim3 rgrid2((unsigned)((inner + 255) / 256));
      hipLaunchKernelGGL(batch_sum2_kernel, rgrid2, rblock, 0, stream,
          tmp.data_ptr<float>(), dbias.data_ptr<float>(), inner);
    } else {
      dbias = ds_saved.to(torch::kFloat32);
    }
  } else {
    dbias = torch::empty({0}, q.options().dtype(torch::kFloat32));
  }
  return {dq, dk, dv, dbias};
}

}  // namespace genrec
