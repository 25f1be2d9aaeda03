// Shared-prefix beam-search decode attention (bf16, forward only, D in
// {64,128}) for LCRec.generate_topk.
//
// The W beams of a prompt share the prompt's keys and values and differ only
// in the t <= 16 tokens generated so far. One decode step therefore is
//
//   * a prefix phase over k_pre/v_pre [B,Hkv,Lp,D] (one copy per prompt):
//     the W*g query rows that read one (prompt, KV head) are packed into
//     64-row Q tiles (row r = w*g + gq is beam w, query head hk*g + gq), so
//     a prompt K/V tile is staged once per (prompt, KV head, Q tile) instead
//     of once per (beam, query head). A K tile is processed by the same
//     flash_fwd_tile step (core/flash_strip.h) as in gqa_fwd_kernel, with
//     the key-only mask: no causal test, every prefix key precedes every
//     decode query. The K tiles are split over blockIdx.y; each split
//     writes an unnormalised fp32 partial (m, l, acc[D]) per row.
//   * a suffix phase over the generated tokens: row (w, gq) sees the t keys
//     k_suf[b, s, anc[b,w,s], hk, :], s < t. They differ per beam, so this
//     is plain VALU work, one wave per output row, in the combine kernel.
//   * the combine: the same wave folds the prefix partials in split order,
//     then the suffix partial, normalises and stores bf16. No atomics: the
//     same inputs and the same split count give the same bits.
//
// Nothing is ever read from suffix slots s >= t or from anc[..., s >= t].
// Padded prefix keys are staged as zeros, so whatever they hold (NaN
// included) cannot reach the output through 0 * x.
//
// Variable-length prefix (VARLEN = true; beam_attn_varlen_fwd): k_pre/v_pre
// are the token-major [Ttot,Hkv,D] K/V of a packed prefill and cu_seqlens
// [B+1] (int32, device) gives prompt b the tokens [cu[b], cu[b+1]), clamped
// by gqa_seq to [0,Ttot] and to end >= start, so no cu_seqlens content
// addresses outside the tensors. There is no pad mask. A block's split
// ranges come from its own prompt's length, so per prompt the tiles, splits
// and fold order, and with them the bits, are those of the fixed-length
// kernel on that prompt alone (B = 1, no pad, same split count). Splits
// beyond a short prompt's tiles, and every split of an empty prompt, take
// the empty-split exit; an empty prompt's rows then are the suffix softmax.

#include <ATen/hip/HIPContext.h>

#include "../core/attn_host.h"

namespace genrec {

namespace {

constexpr int BEAM_MAX_T = 16;

// ------------------------------------------------------------ prefix phase

template <int D, bool VARLEN>
__global__ void __launch_bounds__(256)
beam_prefix_kernel(FlashView q,                       // [B*W,Hq,1,D]
                   FlashView k, FlashView v,          // [B,Hkv,Lp,D] | [Ttot,Hkv,D]
                   const bool* __restrict__ pre_pad,  // null | [B,Lp]
                   float* __restrict__ ws_ml,         // [splits, rows, 2]
                   float* __restrict__ ws_acc,        // [splits, rows, D]
                   int W, int Hq, int Hkv, int Lp_max, int qtiles,
                   int64_t rows_total, float scale,
                   const int* __restrict__ cu, int Ttot) {  // VARLEN only
  constexpr int RS = D * 2;
  const int g = Hq / Hkv;
  const int n_rows = W * g;  // rows of this (prompt, KV head)
  const int qt = blockIdx.x % qtiles;
  const int hk = (blockIdx.x / qtiles) % Hkv;
  const int b = blockIdx.x / (qtiles * Hkv);
  const int split = blockIdx.y;

  const int tid = threadIdx.x;
  const Strip w(tid);

  // this prompt's prefix: Lp_max keys, or (VARLEN) the clamped token range
  // [cu[b], cu[b+1]) of the packed K/V; uniform per block
  const GqaSeq<VARLEN> sq = gqa_seq<VARLEN>(cu, Ttot, b, Lp_max, Lp_max, 0);
  const int Lp = sq.Lk;

  // this split's K tiles
  const int nkt = (Lp + TILE - 1) / TILE;
  const int per = (nkt + gridDim.y - 1) / gridDim.y;
  const int kt_begin = min(split * per, nkt) * TILE;
  const int kt_end = min(min((split + 1) * per, nkt) * TILE, Lp);

  // workspace row of each of this lane's 4 C-fragment rows (-1: unused)
  int64_t ws_row[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int rr = qt * TILE + w.row + r;
    int beam = rr / g, gq = rr % g;
    ws_row[r] = rr < n_rows
        ? (int64_t)split * rows_total +
              ((int64_t)b * W + beam) * Hq + hk * g + gq
        : -1;
  }

  if (kt_begin >= kt_end) {  // empty split: an empty state, acc never read
    if (w.col == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (ws_row[r] < 0) continue;
        ws_ml[ws_row[r] * 2] = -INFINITY;
        ws_ml[ws_row[r] * 2 + 1] = 0.f;
      }
    }
    return;
  }

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qs = smem;               // [64][D]   packed Q rows
  char* ks = qs + TILE * RS;     // [64][D]   K rows (per tile)
  char* vt = ks + TILE * RS;     // [D][64]   V^T (per tile)
  char* ps = vt + D * 128;       // [64][64]  P (per tile)

  // packed Q tile: row rr is beam rr / g, query head hk*g + rr % g
  for (int idx = tid; idx < TILE * (D / 8); idx += 256) {
    int row = idx / (D / 8);
    int d0 = (idx % (D / 8)) * 8;
    int rr = qt * TILE + row;
    int beam = rr / g, gq = rr % g;
    short8v val = load8(
        q.p, ((int64_t)b * W + beam) * q.b + (int64_t)(hk * g + gq) * q.h + d0,
        rr < n_rows);
    tile_store(qs, row, d0, val, RS);
  }

  RunningSoftmax sm;
  float4v accO[D / 16] = {};

  const __hip_bfloat16* kb = sq.rows(k, hk);
  const __hip_bfloat16* vb = sq.rows(v, hk);
  const bool* pad =
      (!VARLEN && pre_pad) ? pre_pad + (int64_t)b * Lp : nullptr;

  for (int kt0 = kt_begin; kt0 < kt_end; kt0 += TILE) {
    __syncthreads();  // previous iteration's ks/vt fully consumed
    gstage<D, true, false>(kb, k.l, kt0, Lp, ks, nullptr, tid, pad);
    gstage<D, false, true>(vb, v.l, kt0, Lp, nullptr, vt, tid, pad);
    __syncthreads();
    flash_fwd_tile<D>(qs, ks, vt, ps, kt0, Lp, pad, KeyMask(), scale, sm, accO,
                      w);
  }

  // ---- unnormalised partial of the live rows
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (ws_row[r] < 0) continue;
    if (w.col == 0) {
      ws_ml[ws_row[r] * 2] = sm.m[r];
      ws_ml[ws_row[r] * 2 + 1] = sm.l[r];
    }
    if (sm.empty(r)) continue;  // empty state: acc never read
#pragma unroll
    for (int f = 0; f < D / 16; ++f) {
      ws_acc[ws_row[r] * D + f * 16 + w.col] = accO[f][r];
    }
  }
}

// ------------------------------------------------- suffix phase + combine

// Fold the partial (m_p, l_p, a_p[]) into the running (m, l, a[]). Empty
// states (m = -inf, l = 0) on either side are guarded: no exp(-inf - -inf).
template <int E>
__device__ __forceinline__ void beam_fold(float& m, float& l, float (&a)[E],
                                          float m_p, float l_p,
                                          const float (&a_p)[E]) {
  if (m_p == -INFINITY) return;
  float m_new = fmaxf(m, m_p);
  float ca = (m == -INFINITY) ? 0.f : __expf(m - m_new);
  float cb = __expf(m_p - m_new);
  l = l * ca + l_p * cb;
#pragma unroll
  for (int e = 0; e < E; ++e) a[e] = a[e] * ca + a_p[e] * cb;
  m = m_new;
}

// One wave per output row (b, w, h); lane owns E = D/64 adjacent columns.
template <int D>
__global__ void __launch_bounds__(256)
beam_combine_kernel(FlashView q,                               // [B*W,Hq,1,D]
                    const __hip_bfloat16* __restrict__ k_suf,  // [B,T,W,Hkv,D]
                    const __hip_bfloat16* __restrict__ v_suf,
                    const int* __restrict__ anc,               // [B,W,T]
                    const float* __restrict__ ws_ml,
                    const float* __restrict__ ws_acc,
                    __hip_bfloat16* __restrict__ out,          // [B*W,1,Hq,D]
                    int W, int Hq, int Hkv, int T, int t, int splits,
                    int64_t rows_total, float scale) {
  constexpr int E = D / 64;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows_total) return;  // wave-uniform
  const int h = row % Hq;
  const int64_t bw = row / Hq;
  const int w = bw % W;
  const int64_t b = bw / W;
  const int hk = h / (Hq / Hkv);
  const int d0 = lane * E;

  float qv[E];
  {
    const __hip_bfloat16* qp = q.p + bw * q.b + (int64_t)h * q.h + d0;
#pragma unroll
    for (int e = 0; e < E; ++e) qv[e] = to_f32(qp[e]);
  }

  // ---- suffix scores; a live slot whose ancestor is not a beam slot is
  // treated as masked rather than read
  float sc[BEAM_MAX_T];
  int src[BEAM_MAX_T];
  float m_s = -INFINITY;
#pragma unroll
  for (int s = 0; s < BEAM_MAX_T; ++s) {
    sc[s] = -INFINITY;
    src[s] = -1;
    if (s < t) {
      int a = anc[(b * W + w) * T + s];
      if (a >= 0 && a < W) {
        src[s] = a;
        const __hip_bfloat16* kp =
            k_suf + ((((b * T + s) * W + a) * Hkv + hk) * D + d0);
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) dot += qv[e] * to_f32(kp[e]);
        sc[s] = __fmul_rn(wave_sum(dot), scale);
        m_s = fmaxf(m_s, sc[s]);
      }
    }
  }
  float l_s = 0.f;
  float a_s[E];
#pragma unroll
  for (int e = 0; e < E; ++e) a_s[e] = 0.f;
#pragma unroll
  for (int s = 0; s < BEAM_MAX_T; ++s) {
    if (s < t && src[s] >= 0 && sc[s] != -INFINITY) {
      float p = __expf(sc[s] - m_s);
      l_s += p;
      const __hip_bfloat16* vp =
          v_suf + ((((b * T + s) * W + src[s]) * Hkv + hk) * D + d0);
#pragma unroll
      for (int e = 0; e < E; ++e) a_s[e] += p * to_f32(vp[e]);
    }
  }

  // ---- fold: prefix partials in split order, then the suffix
  float m = -INFINITY, l = 0.f;
  float a[E];
#pragma unroll
  for (int e = 0; e < E; ++e) a[e] = 0.f;
  for (int p = 0; p < splits; ++p) {
    const int64_t wr = (int64_t)p * rows_total + row;
    float m_p = ws_ml[wr * 2], l_p = ws_ml[wr * 2 + 1];
    if (m_p == -INFINITY) continue;  // acc of an empty state is not written
    float a_p[E];
#pragma unroll
    for (int e = 0; e < E; ++e) a_p[e] = ws_acc[wr * D + d0 + e];
    beam_fold<E>(m, l, a, m_p, l_p, a_p);
  }
  beam_fold<E>(m, l, a, m_s, l_s, a_s);

  const float inv = (l > 0.f) ? 1.0f / l : 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    out[row * D + d0 + e] = __float2bfloat16(a[e] * inv);
  }
}

// ------------------------------------------------------------------ hosts

// k/v: [B,Hkv,Lp,D] with pad, or (VARLEN) token-major [Ttot,Hkv,D] with the
// device offsets cu [B+1]; Lp then is only the host's upper bound.
template <int D, bool VARLEN>
void beam_launch(const torch::Tensor& q, const torch::Tensor& k,
                 const torch::Tensor& v, const bool* pad,
                 const torch::Tensor& k_suf, const torch::Tensor& v_suf,
                 const torch::Tensor& anc, torch::Tensor& ws_ml,
                 torch::Tensor& ws_acc, torch::Tensor& out, int B, int W,
                 int Hq, int Hkv, int Lp, int T, int t, int splits,
                 float scale, const int* cu, int Ttot) {
  auto stream = at::cuda::getCurrentHIPStream();
  const int g = Hq / Hkv;
  const int qtiles = (W * g + TILE - 1) / TILE;
  const int64_t rows_total = (int64_t)B * W * Hq;
  const FlashView qv = view_bhld(q);  // one row per (beam, head)
  {
    dim3 grid((unsigned int)((int64_t)B * Hkv * qtiles), splits);
    size_t smem = 2 * TILE * D * 2 + D * 128 + TILE * 128;  // 56 KiB at 128
    const FlashView kv = VARLEN ? view_thd(k) : view_bhld(k);
    const FlashView vv = VARLEN ? view_thd(v) : view_bhld(v);
    hipLaunchKernelGGL((beam_prefix_kernel<D, VARLEN>), grid, dim3(256), smem,
        stream, qv, kv, vv, pad, ws_ml.data_ptr<float>(),
        ws_acc.data_ptr<float>(), W, Hq, Hkv, Lp, qtiles, rows_total, scale,
        cu, Ttot);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  {
    dim3 grid((unsigned int)((rows_total + 3) / 4));
    hipLaunchKernelGGL(beam_combine_kernel<D>, grid, dim3(256), 0, stream,
        qv, bf16_cptr(k_suf), bf16_cptr(v_suf), anc.data_ptr<int>(),
        ws_ml.data_ptr<float>(), ws_acc.data_ptr<float>(), bf16_ptr(out), W,
        Hq, Hkv, T, t, splits, rows_total, scale);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
}

}  // namespace

// Split count for the prefix phase: about 2 workgroups per CU, at most one
// split per 64-key tile. rows = W * g packed query rows per (prompt, KV head).
int64_t beam_attn_pick_splits(int64_t B, int64_t Hkv, int64_t rows,
                              int64_t Lp) {
  const int64_t cus =
      at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int64_t base =
      std::max<int64_t>(B * Hkv * ((rows + TILE - 1) / TILE), 1);
  const int64_t nkt = std::max<int64_t>((Lp + TILE - 1) / TILE, 1);
  const int64_t want = (2 * cus + base - 1) / base;
  return std::max<int64_t>(1, std::min<int64_t>(want, nkt));
}

namespace {

// What the two hosts share once each has checked its prefix layout and read
// B, Hkv and the prefix length Lp (VARLEN: the host's upper bound) from it:
// the checks of q, the suffix slots and anc, the split choice, the
// workspaces and the launch. kn/vn are the kernel-readable prefix.
template <bool VARLEN>
torch::Tensor beam_run(const torch::Tensor& q, const torch::Tensor& k_pre,
                       const torch::Tensor& v_pre, const torch::Tensor& kn,
                       const torch::Tensor& vn, const bool* pad,
                       const torch::Tensor& k_suf, const torch::Tensor& v_suf,
                       const torch::Tensor& anc, int64_t B, int64_t Hkv,
                       int64_t Lp, int64_t t, double scale, int64_t splits,
                       const int* cu = nullptr, int Ttot = 0) {
  TORCH_CHECK(q.is_cuda() && k_pre.is_cuda() && v_pre.is_cuda() &&
                  k_suf.is_cuda() && v_suf.is_cuda() && anc.is_cuda(),
              "beam_attn: all tensors must be GPU tensors");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
                  k_pre.scalar_type() == torch::kBFloat16 &&
                  v_pre.scalar_type() == torch::kBFloat16 &&
                  k_suf.scalar_type() == torch::kBFloat16 &&
                  v_suf.scalar_type() == torch::kBFloat16,
              "beam_attn: q/k/v must be bfloat16");
  TORCH_CHECK(q.dim() == 4 && q.size(2) == 1,
              "beam_attn: q must be [B*W,Hq,1,D]");
  const int64_t BW = q.size(0), Hq = q.size(1), D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128,
              "beam_attn: head dim must be 64 or 128, got ", D);
  TORCH_CHECK(k_pre.size(-1) == D, "beam_attn: k_pre head dim mismatch");
  TORCH_CHECK(Hkv >= 1 && Hq % Hkv == 0, "beam_attn: Hq (", Hq,
              ") must be a multiple of Hkv (", Hkv, ")");
  TORCH_CHECK(B >= 1 && BW >= B && BW % B == 0,
              "beam_attn: q batch must be a multiple of the prompt batch");
  const int64_t W = BW / B;
  TORCH_CHECK(k_suf.dim() == 5 && k_suf.size(0) == B && k_suf.size(2) == W &&
                  k_suf.size(3) == Hkv && k_suf.size(4) == D &&
                  v_suf.sizes() == k_suf.sizes() && k_suf.is_contiguous() &&
                  v_suf.is_contiguous(),
              "beam_attn: k_suf/v_suf must be contiguous [B,T,W,Hkv,D]");
  const int64_t T = k_suf.size(1);
  TORCH_CHECK(T >= 1 && T <= BEAM_MAX_T && t >= 1 && t <= T,
              "beam_attn: need 1 <= t <= T <= 16, got t=", t, " T=", T);
  TORCH_CHECK(anc.scalar_type() == torch::kInt32 && anc.dim() == 3 &&
                  anc.size(0) == B && anc.size(1) == W && anc.size(2) == T &&
                  anc.is_contiguous(),
              "beam_attn: anc must be a contiguous int32 [B,W,T]");
  TORCH_CHECK(BW * Hq < (int64_t(1) << 31), "beam_attn: batch too large");
  // q has one row per (beam, head): only k/v carry a row stride
  torch::Tensor qn = kernel_readable(q, 2);

  const int64_t g = Hq / Hkv;
  int64_t S = splits > 0 ? splits : beam_attn_pick_splits(B, Hkv, W * g, Lp);
  TORCH_CHECK(S <= 1024, "beam_attn: at most 1024 splits");
  auto f32 = q.options().dtype(torch::kFloat32);
  auto ws_ml = torch::empty({S, BW * Hq, 2}, f32);
  auto ws_acc = torch::empty({S, BW * Hq, D}, f32);
  auto out = torch::empty({BW, 1, Hq, D}, q.options());
  dispatch_head_dim(D, [&](auto d) {
    beam_launch<decltype(d)::value, VARLEN>(
        qn, kn, vn, pad, k_suf, v_suf, anc, ws_ml, ws_acc, out, B, W, Hq, Hkv,
        Lp, T, t, S, (float)scale, cu, Ttot);
  });
  return out;
}

}  // namespace

// One beam-search decode step over a shared prompt prefix; see the header
// comment. splits <= 0: pick. Returns out [B*W, 1, Hq, D].
torch::Tensor beam_attn_fwd(torch::Tensor q, torch::Tensor k_pre,
                            torch::Tensor v_pre,
                            c10::optional<torch::Tensor> pre_pad,
                            torch::Tensor k_suf, torch::Tensor v_suf,
                            torch::Tensor anc, int64_t t, double scale,
                            int64_t splits) {
  TORCH_CHECK(k_pre.dim() == 4 && v_pre.sizes() == k_pre.sizes(),
              "beam_attn: k_pre/v_pre must be [B,Hkv,Lp,D]");
  const int64_t B = k_pre.size(0), Hkv = k_pre.size(1), Lp = k_pre.size(2);
  TORCH_CHECK(Lp >= 1, "beam_attn: empty prefix");
  if (pre_pad.has_value()) {
    TORCH_CHECK(pre_pad->is_cuda() &&
                    pre_pad->scalar_type() == torch::kBool &&
                    pre_pad->dim() == 2 && pre_pad->size(0) == B &&
                    pre_pad->size(1) == Lp,
                "beam_attn: pre_pad must be a bool [B,Lp] GPU tensor");
  }
  torch::Tensor padc;
  const bool* pad = pad_ptr(pre_pad, padc);
  // [B,Hkv,Lp,D]: batch, head and row strides
  return beam_run<false>(q, k_pre, v_pre, kernel_readable(k_pre, 3),
                         kernel_readable(v_pre, 3), pad, k_suf, v_suf, anc, B,
                         Hkv, Lp, t, scale, splits);
}

// The same step over a packed prefill: k_pre/v_pre are token-major
// [Ttot,Hkv,D] views and prompt b owns the tokens [cu[b], cu[b+1]) of them,
// clamped into [0,Ttot]. cu_seqlens stays on the device; max_prefix (a host
// int, >= the longest prompt) only feeds the split choice. Per prompt the
// result is bit-identical to beam_attn_fwd on that prompt alone (B = 1,
// Lp = its length, no pre_pad) with the same splits.
torch::Tensor beam_attn_varlen_fwd(torch::Tensor q, torch::Tensor k_pre,
                                   torch::Tensor v_pre,
                                   torch::Tensor cu_seqlens,
                                   int64_t max_prefix, torch::Tensor k_suf,
                                   torch::Tensor v_suf, torch::Tensor anc,
                                   int64_t t, double scale, int64_t splits) {
  TORCH_CHECK(k_pre.dim() == 3 && v_pre.sizes() == k_pre.sizes(),
              "beam_attn: k_pre/v_pre must be [Ttot,Hkv,D]");
  TORCH_CHECK(cu_seqlens.is_cuda() &&
                  cu_seqlens.scalar_type() == torch::kInt32 &&
                  cu_seqlens.dim() == 1 && cu_seqlens.numel() >= 2 &&
                  cu_seqlens.is_contiguous() &&
                  cu_seqlens.device() == k_pre.device(),
              "beam_attn: cu_seqlens must be a contiguous int32 [B+1] tensor "
              "on the device of k_pre");
  const int64_t B = cu_seqlens.numel() - 1;
  const int64_t Ttot = k_pre.size(0), Hkv = k_pre.size(1);
  TORCH_CHECK(Ttot < (int64_t(1) << 31), "beam_attn: too many tokens");
  TORCH_CHECK(max_prefix >= 0 && max_prefix < (int64_t(1) << 31),
              "beam_attn: max_prefix out of range");
  // [Ttot,Hkv,D]: token and head strides
  return beam_run<true>(q, k_pre, v_pre, kernel_readable(k_pre, 2),
                        kernel_readable(v_pre, 2), nullptr, k_suf, v_suf, anc,
                        B, Hkv, max_prefix, t, scale, splits,
                        cu_seqlens.data_ptr<int>(), (int)Ttot);
}

}  // namespace genrec
