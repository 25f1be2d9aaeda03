// Tiled HSTU pointwise attention for sequences beyond one 64-row tile, gfx950.
//
// Same op as hstu_attn.hip: S = Q K^T + position bias + temporal bias,
// causal / key-pad masks at -1e9, P = SiLU(S), O = P V. SiLU scores need no
// running maximum and no rescale, so the forward is a plain K-tile loop
// accO += SiLU(S_t) V_t over the tiles at or below the diagonal, and the
// backward recomputes S per tile: the bias is a function of (j - i, ts_i,
// ts_j), so nothing of size L x L is read, written or saved.
//
// Position bias: the [L,L] bucket table of RelativePositionBias is Toeplitz,
// bucket(i, j) = rel_bucket[j - i + L - 1] with rel_bucket an int32 [2L-1]
// built on the host by the module's own _bucket. A (Q tile, K tile) pair
// touches 127 consecutive entries of it, staged into LDS per tile; the
// head's columns of the two bias tables sit in LDS as floats for the whole
// block.
//
// Forward: grid (B*H, ceil(L/64)), one block of four waves per Q tile; out is
// written in [B,L,H,D] memory. Backward: one block per (b, h, K tile), K_t
// and V_t staged once, looping over the Q tiles from the diagonal down;
// dK/dV accumulate in registers, dQ goes to an fp32 buffer by atomicAdd, the
// bias-table gradients to an LDS histogram flushed with one global atomicAdd
// per non-zero bucket. The strip steps are flash_strip.h's runtime forms in
// the order hstu_attn.hip calls them, so at L <= 64 the two files agree.
//
// q/k/v/dout are FlashViews ([B,H,L,D]-shaped, d innermost, any 16-byte
// aligned strides): the layer's chunk -> view -> transpose tensors are read
// in place.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../core/attn_host.h"
#include "../core/hstu_bias.h"

namespace genrec {

constexpr int HSTU_DIAG = 2 * TILE;     // 127 diagonals of a tile pair, padded
constexpr int HSTU_MAX_BUCKETS = 4096;  // n_pos + n_time the LDS tables hold

// The head's columns of the position and time tables as floats:
// tab[0..n_pos) position, tab[n_pos..n_pos+n_time) time.
__device__ __forceinline__ void hstu_stage_tables(
    float* tab, const __hip_bfloat16* __restrict__ pos_table,
    const __hip_bfloat16* __restrict__ time_table, int h, int H, int n_pos,
    int n_time, int tid) {
  for (int i = tid; i < n_pos + n_time; i += 256) {
    tab[i] = i < n_pos ? to_f32(pos_table[(int64_t)i * H + h])
                       : to_f32(time_table[(int64_t)(i - n_pos) * H + h]);
  }
}

// Position buckets of the tile pair (q0, kt0): diag[x] is the bucket of
// j - i = kt0 - q0 + x - (TILE - 1), clamped into the table; 0 for a
// distance no (i, j) inside [0,L) has.
__device__ __forceinline__ void hstu_stage_diag(
    int* diag, const int* __restrict__ rel_bucket, int q0, int kt0, int L,
    int n_pos, int tid) {
  if (tid < HSTU_DIAG) {
    const int idx = kt0 - q0 + tid - (TILE - 1) + L - 1;
    int bkt = 0;
    if (tid < 2 * TILE - 1 && idx >= 0 && idx < 2 * L - 1) {
      bkt = min(max(rel_bucket[idx], 0), n_pos - 1);
    }
    diag[tid] = bkt;
  }
}

// Timestamps of rows r0, r0 + step, .. (four of them) of one batch item; 0
// without a time table or beyond L.
__device__ __forceinline__ void hstu_load_ts(const long long* __restrict__ ts,
                                             int r0, int step, int L,
                                             long long (&t)[4]) {
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int i = r0 + n * step;
    t[n] = (ts && i < L) ? ts[i] : 0;
  }
}

// The score of one visible (i, j): dot + position bias + time bias, in the
// order hstu_attn.hip adds them; forward and backward both call this. x is
// the pair's diagonal within the tile pair. pb / tb return the buckets.
__device__ __forceinline__ float hstu_score(float dot, int x, long long ti,
                                            long long tj, const int* diag,
                                            const float* tab, int n_pos,
                                            int n_time, int& pb, int& tb) {
  pb = diag[x];
  float s = dot + tab[pb];
  tb = 0;
  if (n_time) {
    tb = time_bucket(ti, tj, n_time);
    s += tab[n_pos + tb];
  }
  return s;
}

__global__ void __launch_bounds__(256)
hstu_flash_fwd_kernel(
    FlashView q, FlashView k, FlashView v,          // [B,H,L,D] views
    const int* __restrict__ rel_bucket,             // [2L-1]
    const __hip_bfloat16* __restrict__ pos_table,   // [n_pos, H]
    const __hip_bfloat16* __restrict__ time_table,  // null | [n_time, H]
    const long long* __restrict__ ts,               // null | [B,L]
    const bool* __restrict__ key_pad,               // null | [B,L]
    __hip_bfloat16* __restrict__ out,               // [B,L,H,D]
    int H, int L, int D, int n_pos, int n_time) {
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int q0 = blockIdx.y * TILE;
  const __hip_bfloat16* qr = q.rows(b, h);
  const __hip_bfloat16* kr = k.rows(b, h);
  const __hip_bfloat16* vr = v.rows(b, h);
  const long long* ts_row = ts ? ts + (int64_t)b * L : nullptr;
  const bool* pad_row = key_pad ? key_pad + (int64_t)b * L : nullptr;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qs = smem;                 // [64][128B] Q rows
  char* ks = qs + TILE * 128;      // [64][128B] K rows (per tile)
  char* vt = ks + TILE * 128;      // [64(d)][128B(j)] V^T (per tile)
  char* ps = vt + TILE * 128;      // [64][128B] P (per tile)
  float* tab = reinterpret_cast<float*>(ps + TILE * 128);  // [n_pos+n_time]
  int* diag = reinterpret_cast<int*>(tab + n_pos + n_time);  // [HSTU_DIAG]

  const int tid = threadIdx.x;
  const Strip w(tid);

  for (int idx = tid; idx < TILE_CHUNKS; idx += blockDim.x) {
    const TileChunk c = tile_chunk(idx);
    const int qi = q0 + c.row;
    tile_store(qs, c.row, c.d0,
               load8(qr, qi * q.l + c.d0, qi < L && c.d0 < D));
  }
  hstu_stage_tables(tab, pos_table, time_table, h, H, n_pos, n_time, tid);

  long long tsi[4];
  hstu_load_ts(ts_row, q0 + w.row, 1, L, tsi);
  const CausalMask visible(q0, L, L, true, w);
  const int kt_end = visible.kt_end(q0, L);
  const int nfrag_d = (D + 15) / 16;
  float4v accO[4] = {};

  for (int kt0 = 0; kt0 < kt_end; kt0 += TILE) {
    __syncthreads();  // previous tile's ks / vt / diag fully consumed
    for (int idx = tid; idx < TILE_CHUNKS; idx += blockDim.x) {
      const TileChunk c = tile_chunk(idx);
      const int kj = kt0 + c.row;
      const bool ok = kj < L && c.d0 < D;
      tile_store(ks, c.row, c.d0, load8(kr, kj * k.l + c.d0, ok));
      tile_store_tr(vt, c.row, c.d0, w.lane, load8(vr, kj * v.l + c.d0, ok));
    }
    hstu_stage_diag(diag, rel_bucket, q0, kt0, L, n_pos, tid);
    __syncthreads();

    float4v acc[4] = {};
    strip_mma(acc, qs, ks, D, 4, w);

    const KeyCols kc = key_cols(kt0, L, pad_row, w);
    long long tsj[4];
    hstu_load_ts(ts_row, kt0 + w.col, 16, L, tsj);

#pragma unroll
    for (int f = 0; f < 4; ++f) {
      short4v p;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + w.row + r;
        float pv = 0.f;
        if (i < L && kc.j[f] < L) {
          float s = NEG_BIG;  // causal / pad: SiLU(-1e9) is -0
          if (visible(kc, f, r)) {
            int pb, tb;
            s = hstu_score(acc[f][r], f * 16 + w.col - (w.row + r) + TILE - 1,
                           tsi[r], tsj[f], diag, tab, n_pos, n_time, pb, tb);
          }
          pv = s * sigmoidf_dev(s);
        }
        p[r] = bf16_bits(pv);
      }
      strip_stash(ps, f, p, w);
    }
    __builtin_amdgcn_wave_barrier();

    strip_mma(accO, ps, vt, TILE, nfrag_d, w);
  }

  // out[b, i, h, :]: the [B,H,L,D] result in [B,L,H,D] memory
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int d = f * 16 + w.col;
    if (d >= D) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = q0 + w.row + r;
      if (i >= L) continue;
      out[(((int64_t)b * L + i) * H + h) * D + d] =
          __float2bfloat16(accO[f][r]);
    }
  }
}

__global__ void __launch_bounds__(256)
hstu_flash_bwd_kernel(
    FlashView dout, FlashView q, FlashView k, FlashView v,  // [B,H,L,D] views
    const int* __restrict__ rel_bucket,             // [2L-1]
    const __hip_bfloat16* __restrict__ pos_table,   // [n_pos, H]
    const __hip_bfloat16* __restrict__ time_table,  // null | [n_time, H]
    const long long* __restrict__ ts,               // null | [B,L]
    const bool* __restrict__ key_pad,               // null | [B,L]
    float* __restrict__ dq_f32,                     // [B,H,L,D] zero-init
    __hip_bfloat16* __restrict__ dk_out,            // [B,H,L,D]
    __hip_bfloat16* __restrict__ dv_out,
    float* __restrict__ dpos,                       // [n_pos, H] zero-init
    float* __restrict__ dtime,                      // null | [n_time, H]
    int H, int L, int D, int n_pos, int n_time) {
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int kt0 = blockIdx.y * TILE;
  const __hip_bfloat16* dor = dout.rows(b, h);
  const __hip_bfloat16* qr = q.rows(b, h);
  const __hip_bfloat16* kr = k.rows(b, h);
  const __hip_bfloat16* vr = v.rows(b, h);
  const long long* ts_row = ts ? ts + (int64_t)b * L : nullptr;
  const bool* pad_row = key_pad ? key_pad + (int64_t)b * L : nullptr;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ks = smem;                 // [64][128B] K_t rows (persistent)
  char* vs = ks + TILE * 128;      // [64][128B] V_t rows (persistent)
  char* kt = vs + TILE * 128;      // [64(d)][128B(j)] K_t^T (persistent)
  char* qs = kt + TILE * 128;      // [64][128B] Q rows (per Q tile)
  char* dos = qs + TILE * 128;     // [64][128B] dO rows (per Q tile)
  char* qt = dos + TILE * 128;     // [64(d)][128B(i)] Q^T (per Q tile)
  char* dot = qt + TILE * 128;     // [64(d)][128B(i)] dO^T (per Q tile)
  char* dsn = dot + TILE * 128;    // [64(i)][128B(j)] dS
  char* dst = dsn + TILE * 128;    // [64(j)][128B(i)] dS^T
  char* adt = dst + TILE * 128;    // [64(j)][128B(i)] A^T
  const int n_hist = n_pos + n_time;
  float* tab = reinterpret_cast<float*>(adt + TILE * 128);  // [n_hist]
  float* hist = tab + n_hist;                               // [n_hist]
  int* diag = reinterpret_cast<int*>(hist + n_hist);        // [HSTU_DIAG]

  const int tid = threadIdx.x;
  const Strip w(tid);

  for (int i = tid; i < n_hist; i += blockDim.x) hist[i] = 0.f;
  hstu_stage_tables(tab, pos_table, time_table, h, H, n_pos, n_time, tid);
  for (int idx = tid; idx < TILE_CHUNKS; idx += blockDim.x) {
    const TileChunk c = tile_chunk(idx);
    const int kj = kt0 + c.row;
    const bool ok = kj < L && c.d0 < D;
    short8v kk8 = load8(kr, kj * k.l + c.d0, ok);
    tile_store(ks, c.row, c.d0, kk8);
    tile_store_tr(kt, c.row, c.d0, w.lane, kk8);
    tile_store(vs, c.row, c.d0, load8(vr, kj * v.l + c.d0, ok));
  }

  const KeyCols kc = key_cols(kt0, L, pad_row, w);
  long long tsj[4];
  hstu_load_ts(ts_row, kt0 + w.col, 16, L, tsj);
  const int nfrag_d = (D + 15) / 16;
  float4v acck[4] = {};
  float4v accv[4] = {};

  // Q tiles above the diagonal tile see none of these keys
  for (int q0 = kt0; q0 < L; q0 += TILE) {
    __syncthreads();
    for (int idx = tid; idx < TILE_CHUNKS; idx += blockDim.x) {
      const TileChunk c = tile_chunk(idx);
      const int qi = q0 + c.row;
      const bool ok = qi < L && c.d0 < D;
      short8v dd8 = load8(dor, qi * dout.l + c.d0, ok);
      short8v qq8 = load8(qr, qi * q.l + c.d0, ok);
      tile_store(dos, c.row, c.d0, dd8);
      tile_store(qs, c.row, c.d0, qq8);
      tile_store_tr(dot, c.row, c.d0, w.lane, dd8);
      tile_store_tr(qt, c.row, c.d0, w.lane, qq8);
    }
    hstu_stage_diag(diag, rel_bucket, q0, kt0, L, n_pos, tid);
    __syncthreads();

    // S = Q K_t^T (as the forward) and dP = dO V_t^T
    float4v acc[4] = {};
    float4v accp[4] = {};
    strip_mma2(acc, qs, ks, accp, dos, vs, D, 4, w);

    long long tsi[4];
    hstu_load_ts(ts_row, q0 + w.row, 1, L, tsi);
    const CausalMask visible(q0, L, L, true, w);

#pragma unroll
    for (int f = 0; f < 4; ++f) {
      short4v ds, ad;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + w.row + r;
        float dsv = 0.f, adv = 0.f;
        if (i < L && kc.j[f] < L) {
          float s = NEG_BIG;
          int pb = 0, tb = 0;
          if (visible(kc, f, r)) {
            s = hstu_score(acc[f][r], f * 16 + w.col - (w.row + r) + TILE - 1,
                           tsi[r], tsj[f], diag, tab, n_pos, n_time, pb, tb);
          }
          float sg = sigmoidf_dev(s);
          dsv = accp[f][r] * sg * (1.f + s * (1.f - sg));
          adv = s * sg;  // A = SiLU(S)
          // masked scores have SiLU'(-1e9) == 0 and never get here
          if (dsv != 0.f) {
            atomicAdd(&hist[pb], dsv);
            if (n_time) atomicAdd(&hist[n_pos + tb], dsv);
          }
        }
        ds[r] = bf16_bits(dsv);
        ad[r] = bf16_bits(adv);
      }
      strip_stash(dsn, f, ds, w);
      strip_stash_tr(dst, f, ds, w);
      strip_stash_tr(adt, f, ad, w);
    }

    strip_bwd_products(
        dsn, kt, dst, qt, adt, dot, nfrag_d, acck, accv, w,
        [&](const float4v (&accq)[4]) {
#pragma unroll
          for (int f = 0; f < 4; ++f) {
            if (f >= nfrag_d) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = q0 + w.row + r;
              const int d = f * 16 + w.col;
              if (i < L && d < D) {
                atomicAdd(&dq_f32[idx4(b, h, i, d, H, L, D)], accq[f][r]);
              }
            }
          }
        });
  }

  strip_store(dk_out, bh, kt0, L, D, acck, w);
  strip_store(dv_out, bh, kt0, L, D, accv, w);

  // flush the bias histograms: one global atomicAdd per non-zero bucket
  __syncthreads();
  for (int i = tid; i < n_hist; i += blockDim.x) {
    const float val = hist[i];
    if (val != 0.f) {
      if (i < n_pos) atomicAdd(&dpos[(int64_t)i * H + h], val);
      else atomicAdd(&dtime[(int64_t)(i - n_pos) * H + h], val);
    }
  }
}

// ------------------------------------------------------------------ hosts

namespace {

struct HstuFlashArgs {
  int B, H, L, D, n_pos, n_time;
  torch::Tensor rel, pos, time, ts, pad;  // kept alive until the launch
  const __hip_bfloat16* time_ptr = nullptr;
  const long long* ts_ptr = nullptr;
  const bool* pad_ptr = nullptr;
};

HstuFlashArgs hstu_flash_check(
    const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v,
    const torch::Tensor& rel_bucket, const torch::Tensor& pos_table,
    const c10::optional<torch::Tensor>& time_table,
    const c10::optional<torch::Tensor>& timestamps,
    const c10::optional<torch::Tensor>& key_pad) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda(),
              "hstu_attn_flash: q/k/v must be GPU tensors");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
                  k.scalar_type() == torch::kBFloat16 &&
                  v.scalar_type() == torch::kBFloat16,
              "hstu_attn_flash: q/k/v must be bf16");
  TORCH_CHECK(q.dim() == 4 && k.sizes() == q.sizes() && v.sizes() == q.sizes(),
              "hstu_attn_flash: q/k/v must share one [B,H,L,D] shape");
  HstuFlashArgs a;
  a.B = q.size(0), a.H = q.size(1), a.L = q.size(2), a.D = q.size(3);
  TORCH_CHECK(a.B >= 1 && a.H >= 1 && a.L >= 1,
              "hstu_attn_flash: empty batch, head or sequence");
  TORCH_CHECK(a.D % 32 == 0 && a.D <= TILE,
              "hstu_attn_flash: head dim must be 32 or 64");
  TORCH_CHECK((int64_t)q.size(2) <= (int64_t)65535 * TILE,
              "hstu_attn_flash: sequence too long");
  TORCH_CHECK(rel_bucket.is_cuda() &&
                  rel_bucket.scalar_type() == torch::kInt32 &&
                  rel_bucket.numel() == 2 * (int64_t)a.L - 1,
              "hstu_attn_flash: rel_bucket must be an int32 [2L-1] GPU tensor");
  TORCH_CHECK(pos_table.is_cuda() &&
                  pos_table.scalar_type() == torch::kBFloat16 &&
                  pos_table.dim() == 2 && pos_table.size(1) == a.H &&
                  pos_table.size(0) >= 1,
              "hstu_attn_flash: pos_table must be a bf16 [n_pos,H] GPU tensor");
  a.rel = rel_bucket.contiguous();
  a.pos = pos_table.contiguous();
  a.n_pos = pos_table.size(0);
  a.n_time = 0;
  TORCH_CHECK(time_table.has_value() == timestamps.has_value(),
              "hstu_attn_flash: time_table and timestamps go together");
  if (time_table.has_value()) {
    TORCH_CHECK(time_table->is_cuda() &&
                    time_table->scalar_type() == torch::kBFloat16 &&
                    time_table->dim() == 2 && time_table->size(1) == a.H &&
                    time_table->size(0) >= 1,
                "hstu_attn_flash: time_table must be a bf16 [n_time,H] GPU "
                "tensor");
    TORCH_CHECK(timestamps->is_cuda() &&
                    at::isIntegralType(timestamps->scalar_type(), false) &&
                    timestamps->dim() == 2 && timestamps->size(0) == a.B &&
                    timestamps->size(1) == a.L,
                "hstu_attn_flash: timestamps must be an integer [B,L] GPU "
                "tensor");
    a.time = time_table->contiguous();
    a.ts = timestamps->to(torch::kInt64).contiguous();
    a.n_time = time_table->size(0);
    a.time_ptr = bf16_cptr(a.time);
    a.ts_ptr = reinterpret_cast<const long long*>(a.ts.data_ptr());
  }
  TORCH_CHECK(a.n_pos + a.n_time <= HSTU_MAX_BUCKETS,
              "hstu_attn_flash: more than ", HSTU_MAX_BUCKETS,
              " bias buckets");
  if (key_pad.has_value()) {
    TORCH_CHECK(key_pad->is_cuda() && key_pad->scalar_type() == torch::kBool &&
                    key_pad->dim() == 2 && key_pad->size(0) == a.B &&
                    key_pad->size(1) == a.L,
                "hstu_attn_flash: key_pad must be a bool [B,L] GPU tensor");
    a.pad_ptr = pad_ptr(key_pad, a.pad);
  }
  return a;
}

// LDS of the backward: ten tiles, the table and its histogram, the diagonals
size_t hstu_bwd_lds(int n_buckets) {
  return 10 * TILE * 128 + 2 * (size_t)n_buckets * sizeof(float) +
         HSTU_DIAG * sizeof(int);
}

// The backward is above 64 KiB of dynamic LDS: raise its limit, once per
// device, to what the largest table takes.
void hstu_allow_bwd_lds(int dev) {
  static bool done[64] = {};
  if (!done[dev % 64]) {
    C10_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(hstu_flash_bwd_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)hstu_bwd_lds(HSTU_MAX_BUCKETS)));
    done[dev % 64] = true;
  }
}

}  // namespace

// -> out as a [B,H,L,D] view of [B,L,H,D] memory
torch::Tensor hstu_attn_flash_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor rel_bucket, torch::Tensor pos_table,
    c10::optional<torch::Tensor> time_table,
    c10::optional<torch::Tensor> timestamps,
    c10::optional<torch::Tensor> key_pad) {
  HstuFlashArgs a = hstu_flash_check(q, k, v, rel_bucket, pos_table,
                                     time_table, timestamps, key_pad);
  torch::Tensor qn = kernel_readable(q, 3);
  torch::Tensor kn = kernel_readable(k, 3);
  torch::Tensor vn = kernel_readable(v, 3);
  auto out = torch::empty({a.B, a.L, a.H, a.D}, q.options());
  dim3 block(256);
  dim3 grid(a.B * a.H, (a.L + TILE - 1) / TILE);
  size_t smem = 4 * TILE * 128 + (size_t)(a.n_pos + a.n_time) * sizeof(float) +
                HSTU_DIAG * sizeof(int);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(hstu_flash_fwd_kernel, grid, block, smem, stream,
      view_bhld(qn), view_bhld(kn), view_bhld(vn), a.rel.data_ptr<int>(),
      bf16_cptr(a.pos), a.time_ptr, a.ts_ptr, a.pad_ptr, bf16_ptr(out),
      a.H, a.L, a.D, a.n_pos, a.n_time);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out.transpose(1, 2);
}

// -> dq, dk, dv [B,H,L,D] bf16; dpos [n_pos,H], dtime [n_time,H] | [0] fp32
std::vector<torch::Tensor> hstu_attn_flash_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor rel_bucket, torch::Tensor pos_table,
    c10::optional<torch::Tensor> time_table,
    c10::optional<torch::Tensor> timestamps,
    c10::optional<torch::Tensor> key_pad) {
  HstuFlashArgs a = hstu_flash_check(q, k, v, rel_bucket, pos_table,
                                     time_table, timestamps, key_pad);
  TORCH_CHECK(dout.is_cuda() && dout.scalar_type() == torch::kBFloat16 &&
                  dout.sizes() == q.sizes(),
              "hstu_attn_flash: dout must be bf16 and shaped as q");
  torch::Tensor don = kernel_readable(dout, 3);
  torch::Tensor qn = kernel_readable(q, 3);
  torch::Tensor kn = kernel_readable(k, 3);
  torch::Tensor vn = kernel_readable(v, 3);
  auto opts_f = q.options().dtype(torch::kFloat32);
  auto dq_f32 = torch::zeros({a.B, a.H, a.L, a.D}, opts_f);
  auto dk = torch::empty({a.B, a.H, a.L, a.D}, q.options());
  auto dv = torch::empty({a.B, a.H, a.L, a.D}, q.options());
  auto dpos = torch::zeros({a.n_pos, a.H}, opts_f);
  torch::Tensor dtime = a.n_time ? torch::zeros({a.n_time, a.H}, opts_f)
                                 : torch::empty({0}, opts_f);
  dim3 block(256);
  dim3 grid(a.B * a.H, (a.L + TILE - 1) / TILE);
  size_t smem = hstu_bwd_lds(a.n_pos + a.n_time);
  hstu_allow_bwd_lds(q.get_device());
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(hstu_flash_bwd_kernel, grid, block, smem, stream,
      view_bhld(don), view_bhld(qn), view_bhld(kn), view_bhld(vn),
      a.rel.data_ptr<int>(), bf16_cptr(a.pos), a.time_ptr, a.ts_ptr,
      a.pad_ptr, dq_f32.data_ptr<float>(), bf16_ptr(dk), bf16_ptr(dv),
      dpos.data_ptr<float>(), a.n_time ? dtime.data_ptr<float>() : nullptr,
      a.H, a.L, a.D, a.n_pos, a.n_time);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dq_f32.to(torch::kBFloat16), dk, dv, dpos, dtime};
}

}  // namespace genrec
