// Low-rank adapter (LoRA) kernels for a linear layer, gfx950, bf16 operands
// with fp32 accumulation on v_mfma_f32_16x16x32_bf16. With M rows, a wide
// dimension Kw, rank r in {16, 32, 64} (NR = r / 16 rank fragments), a
// scalar c and an optional dropout mask over the logical [M, Kw] matrix:
//
//   lora_down     T[M,r]  = bf16(c * (mask.X)[M,Kw] @ P[r,Kw]^T)
//   lora_up_add_  Y[M,Kw] = bf16(Y + c * mask.(T[M,r] @ Q[Kw,r]^T))  in place
//   lora_grad     G[r,Kw] = bf16(c * T[M,r]^T @ (mask.X)[M,Kw])
//   lora_dropout_mask     the mask itself as uint8 (tests only)
//
// The forward of an adapted linear is down (X = x, P = A, mask on) and
// up_add (Y = y, Q = B); the backward is down (X = dy, P = B^T), up_add
// (Y = dx, Q = A^T, mask on) and grad twice (dA: T = dt, X = x, mask on;
// dB^T: T = t, X = dy). Each kernel passes over its wide operand once; the
// rank side lives in MFMA fragments.
//
// Rounding points (the contract ops/eager.py emulates): T is stored as
// bf16; up_add adds the fp32 product to the upcast Y and rounds once; grad
// sums in fp32 and rounds once; the mask zeroes elements and c (which
// carries 1/keep) multiplies the fp32 product, so a dropped input is an
// exact zero and a kept one is not pre-rounded. An element whose update is
// zero keeps its bits.
//
// keep(row, col) = (hash_rng(seed, row * Kw + col) & 0xFFFFFF) >= p * 2^24,
// the keep test of fused_elementwise.hip on the 64-bit position in the
// logical matrix (independent of strides). The mask is never stored.
//
// Wide operands are read through a row stride that is a multiple of 8
// elements with unit column stride and Kw % 8 == 0, so every access is 16
// bytes per lane. Row offsets are 64-bit, every global access is guarded
// for any M >= 1, there are no atomics: lora_down folds its waves'
// partials through LDS in wave order and lora_grad sums its row chunks in
// index order in a second stage.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../core/mfma_tile.h"

namespace genrec {

namespace {

using bf16 = __hip_bfloat16;

constexpr int LORA_WAVES = 4;      // waves per block, all three kernels
constexpr int UP_COLS = 512;       // columns of Y per lora_up_add_ block
constexpr int GRAD_BLOCKS = 512;   // stage-1 blocks lora_grad aims for

// zero the dropped elements of the 8 bf16 at logical position idx0..idx0+7
template <bool MASK>
__device__ __forceinline__ short8v drop8(short8v v, unsigned int seed,
                                         unsigned int thresh,
                                         unsigned long long idx0) {
  if (MASK) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if ((hash_rng(seed, idx0 + e) & 0xFFFFFF) < thresh) v[e] = 0;
  }
  return v;
}

__device__ __forceinline__ float bits_f32(short b) {
  return __uint_as_float((unsigned int)(unsigned short)b << 16);
}

// ----------------------------------------------------------------- down
// One block per 16 rows. Wave w takes the 64-column pieces w, w + 4, ... of
// the wide dimension (a row's 128-byte line goes to one wave); lane l
// reads row l & 15, columns k0 + (l >> 4) * 8 straight into the A
// fragment, and row n * 16 + (l & 15) of P at the same columns into the B
// fragment of rank fragment n. The four partial tiles are added in wave
// order through LDS; wave n stores rank fragment n.
template <int NR, bool MASK>
__global__ __launch_bounds__(LORA_WAVES * 64) void lora_down_kernel(
    const bf16* __restrict__ X, int64_t ldx, const bf16* __restrict__ P,
    bf16* __restrict__ T, int64_t M, int Kw, float c, unsigned int seed,
    unsigned int thresh) {
  constexpr int R = NR * 16;
  __shared__ float4v part[LORA_WAVES][NR][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * 16;
  const int64_t row = row0 + (lane & 15);
  const bool row_ok = row < M;
  const int kq = (lane >> 4) * 8;

  float4v acc[NR];
#pragma unroll
  for (int n = 0; n < NR; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};

  for (int k0 = wave * 64; k0 < Kw; k0 += LORA_WAVES * 64) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int col = k0 + h * 32 + kq;
      const bool col_ok = col < Kw;
      short8v a = load8(X, row * ldx + col, row_ok && col_ok);
      a = drop8<MASK>(a, seed, thresh,
                      (unsigned long long)row * Kw + col);
#pragma unroll
      for (int n = 0; n < NR; ++n) {
        short8v b = load8(P, (int64_t)(n * 16 + (lane & 15)) * Kw + col,
                          col_ok);
        acc[n] = mfma_bf16(a, b, acc[n]);
      }
    }
  }

#pragma unroll
  for (int n = 0; n < NR; ++n) part[wave][n][lane] = acc[n];
  __syncthreads();
  if (wave < NR) {
    float4v s = part[0][wave][lane];
#pragma unroll
    for (int w = 1; w < LORA_WAVES; ++w) s += part[w][wave][lane];
    const int rank = wave * 16 + frag_col(lane);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t r = row0 + frag_row0(lane) + reg;
      if (r < M) T[r * R + rank] = __float2bfloat16(c * s[reg]);
    }
  }
}

// --------------------------------------------------------------- up_add
// The product is formed transposed, C = Q_tile @ T_rows^T, so that a lane
// ends up with 8 consecutive columns of one row of Y: fragment f (0, 1)
// feeds A row i with column n0 + (i >> 2) * 8 + f * 4 + (i & 3) of Q, and
// lane l then holds columns n0 + (l >> 4) * 8 + f * 4 + reg of row l & 15,
// the 16 bytes an A-fragment load would read. The rank is the k index;
// at r = 16 the upper half of the k range is fed zeros.
// Grid (16-row groups, UP_COLS-column groups); a wave takes 64-column
// pieces of its group.
template <int NR, bool MASK>
__global__ __launch_bounds__(LORA_WAVES * 64) void lora_up_add_kernel(
    bf16* __restrict__ Y, int64_t ldy, const bf16* __restrict__ T,
    const bf16* __restrict__ Q, int64_t M, int Kw, float c,
    unsigned int seed, unsigned int thresh) {
  constexpr int R = NR * 16;
  constexpr int KS = (R + 31) / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 16 + (lane & 15);
  const bool row_ok = row < M;
  const int kq = (lane >> 4) * 8;

  short8v tf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s)
    tf[s] = load8(T, row * R + s * 32 + kq, row_ok && s * 32 + kq < R);

  const int c_begin = blockIdx.y * UP_COLS;
  const int c_end = min(Kw, c_begin + UP_COLS);
  for (int c0 = c_begin + wave * 64; c0 < c_end; c0 += LORA_WAVES * 64) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int n0 = c0 + h * 32;
      float4v acc[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        acc[f] = float4v{0.f, 0.f, 0.f, 0.f};
        const int n = n0 + ((lane & 15) >> 2) * 8 + f * 4 + (lane & 3);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          short8v q = load8(Q, (int64_t)n * R + s * 32 + kq,
                            n < Kw && s * 32 + kq < R);
          acc[f] = mfma_bf16(q, tf[s], acc[f]);
        }
      }
      const int col = n0 + kq;
      if (row_ok && col < Kw) {
        short8va* yp = reinterpret_cast<short8va*>(Y + row * ldy + col);
        short8v y = *yp;
        const unsigned long long idx0 = (unsigned long long)row * Kw + col;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float d = c * acc[e >> 2][e & 3];
          if (MASK && (hash_rng(seed, idx0 + e) & 0xFFFFFF) < thresh) d = 0.f;
          if (d != 0.f) y[e] = bf16_bits(bits_f32(y[e]) + d);
        }
        *yp = y;
      }
    }
  }
}

// ----------------------------------------------------------------- grad
// Contracts over rows, so both operands are needed by columns: 64 x 64
// tiles of X (masked while staging, zero-padded) and 64 x r tiles of T go
// to LDS as dual-use images and are read with frag_load_tr (wave-uniform
// control flow: it needs EXEC all ones). Stage 1, grid (64-column strips,
// row chunks): wave w owns columns 16 w .. 16 w + 15 of the strip for all
// NR rank fragments and writes fp32 partials [chunks, r, Kw]. Stage 2 sums
// the chunks in index order, scales and rounds.
template <int NR, bool MASK>
__global__ __launch_bounds__(LORA_WAVES * 64) void lora_grad_kernel(
    const bf16* __restrict__ T, const bf16* __restrict__ X, int64_t ldx,
    float* __restrict__ part, int64_t M, int Kw, int64_t chunk_rows,
    unsigned int seed, unsigned int thresh) {
  constexpr int R = NR * 16;
  __shared__ __attribute__((aligned(16))) char tiles[2 * TILE * 128];
  char* xt = tiles;
  char* tt = tiles + TILE * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * 64;
  const int64_t r_begin = (int64_t)blockIdx.y * chunk_rows;
  const int64_t r_end =
      r_begin + chunk_rows < M ? r_begin + chunk_rows : M;

  float4v acc[NR];
#pragma unroll
  for (int n = 0; n < NR; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};

  for (int64_t r0 = r_begin; r0 < r_end; r0 += TILE) {
    for (int idx = tid; idx < TILE_CHUNKS; idx += LORA_WAVES * 64) {
      const TileChunk ch = tile_chunk(idx);
      const int64_t gr = r0 + ch.row;
      const bool live = gr < r_end;
      const int col = c0 + ch.d0;
      short8v xv = load8(X, gr * ldx + col, live && col < Kw);
      xv = drop8<MASK>(xv, seed, thresh, (unsigned long long)gr * Kw + col);
      tile_store<true>(xt, ch.row, ch.d0, xv);
      if (ch.d0 < R)
        tile_store<true>(tt, ch.row, ch.d0, load8(T, gr * R + ch.d0, live));
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < TILE / 32; ++ks) {
      const short8v b = frag_load_tr(xt, ks * 32, wave * 16, lane);
#pragma unroll
      for (int n = 0; n < NR; ++n)
        acc[n] = mfma_bf16(frag_load_tr(tt, ks * 32, n * 16, lane), b,
                           acc[n]);
    }
    __syncthreads();
  }

  const int col = c0 + wave * 16 + frag_col(lane);
  if (col < Kw) {
#pragma unroll
    for (int n = 0; n < NR; ++n)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int rank = n * 16 + frag_row0(lane) + reg;
        part[((int64_t)blockIdx.y * R + rank) * Kw + col] = acc[n][reg];
      }
  }
}

// G[i] = bf16(c * sum over chunks, in index order, of part[chunk][i])
__global__ void lora_grad_reduce_kernel(const float* __restrict__ part,
                                        bf16* __restrict__ G, int chunks,
                                        int64_t n, float c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = part[i];
  for (int k = 1; k < chunks; ++k) s += part[(int64_t)k * n + i];
  G[i] = __float2bfloat16(c * s);
}

__global__ void lora_mask_kernel(unsigned char* __restrict__ mask, int64_t n,
                                 unsigned int seed, unsigned int thresh) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    mask[i] = (hash_rng(seed, (unsigned long long)i) & 0xFFFFFF) >= thresh;
}

// ----------------------------------------------------------------- host

inline const bf16* cbf(const torch::Tensor& t) {
  return reinterpret_cast<const bf16*>(t.data_ptr());
}
inline bf16* bfp(torch::Tensor& t) {
  return reinterpret_cast<bf16*>(t.data_ptr());
}
inline bool aligned16(const torch::Tensor& t) {
  return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
}

// a wide operand [M, Kw]: bf16 on the GPU, unit column stride, a row stride
// that is a multiple of 8 and at least Kw, 16-byte aligned -> its row stride
int64_t wide_stride(const torch::Tensor& t, const char* op, const char* name) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be on the GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, op, ": ", name,
              " must be bf16");
  TORCH_CHECK(t.dim() == 2, op, ": ", name, " must be 2-D");
  const int64_t M = t.size(0), Kw = t.size(1);
  TORCH_CHECK(Kw > 0 && Kw % 8 == 0 && Kw < (1LL << 31), op, ": ", name,
              " width must be a positive multiple of 8, got ", Kw);
  TORCH_CHECK(M < (1LL << 31) * 16, op, ": too many rows");
  if (M == 0) return Kw;
  TORCH_CHECK(t.stride(1) == 1, op, ": ", name,
              " must have a contiguous last dimension");
  TORCH_CHECK(M == 1 || (t.stride(0) % 8 == 0 && t.stride(0) >= Kw), op, ": ",
              name, " row stride must be a multiple of 8 and >= its width");
  TORCH_CHECK(aligned16(t), op, ": ", name, " must be 16-byte aligned");
  return M == 1 ? Kw : t.stride(0);
}

// a rank-side matrix: bf16, contiguous, on `like`'s device, 16-byte aligned
void check_small(const torch::Tensor& t, const torch::Tensor& like,
                 const char* op, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), op, ": ", name,
              " must be on the same GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, op, ": ", name,
              " must be bf16");
  TORCH_CHECK(t.dim() == 2 && t.is_contiguous(), op, ": ", name,
              " must be a contiguous 2-D tensor");
  TORCH_CHECK(aligned16(t), op, ": ", name, " must be 16-byte aligned");
}

void check_rank(int64_t r, const char* op) {
  TORCH_CHECK(r == 16 || r == 32 || r == 64, op,
              ": rank must be 16, 32 or 64, got ", r);
}

// p in [0, 1) -> the keep threshold of fused_elementwise.hip (0 = no mask)
unsigned int drop_thresh(double p, const char* op) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, op, ": dropout p must be in [0, 1)");
  return (unsigned int)((float)p * 16777216.0f);
}

// KERNEL<NR, MASK> for the rank and the mask switch
#define LORA_LAUNCH(KERNEL, r, masked, grid, ...)                            \
  do {                                                                       \
    auto stream_ = at::cuda::getCurrentHIPStream();                          \
    const dim3 block_(LORA_WAVES * 64);                                      \
    if ((r) == 16 && (masked))                                               \
      hipLaunchKernelGGL((KERNEL<1, true>), grid, block_, 0, stream_,        \
                         __VA_ARGS__);                                       \
    else if ((r) == 16)                                                      \
      hipLaunchKernelGGL((KERNEL<1, false>), grid, block_, 0, stream_,       \
                         __VA_ARGS__);                                       \
    else if ((r) == 32 && (masked))                                          \
      hipLaunchKernelGGL((KERNEL<2, true>), grid, block_, 0, stream_,        \
                         __VA_ARGS__);                                       \
    else if ((r) == 32)                                                      \
      hipLaunchKernelGGL((KERNEL<2, false>), grid, block_, 0, stream_,       \
                         __VA_ARGS__);                                       \
    else if (masked)                                                         \
      hipLaunchKernelGGL((KERNEL<4, true>), grid, block_, 0, stream_,        \
                         __VA_ARGS__);                                       \
    else                                                                     \
      hipLaunchKernelGGL((KERNEL<4, false>), grid, block_, 0, stream_,       \
                         __VA_ARGS__);                                       \
  } while (0)

}  // namespace

// T[M,r] = bf16(c * (mask.x)[M,Kw] @ p_mat[r,Kw]^T)
torch::Tensor lora_down(torch::Tensor x, torch::Tensor p_mat, double c,
                        double drop_p, int64_t seed) {
  const int64_t ldx = wide_stride(x, "lora_down", "x");
  check_small(p_mat, x, "lora_down", "p_mat");
  const int64_t M = x.size(0), Kw = x.size(1), r = p_mat.size(0);
  check_rank(r, "lora_down");
  TORCH_CHECK(p_mat.size(1) == Kw, "lora_down: p_mat must be [r, ", Kw, "]");
  const unsigned int thresh = drop_thresh(drop_p, "lora_down");
  auto t = torch::empty({M, r}, x.options());
  if (M == 0) return t;
  const dim3 grid((unsigned int)((M + 15) / 16));
  LORA_LAUNCH(lora_down_kernel, r, thresh > 0, grid, cbf(x), ldx, cbf(p_mat),
              bfp(t), M, (int)Kw, (float)c, (unsigned int)seed, thresh);
  return t;
}

// y[M,Kw] = bf16(y + c * mask.(t[M,r] @ q[Kw,r]^T)), in place
torch::Tensor lora_up_add_(torch::Tensor y, torch::Tensor t, torch::Tensor q,
                           double c, double drop_p, int64_t seed) {
  const int64_t ldy = wide_stride(y, "lora_up_add_", "y");
  check_small(t, y, "lora_up_add_", "t");
  check_small(q, y, "lora_up_add_", "q");
  const int64_t M = y.size(0), Kw = y.size(1), r = t.size(1);
  check_rank(r, "lora_up_add_");
  TORCH_CHECK(t.size(0) == M, "lora_up_add_: t must be [", M, ", r]");
  TORCH_CHECK(q.size(0) == Kw && q.size(1) == r, "lora_up_add_: q must be [",
              Kw, ", ", r, "]");
  const unsigned int thresh = drop_thresh(drop_p, "lora_up_add_");
  if (M == 0) return y;
  const dim3 grid((unsigned int)((M + 15) / 16),
                  (unsigned int)((Kw + UP_COLS - 1) / UP_COLS));
  LORA_LAUNCH(lora_up_add_kernel, r, thresh > 0, grid, bfp(y), ldy, cbf(t),
              cbf(q), M, (int)Kw, (float)c, (unsigned int)seed, thresh);
  return y;
}

// G[r,Kw] = bf16(c * t[M,r]^T @ (mask.x)[M,Kw])
torch::Tensor lora_grad(torch::Tensor t, torch::Tensor x, double c,
                        double drop_p, int64_t seed) {
  const int64_t ldx = wide_stride(x, "lora_grad", "x");
  check_small(t, x, "lora_grad", "t");
  const int64_t M = x.size(0), Kw = x.size(1), r = t.size(1);
  check_rank(r, "lora_grad");
  TORCH_CHECK(t.size(0) == M, "lora_grad: t must be [", M, ", r]");
  const unsigned int thresh = drop_thresh(drop_p, "lora_grad");
  if (M == 0) return torch::zeros({r, Kw}, x.options());
  // row chunks: about GRAD_BLOCKS blocks over all strips, whole 64-row tiles
  const int64_t strips = (Kw + 63) / 64, tiles = (M + TILE - 1) / TILE;
  int64_t chunks = std::min<int64_t>(
      tiles, std::max<int64_t>(1, (GRAD_BLOCKS + strips - 1) / strips));
  const int64_t chunk_rows = (tiles + chunks - 1) / chunks * TILE;
  chunks = (M + chunk_rows - 1) / chunk_rows;
  auto part = torch::empty({chunks, r, Kw},
                           x.options().dtype(torch::kFloat32));
  auto g = torch::empty({r, Kw}, x.options());
  const dim3 grid((unsigned int)strips, (unsigned int)chunks);
  LORA_LAUNCH(lora_grad_kernel, r, thresh > 0, grid, cbf(t), cbf(x), ldx,
              part.data_ptr<float>(), M, (int)Kw, chunk_rows,
              (unsigned int)seed, thresh);
  const int64_t n = r * Kw;
  hipLaunchKernelGGL(lora_grad_reduce_kernel,
                     dim3((unsigned int)((n + 255) / 256)), dim3(256), 0,
                     at::cuda::getCurrentHIPStream(), part.data_ptr<float>(),
                     bfp(g), (int)chunks, n, (float)c);
  return g;
}

// the keep mask (1 = kept) of an [M, Kw] matrix as uint8, on the current GPU
torch::Tensor lora_dropout_mask(int64_t M, int64_t Kw, double p,
                                int64_t seed) {
  TORCH_CHECK(M >= 0 && Kw >= 0, "lora_dropout_mask: negative shape");
  const unsigned int thresh = drop_thresh(p, "lora_dropout_mask");
  auto mask = torch::empty(
      {M, Kw}, torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA));
  const int64_t n = M * Kw;
  if (n == 0) return mask;
  const unsigned int blocks =
      (unsigned int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(lora_mask_kernel, dim3(blocks), dim3(256), 0,
                     at::cuda::getCurrentHIPStream(),
                     mask.data_ptr<unsigned char>(), n, (unsigned int)seed,
                     thresh);
  return mask;
}

}  // namespace genrec
