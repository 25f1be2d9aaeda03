// In-place cross-entropy over one chunk of LM-head logits (gfx950).
//
// The linear-cross-entropy op (genrec_amd/ops/losses.py) forms the logits
// of a few hundred rows at a time with a hipBLASLt GEMM and hands the chunk
// logits[R, V] (bf16 or fp32, row stride >= V) to the two kernels below.
// V is the LLM vocabulary (~150k) and R is small, so unlike ce.hip (one wave
// per row) every row is cut into S column slices and the grid is (R, S):
//
//   lce_stats  one 256-thread workgroup per (row, slice): online
//              (max, sum-exp) in fp32 over 16-byte loads, wave reduce, then
//              a fixed-order LDS reduce across the 4 waves -> partial[R,S,2]
//   lce_grad   every workgroup folds the row's S partials in index order
//              into lse and overwrites its slice with
//              inv_n * (exp(x - lse) - onehot), zeros for an ignored row.
//
// row_loss = lse - logit[target] is written by the one thread that owns the
// target column, before it overwrites that column: another workgroup reading
// the target logit would race with the in-place store. No atomics anywhere;
// the caller reduces row_loss with one fixed-order sum, so loss and
// gradients are bitwise reproducible. Targets outside [0, V) other than
// ignore_index are treated as ignored (no out-of-range access).
//
// Slices start at multiples of 8 elements. Vector access needs a 16-byte
// aligned base and a row stride that keeps every row aligned; otherwise the
// whole slice takes the scalar loop (same results, slower).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../core/common.h"

namespace genrec {

namespace {

constexpr int LCE_THREADS = 256;
constexpr int LCE_WAVES = LCE_THREADS / WAVE;

template <typename T> struct LceVec;
template <> struct LceVec<float> {
  static constexpr int N = 4;
  __device__ static void load(const float* p, float (&x)[4]) {
    float4 v = *reinterpret_cast<const float4*>(p);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  }
  __device__ static void store(float* p, const float (&x)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  }
  // fp32 logits are compared at fp32 tolerances: full-precision exp
  __device__ static float exp(float x) { return expf(x); }
};
template <> struct LceVec<__hip_bfloat16> {
  static constexpr int N = 8;
  __device__ static void load(const __hip_bfloat16* p, float (&x)[8]) {
    uint4 v = *reinterpret_cast<const uint4*>(p);
    const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[2 * i] = __uint_as_float(w[i] << 16);
      x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  __device__ static void store(__hip_bfloat16* p, const float (&x)[8]) {
    unsigned int w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned int lo = __bfloat16_as_ushort(__float2bfloat16(x[2 * i]));
      unsigned int hi = __bfloat16_as_ushort(__float2bfloat16(x[2 * i + 1]));
      w[i] = lo | (hi << 16);
    }
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  // the result is rounded to bf16 (2^-8): the fast exp is far below that
  __device__ static float exp(float x) { return __expf(x); }
};

// (m, s) <- merge((m, s), (m2, s2)) of two online-softmax states; an empty
// state is (-inf, 0) and must not produce inf - inf.
__device__ __forceinline__ void lce_merge(float& m, float& s, float m2,
                                          float s2) {
  const float mn = fmaxf(m, m2);
  const float a = (m == mn) ? 1.f : expf(m - mn);
  const float b = (m2 == mn) ? 1.f : expf(m2 - mn);
  s = s * a + s2 * b;
  m = mn;
}

struct LceSlice {
  int64_t begin, end;   // columns [begin, end) of this workgroup
};

__device__ __forceinline__ LceSlice lce_slice(int64_t V, int64_t slice_len) {
  LceSlice r;
  r.begin = (int64_t)blockIdx.y * slice_len;
  r.end = r.begin + slice_len;
  if (r.begin > V) r.begin = V;
  if (r.end > V) r.end = V;
  return r;
}

template <typename T>
__global__ void __launch_bounds__(LCE_THREADS)
lce_stats_kernel(const T* __restrict__ logits, int64_t stride, int64_t V,
                 int64_t slice_len, int vec_ok, float* __restrict__ partial) {
  constexpr int N = LceVec<T>::N;
  const int64_t row = blockIdx.x;
  const T* lr = logits + row * stride;
  const LceSlice sl = lce_slice(V, slice_len);
  const int64_t n_vec = vec_ok ? (sl.end - sl.begin) / N : 0;

  float m = -INFINITY, s = 0.f;
  for (int64_t i = threadIdx.x; i < n_vec; i += LCE_THREADS) {
    float x[N];
    LceVec<T>::load(lr + sl.begin + i * N, x);
    float vm = x[0];
#pragma unroll
    for (int k = 1; k < N; ++k) vm = fmaxf(vm, x[k]);
    const float mn = fmaxf(m, vm);
    if (mn > -INFINITY) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < N; ++k) acc += LceVec<T>::exp(x[k] - mn);
      s = s * LceVec<T>::exp(m - mn) + acc;
      m = mn;
    }
  }
  for (int64_t j = sl.begin + n_vec * N + threadIdx.x; j < sl.end;
       j += LCE_THREADS)
    lce_merge(m, s, to_f32(lr[j]), 1.f);

  // wave: common max, rescale, sum
  const float wm = wave_max(m);
  s = (m == wm) ? s : s * expf(m - wm);   // m == wm also covers -inf == -inf
  s = wave_sum(s);

  __shared__ float sh[LCE_WAVES][2];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  if (lane == 0) { sh[wave][0] = wm; sh[wave][1] = s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float bm = sh[0][0], bs = sh[0][1];
#pragma unroll
    for (int w = 1; w < LCE_WAVES; ++w) lce_merge(bm, bs, sh[w][0], sh[w][1]);
    float* p = partial + (row * gridDim.y + blockIdx.y) * 2;
    p[0] = bm;
    p[1] = bs;
  }
}

template <typename T>
__global__ void __launch_bounds__(LCE_THREADS)
lce_grad_kernel(T* __restrict__ logits, int64_t stride, int64_t V,
                int64_t slice_len, int vec_ok,
                const float* __restrict__ partial,
                const int64_t* __restrict__ targets,
                const float* __restrict__ inv_n, int64_t ignore_index,
                float* __restrict__ row_loss, float* __restrict__ lse_out) {
  constexpr int N = LceVec<T>::N;
  const int64_t row = blockIdx.x;
  T* lr = logits + row * stride;
  const LceSlice sl = lce_slice(V, slice_len);
  const int64_t n_vec = vec_ok ? (sl.end - sl.begin) / N : 0;

  // every thread folds the S partials in the same order: same lse everywhere
  const float* p = partial + row * gridDim.y * 2;
  float m = p[0], s = p[1];
  for (unsigned int k = 1; k < gridDim.y; ++k)
    lce_merge(m, s, p[2 * k], p[2 * k + 1]);
  const float lse = m + logf(s);

  const int64_t t = targets[row];
  const bool ok = t != ignore_index && t >= 0 && t < V;
  const float g = inv_n[0];
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    lse_out[row] = lse;
    if (!ok) row_loss[row] = 0.f;
  }

  for (int64_t i = threadIdx.x; i < n_vec; i += LCE_THREADS) {
    const int64_t j0 = sl.begin + i * N;
    float x[N];
    if (ok) {
      LceVec<T>::load(lr + j0, x);
      if (t >= j0 && t < j0 + N) row_loss[row] = lse - x[t - j0];
#pragma unroll
      for (int k = 0; k < N; ++k)
        x[k] = g * (LceVec<T>::exp(x[k] - lse) - (j0 + k == t ? 1.f : 0.f));
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) x[k] = 0.f;
    }
    LceVec<T>::store(lr + j0, x);
  }
  for (int64_t j = sl.begin + n_vec * N + threadIdx.x; j < sl.end;
       j += LCE_THREADS) {
    float d = 0.f;
    if (ok) {
      const float x = to_f32(lr[j]);
      if (j == t) row_loss[row] = lse - x;
      d = g * (LceVec<T>::exp(x - lse) - (j == t ? 1.f : 0.f));
    }
    lr[j] = from_f32<T>(d);
  }
}

template <typename T>
void lce_launch(torch::Tensor& logits, const torch::Tensor& targets,
                const torch::Tensor& inv_n, int64_t ignore_index,
                torch::Tensor& partial, torch::Tensor& row_loss,
                torch::Tensor& lse, int64_t S, int64_t slice_len) {
  const int64_t R = logits.size(0), V = logits.size(1);
  const int64_t stride = logits.stride(0);
  T* ptr = reinterpret_cast<T*>(logits.data_ptr());
  const int vec_ok =
      reinterpret_cast<uintptr_t>(ptr) % 16 == 0 &&
      (stride * (int64_t)sizeof(T)) % 16 == 0;
  dim3 grid((unsigned)R, (unsigned)S), block(LCE_THREADS);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL((lce_stats_kernel<T>), grid, block, 0, stream, ptr,
                     stride, V, slice_len, vec_ok, partial.data_ptr<float>());
  hipLaunchKernelGGL((lce_grad_kernel<T>), grid, block, 0, stream, ptr,
                     stride, V, slice_len, vec_ok, partial.data_ptr<float>(),
                     targets.data_ptr<int64_t>(), inv_n.data_ptr<float>(),
                     ignore_index, row_loss.data_ptr<float>(),
                     lse.data_ptr<float>());
}

}  // namespace

// Number of column slices per row: enough workgroups for ~4 per CU, but no
// slice shorter than one 16-byte access per thread.
int64_t lce_pick_slices(int64_t R, int64_t V) {
  const int64_t cus =
      at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int64_t want = (4 * cus + R - 1) / std::max<int64_t>(R, 1);
  const int64_t cap = std::max<int64_t>(V / (8 * LCE_THREADS), 1);
  return std::max<int64_t>(1, std::min<int64_t>({want, cap, 65535}));
}

// logits[R, V] (row stride >= V, unit column stride) is overwritten with
// dlogits. Returns {row_loss[R], lse[R]} in fp32. slices <= 0: pick.
std::vector<torch::Tensor> lce_inplace(torch::Tensor logits,
                                       torch::Tensor targets,
                                       torch::Tensor inv_n,
                                       int64_t ignore_index, int64_t slices) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "lce: logits [R, V]");
  const int64_t R = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && logits.stride(1) == 1 &&
              (R <= 1 || logits.stride(0) >= V),
              "lce: logits need unit column stride and row stride >= V");
  TORCH_CHECK(targets.is_cuda() && targets.scalar_type() == torch::kInt64 &&
              targets.dim() == 1 && targets.size(0) == R &&
              targets.is_contiguous(), "lce: targets int64 [R]");
  TORCH_CHECK(inv_n.is_cuda() && inv_n.scalar_type() == torch::kFloat32 &&
              inv_n.numel() == 1, "lce: inv_n is a device fp32 scalar");
  TORCH_CHECK(R < (int64_t(1) << 31), "lce: too many rows in one chunk");
  auto f32 = logits.options().dtype(torch::kFloat32);
  auto row_loss = torch::empty({R}, f32);
  auto lse = torch::empty({R}, f32);
  if (R == 0) return {row_loss, lse};

  int64_t S = slices > 0 ? std::min<int64_t>(slices, 65535)
                         : lce_pick_slices(R, V);
  const int64_t slice_len = ((V + S - 1) / S + 7) / 8 * 8;
  auto partial = torch::empty({R, S, 2}, f32);
  if (logits.scalar_type() == torch::kFloat32) {
    lce_launch<float>(logits, targets, inv_n, ignore_index, partial,
                      row_loss, lse, S, slice_len);
  } else if (logits.scalar_type() == torch::kBFloat16) {
    lce_launch<__hip_bfloat16>(logits, targets, inv_n, ignore_index, partial,
                               row_loss, lse, S, slice_len);
  } else {
    TORCH_CHECK(false, "lce: unsupported dtype");
  }
  return {row_loss, lse};
}

}  // namespace genrec
