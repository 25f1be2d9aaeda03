// Fused elementwise/row kernels of a Qwen2 decoder layer (LCRec / NoteLLM
// backbone), gfx950, bf16 only:
//
//   add_rms_norm_{fwd,bwd}  wide-row RMSNorm (d <= 4096) with an optional
//                           residual add in front of it
//   rope_qk_fwd             rotary embedding of q and k in one launch, both
//                           directions (inverse = the gradient)
//   swiglu_{fwd,bwd}        silu(gate) * up
//
// All are memory-bound: every global access is 16 bytes per lane (8 bf16),
// row offsets are 64-bit, there are no atomics and nothing synchronises
// with the host. Loads that depend only on the index (norm weight, cos/sin)
// are issued before the data-dependent work. Rounding points follow the
// stock bf16 op sequences (see each kernel), so the results differ from
// the transformers composition only where a kernel keeps an intermediate
// in fp32 that stock rounds.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../core/common.h"

// The rounding points below are part of the contract (RoPE must equal the
// stock bf16 composition bit for bit). With contraction on, hipcc turns
// bf16(x*c) + bf16(y*s) into fma(x, c, bf16(y*s)) and drops the first
// rounding, so this file is compiled without fp contraction.
#pragma clang fp contract(off)

namespace genrec {

// norms.hip: column sum of [n_blocks, d] fp32 partials (fixed order, two
// stages: rms_dw_reduce1/2), cast to w's dtype
torch::Tensor rms_dw_finish(const torch::Tensor& dw, int n_blocks, int d,
                            const torch::Tensor& w, hipStream_t stream);

namespace {

// 8 bf16 = one 16-byte access
union BF16x8 {
  unsigned int u[4];
  __hip_bfloat16 e[8];
};

__device__ __forceinline__ BF16x8 load8(const __hip_bfloat16* p) {
  const uint4 t = *reinterpret_cast<const uint4*>(p);
  BF16x8 v;
  v.u[0] = t.x; v.u[1] = t.y; v.u[2] = t.z; v.u[3] = t.w;
  return v;
}

__device__ __forceinline__ void store8(__hip_bfloat16* p, const BF16x8& v) {
  *reinterpret_cast<uint4*>(p) = make_uint4(v.u[0], v.u[1], v.u[2], v.u[3]);
}

__device__ __forceinline__ BF16x8 zero8() {
  BF16x8 v;
  v.u[0] = v.u[1] = v.u[2] = v.u[3] = 0u;
  return v;
}

// fp32 value of x rounded to bf16
__device__ __forceinline__ float rbf(float x) {
  return to_f32(from_f32<__hip_bfloat16>(x));
}

inline bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

constexpr int NORM_WAVES = 4;        // waves (= rows in flight) per block
constexpr int NORM_MAX_D = 4096;     // 8 chunks of 8 columns per lane
constexpr int NORM_BWD_BLOCKS = 1024;

// ------------------------------------------------------- add + RMSNorm
// One wave per row, the row held in registers: lane owns the 8-column
// chunks lane, lane + 64, ... (NCH of them, d <= 512 * NCH).
//   h = bf16(x + res)                      (one rounding, = torch.add)
//   r = rsqrt(mean(h^2) + eps)             (fp32, from the rounded h)
//   n = bf16(w * bf16(h * r))              (Qwen2RMSNorm with a bf16 weight)

template <int NCH, bool HAS_RES>
__global__ void __launch_bounds__(64 * NORM_WAVES) add_rms_norm_fwd_kernel(
    const __hip_bfloat16* __restrict__ x, const __hip_bfloat16* __restrict__ res,
    const __hip_bfloat16* __restrict__ w, __hip_bfloat16* __restrict__ h,
    __hip_bfloat16* __restrict__ n, float* __restrict__ inv_rms,
    int64_t n_rows, int d, float eps) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave_id =
      (int64_t)blockIdx.x * NORM_WAVES + (int)(threadIdx.x / WAVE);
  const int64_t n_waves = (int64_t)gridDim.x * NORM_WAVES;
  const int d8 = d >> 3;

  BF16x8 wv[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = lane + c * WAVE;
    wv[c] = j < d8 ? load8(w + j * 8) : zero8();
  }

  for (int64_t row = wave_id; row < n_rows; row += n_waves) {
    const int64_t base = row * d;
    BF16x8 hv[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = lane + c * WAVE;
      hv[c] = j < d8 ? load8(x + base + j * 8) : zero8();
    }
    if (HAS_RES) {
      BF16x8 rv[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int j = lane + c * WAVE;
        rv[c] = j < d8 ? load8(res + base + j * 8) : zero8();
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int j = lane + c * WAVE;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          hv[c].e[k] = from_f32<__hip_bfloat16>(to_f32(hv[c].e[k]) +
                                                to_f32(rv[c].e[k]));
        if (j < d8) store8(h + base + j * 8, hv[c]);
      }
    }
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float v = to_f32(hv[c].e[k]);   // dead chunks hold zeros
        ss += v * v;
      }
    }
    ss = wave_sum(ss);
    const float r = rsqrtf(ss / d + eps);
    if (lane == 0) inv_rms[row] = r;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = lane + c * WAVE;
      if (j < d8) {
        BF16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          o.e[k] = from_f32<__hip_bfloat16>(to_f32(wv[c].e[k]) *
                                            rbf(to_f32(hv[c].e[k]) * r));
        store8(n + base + j * 8, o);
      }
    }
  }
}

// Backward, one pass:
//   g  = w*dn*r - r^3/d * h * sum_j(w_j*dn_j*h_j)     (fp32)
//   dx = bf16(dh + g)          (one rounding; stock rounds g first)
//   dw partial += dn * h * r   (fp32, per lane in registers)
// Block b / wave v always takes rows (4b + v) + k * 4 * gridDim.x in
// order, the four waves' partials are added in wave order through LDS,
// and one [d] partial row per block goes to global: bit-stable.

template <int NCH, bool HAS_DH>
__global__ void __launch_bounds__(64 * NORM_WAVES) add_rms_norm_bwd_kernel(
    const __hip_bfloat16* __restrict__ dn, const __hip_bfloat16* __restrict__ dh,
    const __hip_bfloat16* __restrict__ h, const __hip_bfloat16* __restrict__ w,
    const float* __restrict__ inv_rms, __hip_bfloat16* __restrict__ dx,
    float* __restrict__ dw, int64_t n_rows, int d) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int64_t wave_id = (int64_t)blockIdx.x * NORM_WAVES + wave;
  const int64_t n_waves = (int64_t)gridDim.x * NORM_WAVES;
  const int d8 = d >> 3;

  BF16x8 wv[NCH];
  float dw_acc[NCH][8];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = lane + c * WAVE;
    wv[c] = j < d8 ? load8(w + j * 8) : zero8();
#pragma unroll
    for (int k = 0; k < 8; ++k) dw_acc[c][k] = 0.f;
  }

  for (int64_t row = wave_id; row < n_rows; row += n_waves) {
    const int64_t base = row * d;
    BF16x8 hv[NCH], gv[NCH], av[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = lane + c * WAVE;
      hv[c] = j < d8 ? load8(h + base + j * 8) : zero8();
      gv[c] = j < d8 ? load8(dn + base + j * 8) : zero8();
      if (HAS_DH) av[c] = j < d8 ? load8(dh + base + j * 8) : zero8();
    }
    const float r = inv_rms[row];
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        dot += to_f32(wv[c].e[k]) * to_f32(gv[c].e[k]) * to_f32(hv[c].e[k]);
    }
    dot = wave_sum(dot);
    const float coef = r * r * r / d * dot;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = lane + c * WAVE;
      BF16x8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float hf = to_f32(hv[c].e[k]);
        const float gf = to_f32(gv[c].e[k]);
        float g = to_f32(wv[c].e[k]) * gf * r - coef * hf;
        if (HAS_DH) g += to_f32(av[c].e[k]);
        o.e[k] = from_f32<__hip_bfloat16>(g);
        dw_acc[c][k] += gf * hf * r;
      }
      if (j < d8) store8(dx + base + j * 8, o);
    }
  }

  // waves 1..3 park their partials in LDS [3][d]; wave 0 adds them to its
  // own in wave order and writes the block's row
  extern __shared__ __attribute__((aligned(16))) float dw_lds[];
  if (wave > 0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = lane + c * WAVE;
      if (j < d8) {
        float4* p = reinterpret_cast<float4*>(dw_lds + (wave - 1) * d + j * 8);
        p[0] = make_float4(dw_acc[c][0], dw_acc[c][1], dw_acc[c][2],
                           dw_acc[c][3]);
        p[1] = make_float4(dw_acc[c][4], dw_acc[c][5], dw_acc[c][6],
                           dw_acc[c][7]);
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    float* out = dw + (int64_t)blockIdx.x * d;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = lane + c * WAVE;
      if (j < d8) {
#pragma unroll
        for (int v = 0; v < NORM_WAVES - 1; ++v) {
          const float4* p =
              reinterpret_cast<const float4*>(dw_lds + v * d + j * 8);
          const float4 a = p[0], b = p[1];
          dw_acc[c][0] += a.x; dw_acc[c][1] += a.y;
          dw_acc[c][2] += a.z; dw_acc[c][3] += a.w;
          dw_acc[c][4] += b.x; dw_acc[c][5] += b.y;
          dw_acc[c][6] += b.z; dw_acc[c][7] += b.w;
        }
        float4* q = reinterpret_cast<float4*>(out + j * 8);
        q[0] = make_float4(dw_acc[c][0], dw_acc[c][1], dw_acc[c][2],
                           dw_acc[c][3]);
        q[1] = make_float4(dw_acc[c][4], dw_acc[c][5], dw_acc[c][6],
                           dw_acc[c][7]);
      }
    }
  }
}

// ---------------------------------------------------------------- RoPE
// A thread owns, for one (b, l), 8 columns of the first half and the 8
// partner columns D/2 away; it loads the four cos/sin chunks once and
// walks the Hq + Hkv heads. Every product is rounded to bf16 before the
// add, as the stock bf16 composition does (so nothing can contract to an
// fma):
//   forward   out[d] = bf16(bf16(x[d]*cos[d]) + bf16(xr[d]*sin[d])),
//             xr = (-x[d + D/2] | x[d - D/2])
//   inverse   dx[d]  = bf16(bf16(g[d]*cos[d]) + tr[d]),  t = bf16(g*sin),
//             tr = (t[d + D/2] | -t[d - D/2])
// Inputs are [B,H,L,D] views with element strides (d innermost); outputs
// are [B,L,H,D] contiguous.

template <bool INVERSE>
__global__ void __launch_bounds__(256) rope_qk_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ cosp,
    const __hip_bfloat16* __restrict__ sinp, __hip_bfloat16* __restrict__ qo,
    __hip_bfloat16* __restrict__ ko, int64_t n_items, int L, int D, int Hq,
    int Hkv, int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb,
    int64_t k_sh, int64_t k_sl, int64_t cs_sb) {
  const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= n_items) return;
  const int half = D >> 1;
  const int cpr = half >> 3;               // chunks per (b, l): 4 or 8
  const int c = (int)(item % cpr) * 8;     // first-half column
  const int64_t bl = item / cpr;
  const int l = (int)(bl % L);
  const int64_t b = bl / L;

  const int64_t cs = b * cs_sb + (int64_t)l * D + c;
  const BF16x8 c_lo = load8(cosp + cs), c_hi = load8(cosp + cs + half);
  const BF16x8 s_lo = load8(sinp + cs), s_hi = load8(sinp + cs + half);

  const int H = Hq + Hkv;
#pragma unroll 2
  for (int hh = 0; hh < H; ++hh) {
    const bool is_q = hh < Hq;
    const int hd = is_q ? hh : hh - Hq;
    const __hip_bfloat16* src =
        is_q ? q + b * q_sb + hd * q_sh + l * q_sl + c
             : k + b * k_sb + hd * k_sh + l * k_sl + c;
    __hip_bfloat16* dst =
        is_q ? qo + ((bl * Hq + hd) * (int64_t)D + c)
             : ko + ((bl * Hkv + hd) * (int64_t)D + c);
    const BF16x8 lo = load8(src), hi = load8(src + half);
    BF16x8 o_lo, o_hi;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xl = to_f32(lo.e[e]), xh = to_f32(hi.e[e]);
      const float a_lo = rbf(xl * to_f32(c_lo.e[e]));
      const float a_hi = rbf(xh * to_f32(c_hi.e[e]));
      float b_lo, b_hi;
      if (INVERSE) {
        b_lo = rbf(xh * to_f32(s_hi.e[e]));      //  t[d + D/2]
        b_hi = -rbf(xl * to_f32(s_lo.e[e]));     // -t[d - D/2]
      } else {
        b_lo = -rbf(xh * to_f32(s_lo.e[e]));     // -x[d + D/2] * sin[d]
        b_hi = rbf(xl * to_f32(s_hi.e[e]));      //  x[d - D/2] * sin[d]
      }
      o_lo.e[e] = from_f32<__hip_bfloat16>(a_lo + b_lo);
      o_hi.e[e] = from_f32<__hip_bfloat16>(a_hi + b_hi);
    }
    store8(dst, o_lo);
    store8(dst + half, o_hi);
  }
}

// -------------------------------------------------------------- SwiGLU
//   y     = bf16(bf16(silu(gate)) * up)
//   dup   = bf16(dy * bf16(silu(gate)))
//   dgate = bf16(dy * up * s * (1 + gate * (1 - s))),  s = sigmoid(gate)
// e = exp(-gate) may overflow to inf: gate / (1 + inf) = -0 and
// 1 / (1 + inf) = 0, never inf / inf.
// gate / up / dy are [rows, I] with a row stride; outputs are contiguous.

constexpr int SWIGLU_MAX_BLOCKS = 2048;

__global__ void __launch_bounds__(256) swiglu_fwd_kernel(
    const __hip_bfloat16* __restrict__ gate, const __hip_bfloat16* __restrict__ up,
    __hip_bfloat16* __restrict__ y, int64_t n_chunks, int i8, int64_t g_sr,
    int64_t u_sr) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < n_chunks; idx += step) {
    const int64_t row = idx / i8;
    const int col = (int)(idx - row * i8) * 8;
    const BF16x8 g = load8(gate + row * g_sr + col);
    const BF16x8 u = load8(up + row * u_sr + col);
    BF16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gf = to_f32(g.e[e]);
      const float act = rbf(gf / (1.0f + expf(-gf)));
      o.e[e] = from_f32<__hip_bfloat16>(act * to_f32(u.e[e]));
    }
    store8(y + idx * 8, o);
  }
}

__global__ void __launch_bounds__(256) swiglu_bwd_kernel(
    const __hip_bfloat16* __restrict__ dy, const __hip_bfloat16* __restrict__ gate,
    const __hip_bfloat16* __restrict__ up, __hip_bfloat16* __restrict__ dgate,
    __hip_bfloat16* __restrict__ dup, int64_t n_chunks, int i8, int64_t dy_sr,
    int64_t g_sr, int64_t u_sr) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < n_chunks; idx += step) {
    const int64_t row = idx / i8;
    const int col = (int)(idx - row * i8) * 8;
    const BF16x8 g = load8(gate + row * g_sr + col);
    const BF16x8 u = load8(up + row * u_sr + col);
    const BF16x8 t = load8(dy + row * dy_sr + col);
    BF16x8 og, ou;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gf = to_f32(g.e[e]);
      const float tf = to_f32(t.e[e]);
      const float den = 1.0f + expf(-gf);
      const float s = 1.0f / den;
      const float act = rbf(gf / den);
      ou.e[e] = from_f32<__hip_bfloat16>(tf * act);
      og.e[e] = from_f32<__hip_bfloat16>(tf * to_f32(u.e[e]) * s *
                                         (1.0f + gf * (1.0f - s)));
    }
    store8(dgate + idx * 8, og);
    store8(dup + idx * 8, ou);
  }
}

// ---------------------------------------------------------------- host

void check_rows_bf16(const torch::Tensor& t, int64_t n_rows, int d,
                     const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == torch::kBFloat16 && t.dim() >= 1 &&
              t.size(-1) == d && t.numel() == n_rows * d &&
              aligned16(t.data_ptr()),
              "add_rms_norm: ", what,
              " must be a contiguous, 16-byte aligned bf16 CUDA tensor of "
              "the input's shape");
}

inline const __hip_bfloat16* cbf(const torch::Tensor& t) {
  return reinterpret_cast<const __hip_bfloat16*>(t.data_ptr());
}
inline __hip_bfloat16* bf(torch::Tensor& t) {
  return reinterpret_cast<__hip_bfloat16*>(t.data_ptr());
}

int norm_dim(const torch::Tensor& x, const torch::Tensor& w) {
  TORCH_CHECK(x.dim() >= 1, "add_rms_norm: input needs a feature dim");
  const int64_t d = x.size(-1);
  TORCH_CHECK(d > 0 && d % 8 == 0 && d <= NORM_MAX_D,
              "add_rms_norm: d must be a multiple of 8 and <= ", NORM_MAX_D,
              ", got ", d);
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 &&
              w.dim() == 1 && w.numel() == d,
              "add_rms_norm: weight must be a bf16 CUDA vector of length d");
  return (int)d;
}

}  // namespace

#define GENREC_NCH_SWITCH(nch, LAUNCH)                                         \
  switch (nch) {                                                               \
    case 1: LAUNCH(1); break;                                                  \
    case 2: LAUNCH(2); break;                                                  \
    case 3: LAUNCH(3); break;                                                  \
    case 4: LAUNCH(4); break;                                                  \
    case 5: LAUNCH(5); break;                                                  \
    case 6: LAUNCH(6); break;                                                  \
    case 7: LAUNCH(7); break;                                                  \
    default: LAUNCH(8); break;                                                 \
  }

// -> (h, n, inv_rms); h is x itself when there is no residual
std::vector<torch::Tensor> add_rms_norm_fwd(
    torch::Tensor x, c10::optional<torch::Tensor> residual, torch::Tensor w,
    double eps) {
  const int d = norm_dim(x, w);
  const int64_t n_rows = x.numel() / d;
  check_rows_bf16(x, n_rows, d, "x");
  const bool has_res = residual.has_value();
  if (has_res) check_rows_bf16(*residual, n_rows, d, "residual");
  auto wc = w.contiguous();
  TORCH_CHECK(aligned16(wc.data_ptr()), "add_rms_norm: unaligned weight");
  auto h = has_res ? torch::empty_like(x) : x;
  auto n = torch::empty_like(x);
  auto inv_rms = torch::empty({n_rows}, x.options().dtype(torch::kFloat32));
  if (n_rows == 0) return {h, n, inv_rms};
  const int nch = (d / 8 + WAVE - 1) / WAVE;
  dim3 block(WAVE * NORM_WAVES);
  dim3 grid((unsigned)std::min<int64_t>(
      (n_rows + NORM_WAVES - 1) / NORM_WAVES, 8192));
  auto stream = at::cuda::getCurrentHIPStream();
#define LAUNCH_F(NCH)                                                          \
  do {                                                                         \
    if (has_res)                                                               \
      hipLaunchKernelGGL((add_rms_norm_fwd_kernel<NCH, true>), grid, block,    \
                         0, stream, cbf(x), cbf(*residual), cbf(wc), bf(h),    \
                         bf(n), inv_rms.data_ptr<float>(), n_rows, d,          \
                         (float)eps);                                          \
    else                                                                       \
      hipLaunchKernelGGL((add_rms_norm_fwd_kernel<NCH, false>), grid, block,   \
                         0, stream, cbf(x), nullptr, cbf(wc), nullptr, bf(n),  \
                         inv_rms.data_ptr<float>(), n_rows, d, (float)eps);    \
  } while (0)
  GENREC_NCH_SWITCH(nch, LAUNCH_F)
#undef LAUNCH_F
  return {h, n, inv_rms};
}

// -> (dx, dw) with dx = bf16(dh + norm input gradient)
std::vector<torch::Tensor> add_rms_norm_bwd(
    torch::Tensor dn, c10::optional<torch::Tensor> dh, torch::Tensor h,
    torch::Tensor w, torch::Tensor inv_rms) {
  const int d = norm_dim(h, w);
  const int64_t n_rows = h.numel() / d;
  check_rows_bf16(h, n_rows, d, "h");
  check_rows_bf16(dn, n_rows, d, "dn");
  const bool has_dh = dh.has_value();
  if (has_dh) check_rows_bf16(*dh, n_rows, d, "dh");
  TORCH_CHECK(inv_rms.is_cuda() && inv_rms.is_contiguous() &&
              inv_rms.scalar_type() == torch::kFloat32 &&
              inv_rms.numel() == n_rows,
              "add_rms_norm_bwd: inv_rms must be fp32 [rows]");
  auto wc = w.contiguous();
  TORCH_CHECK(aligned16(wc.data_ptr()), "add_rms_norm: unaligned weight");
  auto dx = torch::empty_like(h);
  if (n_rows == 0) return {dx, torch::zeros({(int64_t)d}, w.options())};
  const int nch = (d / 8 + WAVE - 1) / WAVE;
  const int n_blocks = (int)std::min<int64_t>(
      (n_rows + NORM_WAVES - 1) / NORM_WAVES, NORM_BWD_BLOCKS);
  auto dw = torch::empty({n_blocks, (int64_t)d},
                         h.options().dtype(torch::kFloat32));
  dim3 block(WAVE * NORM_WAVES);
  dim3 grid(n_blocks);
  const size_t smem = (size_t)(NORM_WAVES - 1) * d * sizeof(float);  // <= 48 KiB
  auto stream = at::cuda::getCurrentHIPStream();
#define LAUNCH_B(NCH)                                                          \
  do {                                                                         \
    if (has_dh)                                                                \
      hipLaunchKernelGGL((add_rms_norm_bwd_kernel<NCH, true>), grid, block,    \
                         smem, stream, cbf(dn), cbf(*dh), cbf(h), cbf(wc),     \
                         inv_rms.data_ptr<float>(), bf(dx),                    \
                         dw.data_ptr<float>(), n_rows, d);                     \
    else                                                                       \
      hipLaunchKernelGGL((add_rms_norm_bwd_kernel<NCH, false>), grid, block,   \
                         smem, stream, cbf(dn), nullptr, cbf(h), cbf(wc),      \
                         inv_rms.data_ptr<float>(), bf(dx),                    \
                         dw.data_ptr<float>(), n_rows, d);                     \
  } while (0)
  GENREC_NCH_SWITCH(nch, LAUNCH_B)
#undef LAUNCH_B
  return {dx, rms_dw_finish(dw, n_blocks, d, w, stream)};
}

#undef GENREC_NCH_SWITCH

namespace {

// element stride of a dim the kernel may index; a size-1 dim is never
// stepped over, whatever stride the view carries
int64_t rope_stride(const torch::Tensor& t, int dim, const char* what) {
  if (t.size(dim) == 1) return 0;
  const int64_t s = t.stride(dim);
  TORCH_CHECK(s >= 0 && s % 8 == 0, "rope_qk: ", what, " stride ", s,
              " of dim ", dim, " is not a multiple of 8");
  return s;
}

torch::Tensor rope_table(const torch::Tensor& t, int64_t B, int64_t L,
                         int64_t D, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
              t.dim() == 3 && (t.size(0) == 1 || t.size(0) == B) &&
              t.size(1) == L && t.size(2) == D,
              "rope_qk: ", what, " must be bf16 [B|1, L, D]");
  auto c = t.contiguous();
  TORCH_CHECK(aligned16(c.data_ptr()), "rope_qk: unaligned ", what);
  return c;
}

}  // namespace

// q [B,Hq,L,D], k [B,Hkv,L,D] (views, d innermost) -> (q_out, k_out) as
// [B,H,L,D] transpose views of contiguous [B,L,H,D] memory
std::vector<torch::Tensor> rope_qk_fwd(torch::Tensor q, torch::Tensor k,
                                       torch::Tensor cos, torch::Tensor sin,
                                       bool inverse) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() &&
              q.scalar_type() == torch::kBFloat16 &&
              k.scalar_type() == torch::kBFloat16,
              "rope_qk: q and k must be bf16 CUDA tensors");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && q.size(0) == k.size(0) &&
              q.size(2) == k.size(2) && q.size(3) == k.size(3),
              "rope_qk: expected q [B,Hq,L,D] and k [B,Hkv,L,D]");
  const int64_t B = q.size(0), Hq = q.size(1), L = q.size(2), D = q.size(3);
  const int64_t Hkv = k.size(1);
  TORCH_CHECK(D == 64 || D == 128, "rope_qk: head dim must be 64 or 128, got ",
              D);
  TORCH_CHECK(Hq >= 1 && Hkv >= 1 && L < (1LL << 31) && Hq + Hkv < (1 << 20),
              "rope_qk: bad head count or length");
  TORCH_CHECK(q.stride(3) == 1 && k.stride(3) == 1,
              "rope_qk: head dim must be innermost (stride 1)");
  TORCH_CHECK(aligned16(q.data_ptr()) && aligned16(k.data_ptr()),
              "rope_qk: unaligned q or k");
  const int64_t q_sb = rope_stride(q, 0, "q"), q_sh = rope_stride(q, 1, "q"),
                q_sl = rope_stride(q, 2, "q");
  const int64_t k_sb = rope_stride(k, 0, "k"), k_sh = rope_stride(k, 1, "k"),
                k_sl = rope_stride(k, 2, "k");
  auto cc = rope_table(cos, B, L, D, "cos");
  auto sc = rope_table(sin, B, L, D, "sin");
  TORCH_CHECK(cc.size(0) == sc.size(0), "rope_qk: cos/sin batch mismatch");
  const int64_t cs_sb = cc.size(0) == 1 ? 0 : L * D;
  auto qo = torch::empty({B, L, Hq, D}, q.options());
  auto ko = torch::empty({B, L, Hkv, D}, k.options());
  const int64_t n_items = B * L * (D / 16);
  if (n_items > 0) {
    dim3 block(256);
    TORCH_CHECK((n_items + 255) / 256 < (1LL << 31), "rope_qk: too large");
    dim3 grid((unsigned)((n_items + 255) / 256));
    auto stream = at::cuda::getCurrentHIPStream();
#define LAUNCH_ROPE(INV)                                                       \
  hipLaunchKernelGGL((rope_qk_kernel<INV>), grid, block, 0, stream, cbf(q),    \
                     cbf(k), cbf(cc), cbf(sc), bf(qo), bf(ko), n_items,        \
                     (int)L, (int)D, (int)Hq, (int)Hkv, q_sb, q_sh, q_sl,      \
                     k_sb, k_sh, k_sl, cs_sb)
    if (inverse) LAUNCH_ROPE(true);
    else LAUNCH_ROPE(false);
#undef LAUNCH_ROPE
  }
  return {qo.transpose(1, 2), ko.transpose(1, 2)};
}

namespace {

// [rows, I] bf16 view with unit column stride -> row stride in elements
int64_t swiglu_rows(const torch::Tensor& t, int64_t rows, int64_t I,
                    const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
              t.dim() == 2 && t.size(0) == rows && t.size(1) == I,
              "swiglu: ", what, " must be a bf16 CUDA [rows, I] tensor");
  TORCH_CHECK(t.stride(1) == 1 && aligned16(t.data_ptr()),
              "swiglu: ", what, " needs unit column stride and 16-byte "
              "alignment");
  if (rows == 1) return 0;
  const int64_t s = t.stride(0);
  TORCH_CHECK(s >= I && s % 8 == 0, "swiglu: ", what, " row stride ", s,
              " must be >= I and a multiple of 8");
  return s;
}

int swiglu_grid(int64_t n_chunks) {
  return (int)std::min<int64_t>((n_chunks + 255) / 256, SWIGLU_MAX_BLOCKS);
}

}  // namespace

torch::Tensor swiglu_fwd(torch::Tensor gate, torch::Tensor up) {
  TORCH_CHECK(gate.dim() == 2, "swiglu: expected 2-D inputs");
  const int64_t rows = gate.size(0), I = gate.size(1);
  TORCH_CHECK(I > 0 && I % 8 == 0 && I < (1LL << 31),
              "swiglu: I must be a positive multiple of 8");
  const int64_t g_sr = swiglu_rows(gate, rows, I, "gate");
  const int64_t u_sr = swiglu_rows(up, rows, I, "up");
  auto y = torch::empty({rows, I}, gate.options());
  const int64_t n_chunks = rows * (I / 8);
  if (n_chunks == 0) return y;
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(swiglu_fwd_kernel, dim3(swiglu_grid(n_chunks)), dim3(256),
                     0, stream, cbf(gate), cbf(up), bf(y), n_chunks,
                     (int)(I / 8), g_sr, u_sr);
  return y;
}

// -> (dgate, dup), both contiguous [rows, I]
std::vector<torch::Tensor> swiglu_bwd(torch::Tensor dy, torch::Tensor gate,
                                      torch::Tensor up) {
  TORCH_CHECK(gate.dim() == 2, "swiglu: expected 2-D inputs");
  const int64_t rows = gate.size(0), I = gate.size(1);
  TORCH_CHECK(I > 0 && I % 8 == 0 && I < (1LL << 31),
              "swiglu: I must be a positive multiple of 8");
  const int64_t g_sr = swiglu_rows(gate, rows, I, "gate");
  const int64_t u_sr = swiglu_rows(up, rows, I, "up");
  const int64_t dy_sr = swiglu_rows(dy, rows, I, "dy");
  auto dgate = torch::empty({rows, I}, gate.options());
  auto dup = torch::empty({rows, I}, gate.options());
  const int64_t n_chunks = rows * (I / 8);
  if (n_chunks == 0) return {dgate, dup};
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3(swiglu_grid(n_chunks)), dim3(256),
                     0, stream, cbf(dy), cbf(gate), cbf(up), bf(dgate),
                     bf(dup), n_chunks, (int)(I / 8), dy_sr, g_sr, u_sr);
  return {dgate, dup};
}

}  // namespace genrec
