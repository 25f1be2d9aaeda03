// Host-side helpers shared by the flash_strip.h kernels' launch code
// (attention_gqa, attention_beam, attention_flash, hstu_attn,
// hstu_attn_flash): head-dim dispatch, the stride predicate, operand views
// and pointer casts.
#pragma once

#include <torch/extension.h>

#include <type_traits>

#include "flash_strip.h"

namespace genrec {

// fn(std::integral_constant<int, D>) for the supported head dims; callers
// have checked D to be 64 or 128.
template <typename F>
void dispatch_head_dim(int64_t D, F&& fn) {
  if (D == 64) {
    fn(std::integral_constant<int, 64>{});
  } else {
    fn(std::integral_constant<int, 128>{});
  }
}

// What the kernels' 16-byte loads need: d innermost, the first n_strided
// dims (those that carry batch / head / rows) with strides that are
// multiples of 8 elements, and a 16-byte aligned base.
inline bool ok_strides(const torch::Tensor& t, int n_strided) {
  if (t.stride(t.dim() - 1) != 1) return false;
  for (int d = 0; d < n_strided; ++d) {
    if (t.stride(d) % 8 != 0) return false;
  }
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}
// t itself when the kernels can read it in place, else a contiguous copy
inline torch::Tensor kernel_readable(const torch::Tensor& t, int n_strided) {
  return ok_strides(t, n_strided) ? t : t.contiguous();
}

// Device pointer of an optional bool pad mask (null when absent); hold keeps
// the contiguous tensor alive.
inline const bool* pad_ptr(const c10::optional<torch::Tensor>& pad,
                           torch::Tensor& hold) {
  if (!pad.has_value()) return nullptr;
  hold = pad->contiguous();
  return hold.data_ptr<bool>();
}

inline const __hip_bfloat16* bf16_cptr(const torch::Tensor& t) {
  return reinterpret_cast<const __hip_bfloat16*>(t.data_ptr());
}
inline __hip_bfloat16* bf16_ptr(torch::Tensor& t) {
  return reinterpret_cast<__hip_bfloat16*>(t.data_ptr());
}

// [B,H,L,D] view
inline FlashView view_bhld(const torch::Tensor& t) {
  return {bf16_cptr(t), t.stride(0), t.stride(1), t.stride(2)};
}
// [B,L,H,D] view
inline FlashView view_blhd(const torch::Tensor& t) {
  return {bf16_cptr(t), t.stride(0), t.stride(2), t.stride(1)};
}
// token-major [T,H,D] view of packed sequences: no batch stride
inline FlashView view_thd(const torch::Tensor& t) {
  return {bf16_cptr(t), 0, t.stride(1), t.stride(0)};
}

}  // namespace genrec
