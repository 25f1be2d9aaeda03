// HSTU temporal-bias bucketing, shared by hstu_attn.hip (one tile, L <= 64)
// and hstu_attn_flash.hip (tiled, any L): the ln2 bucket of |ts_i - ts_j|
// (ref hstu.py:352-409, models/hstu.py TemporalBias). One definition, so the
// two kernels put a pair of timestamps into the same bucket.
#pragma once

#include "common.h"

namespace genrec {

__device__ __forceinline__ int time_bucket(long long ti, long long tj,
                                           int n_buckets) {
  long long diff = ti - tj;
  if (diff < 0) diff = -diff;
  if (diff < 1) diff = 1;
  int b = (int)(__logf((float)diff) / 0.693f);
  return min(max(b, 0), n_buckets - 1);
}

}  // namespace genrec
