// Tile primitives shared by the v_mfma_f32_16x16x32_bf16 kernels
// (attention_mfma, attention_flash, hstu_attn, attention_gqa, skinny_gemm).
//
// LDS image: a tile is 64 rows of bf16 with 128-byte rows (64 columns) or
// 256-byte rows (128 columns), stored with an XOR swizzle on 16-byte slots
// (byte ^= (row&7)<<4) so ds_read_b128 fragment loads are conflict-free.
// A/B operands are natural 16-byte row chunks (lane l: row l&15, k-chunk
// (l>>4)*8), so a fragment load is a single b128 read. Transposed images
// are built from coalesced b128 natural-row global loads, an in-register
// 8x8 butterfly transpose across the lane group and ONE b128 store.
//
// C/D fragment layout: lane l holds rows (l>>4)*4 + reg (reg = 0..3) of
// column l&15 — a row reduction is an op over the column fragments
// followed by shuffle-xor over the 16-lane group.
//
// Tiles are written with one vector width and read back with another, so
// every LDS access here goes through a may_alias type.
#pragma once

#include "common.h"

namespace genrec {

typedef __attribute__((ext_vector_type(8))) short short8v;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(4))) float float4v;
typedef short8v __attribute__((may_alias)) short8va;
typedef short4v __attribute__((may_alias)) short4va;
typedef float4v __attribute__((may_alias)) float4va;
typedef short __attribute__((may_alias)) short1a;

constexpr int TILE = 64;           // tile rows (queries / keys per block)
constexpr float NEG_BIG = -1e9f;   // masked score

// flat index into a contiguous [*, H, I, J] tensor
__device__ __forceinline__ int64_t idx4(int b, int h, int i, int j, int H,
                                        int I, int J) {
  return (((int64_t)b * H + h) * I + i) * J + j;
}

// swizzled byte offset of (row, byte_in_row) in a tile
__device__ __forceinline__ int swz(int row, int byte_in_row,
                                   int row_bytes = 128) {
  return row * row_bytes + (byte_in_row ^ ((row & 7) << 4));
}

// load one 16x32 A/B fragment (8 bf16 = 16 B per lane) from a swizzled tile
__device__ __forceinline__ short8v frag_load(const char* base, int row0,
                                             int k0, int lane,
                                             int row_bytes = 128) {
  int row = row0 + (lane & 15);
  int byte = (k0 + ((lane >> 4) << 3)) * 2;
  return *reinterpret_cast<const short8va*>(base + swz(row, byte, row_bytes));
}

// In-register 8x8 bf16 block transpose across the 8 lanes {8g+c : g=0..7}
// (3 butterfly stages of shfl_xor; validated against a host simulation).
// Turns a lane's natural row-chunk into a transposed row-chunk so the
// LDS transpose staging becomes ONE b128 store instead of 8 scattered
// u16 stores. A variant that exchanges only the four replaced elements per
// stage, packed two per shuffle, measured slower.
__device__ __forceinline__ void xpose8x8(short (&vals)[8], int g) {
#pragma unroll
  for (int m = 1; m < 8; m <<= 1) {
    short nv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int t = __shfl_xor((int)vals[e ^ m], 8 * m, 64);
      nv[e] = ((e & m) != (g & m)) ? (short)t : vals[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) vals[e] = nv[e];
  }
}

// ---- per-chunk staging (one 8-element chunk per call; the caller owns the
// loop, so several tensors' global loads stay in flight together)

// 16-byte global load of the 8 bf16 at base[off..off+7]; zero when !pred
// (the address is then neither formed nor read)
__device__ __forceinline__ short8v load8(const __hip_bfloat16* base,
                                         int64_t off, bool pred) {
  short8v val = {};
  if (pred) val = *reinterpret_cast<const short8v*>(base + off);
  return val;
}

// natural store of 8 / 4 / 1 bf16 at (row, column d0) of a tile
__device__ __forceinline__ void tile_store(char* tile, int row, int d0,
                                           short8v val, int row_bytes = 128) {
  *reinterpret_cast<short8va*>(tile + swz(row, d0 * 2, row_bytes)) = val;
}
__device__ __forceinline__ void tile_store(char* tile, int row, int d0,
                                           short4v val, int row_bytes = 128) {
  *reinterpret_cast<short4va*>(tile + swz(row, d0 * 2, row_bytes)) = val;
}
__device__ __forceinline__ void tile_store(char* tile, int row, int d0,
                                           short val, int row_bytes = 128) {
  *reinterpret_cast<short1a*>(tile + swz(row, d0 * 2, row_bytes)) = val;
}

// transposed store: val is source (row, d0..d0+7); the 8 lanes (lane>>3)&7
// of a wave must hold 8 consecutive rows of the same chunk. After the
// transpose this lane holds source rows (row&~7)..+7 of column d0+g, which
// is one b128 chunk of row d0+g in the [*][64] transposed tile.
__device__ __forceinline__ void tile_store_tr(char* tile, int row, int d0,
                                              int lane, short8v val) {
  const int g = (lane >> 3) & 7;
  short t[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) t[e] = val[e];
  xpose8x8(t, g);
  short8v pack;
#pragma unroll
  for (int e = 0; e < 8; ++e) pack[e] = t[e];
  tile_store(tile, d0 + g, row & ~7, pack);
}

__device__ __forceinline__ float4v mfma_bf16(short8v a, short8v b,
                                             float4v acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}

// C-fragment coordinates of a lane: its column, and the first of its 4 rows
__device__ __forceinline__ int frag_col(int lane) { return lane & 15; }
__device__ __forceinline__ int frag_row0(int lane) { return (lane >> 4) << 2; }

// reductions over the 16 lanes that hold one C-fragment row
__device__ __forceinline__ float grp16_max(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float grp16_sum(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ short bf16_bits(float x) {
  __hip_bfloat16 h = __float2bfloat16(x);
  return *reinterpret_cast<short*>(&h);
}

}  // namespace genrec
