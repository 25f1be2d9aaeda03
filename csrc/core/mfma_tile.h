// Tile primitives shared by the v_mfma_f32_16x16x32_bf16 kernels
// (attention_mfma, attention_flash, hstu_attn, attention_gqa, attention_beam,
// skinny_gemm). This header stops at fragment level; the strip-level steps
// of a flash tile that attention_gqa, attention_beam, attention_flash and
// hstu_attn share (strip products, key columns, masking, running softmax,
// stashes, row store, backward products) are built on it in flash_strip.h.
//
// LDS image: a tile is 64 rows of bf16 with 128-byte rows (64 columns) or
// 256-byte rows (128 columns), stored with an XOR swizzle on 16-byte slots
// (byte ^= (row&7)<<4) so ds_read_b128 fragment loads are conflict-free.
// A/B operands are natural 16-byte row chunks (lane l: row l&15, k-chunk
// (l>>4)*8), so a fragment load is a single b128 read. Transposed images
// are built from coalesced b128 natural-row global loads, an in-register
// 8x8 butterfly transpose across the lane group and ONE b128 store
// (tile_store_tr), or not built at all: a dual-use image (swz_dual) is a
// natural tile that frag_load_tr reads by columns with ds_read_b64_tr_b16
// (attention_mfma; the other kernels still stage transposed copies).
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

// Dual-use image (128-byte rows only): one natural row-major tile that is
// read by rows (frag_load, ds_read_b128) AND by columns (frag_load_tr,
// ds_read_b64_tr_b16). The slot XOR is row bits {0,1,3} instead of {0,1,2}.
// Bank = (byte/4) % 64 for both reads, so row bit 0 picks the 32-bank half
// and the XOR has to separate the even (odd) rows that one lane group
// touches in the same 16-byte slot column:
//   b128 row read, groups {0-3,12-15,20-27} / {4-11,16-19,28-31}: rows>>1 in
//     {0,1,6,7} share one slot, {2,3,4,5} the next -> (bit1,bit3) distinct;
//   tr read, per 32-lane half two 4-row blocks 8 rows apart: rows>>1 in
//     {0,1,4,5} or {2,3,6,7} on one 32-byte column pair -> (bit1,bit3)
//     distinct, where (row&7) maps both blocks to the same banks (2-way).
// Both reads are conflict-free; b128 / b64 stores bank as with swz().
// Store and read a dual-use tile only through tile_off<true>.
__device__ __forceinline__ int swz_dual(int row, int byte_in_row) {
  return row * 128 + (byte_in_row ^ (((row & 3) | ((row & 8) >> 1)) << 4));
}

// the one offset function of a tile: DUAL picks the image
template <bool DUAL>
__device__ __forceinline__ int tile_off(int row, int byte_in_row,
                                        int row_bytes) {
  return DUAL ? swz_dual(row, byte_in_row) : swz(row, byte_in_row, row_bytes);
}

// load one 16x32 A/B fragment (8 bf16 = 16 B per lane) from a swizzled tile
template <bool DUAL = false>
__device__ __forceinline__ short8v frag_load(const char* base, int row0,
                                             int k0, int lane,
                                             int row_bytes = 128) {
  int row = row0 + (lane & 15);
  int byte = (k0 + ((lane >> 4) << 3)) * 2;
  return *reinterpret_cast<const short8va*>(
      base + tile_off<DUAL>(row, byte, row_bytes));
}

// Transposed fragment load from a dual-use tile: the operand's k index runs
// down the tile's rows [k_row0, k_row0+32) and its m/n index along columns
// [col0, col0+16). Returns what frag_load(row0=col0, k0=k_row0) reads from
// the transposed image, same k order, as two ds_read_b64_tr_b16: per
// 16-lane group g the instruction gathers a 4-row x 16-column block and
// hands lane i column i, so rows 8g..8g+3 fill elements 0..3 and rows
// 8g+4..8g+7 elements 4..7. Lane 16g+4q+p supplies the address of row
// k_row0+8g+q (+4), columns col0+4p..+3 (8-byte aligned; the 16-byte slot
// XOR keeps them contiguous).
// EXEC must be all ones: call only from wave-uniform control flow, on a
// tile zero-padded to 64x64 so every lane's address is in bounds.
__device__ __forceinline__ short8v frag_load_tr(const char* tile, int k_row0,
                                                int col0, int lane) {
  typedef __attribute__((address_space(3))) short4v lds_short4v;
  const int row = k_row0 + ((lane >> 4) << 3) + ((lane >> 2) & 3);
  const int byte = (col0 + ((lane & 3) << 2)) * 2;
  short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_short4v*)(tile + tile_off<true>(row, byte, 128)));
  short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_short4v*)(tile + tile_off<true>(row + 4, byte, 128)));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
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

// chunk idx of a [64][64] tile walked row by row in 8-column chunks (the
// loop of a kernel whose D <= 64 is an argument; a chunk at d0 >= D is zero)
struct TileChunk {
  int row, d0;
};
__device__ __forceinline__ TileChunk tile_chunk(int idx) {
  return {idx / (TILE / 8), (idx % (TILE / 8)) * 8};
}
constexpr int TILE_CHUNKS = TILE * (TILE / 8);

// 16-byte global load of the 8 bf16 at base[off..off+7]; zero when !pred
// (the address is then neither formed nor read)
__device__ __forceinline__ short8v load8(const __hip_bfloat16* base,
                                         int64_t off, bool pred) {
  short8v val = {};
  if (pred) val = *reinterpret_cast<const short8v*>(base + off);
  return val;
}

// natural store of 8 / 4 / 1 bf16 at (row, column d0) of a tile
template <bool DUAL = false>
__device__ __forceinline__ void tile_store(char* tile, int row, int d0,
                                           short8v val, int row_bytes = 128) {
  *reinterpret_cast<short8va*>(
      tile + tile_off<DUAL>(row, d0 * 2, row_bytes)) = val;
}
template <bool DUAL = false>
__device__ __forceinline__ void tile_store(char* tile, int row, int d0,
                                           short4v val, int row_bytes = 128) {
  *reinterpret_cast<short4va*>(
      tile + tile_off<DUAL>(row, d0 * 2, row_bytes)) = val;
}
template <bool DUAL = false>
__device__ __forceinline__ void tile_store(char* tile, int row, int d0,
                                           short val, int row_bytes = 128) {
  *reinterpret_cast<short1a*>(
      tile + tile_off<DUAL>(row, d0 * 2, row_bytes)) = val;
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

// Stage 64 rows x D of a [*, L, D]-strided operand (row stride sl) into a
// natural tile nat[64][D] and/or a transposed tile tr[D][64] (256 threads).
// Rows at or beyond L, and rows that row_pad (null | [L]) marks, are zero.
// Items are walked in 64-wide column halves so that the 8 lanes
// (lane>>3)&7 of a wave hold 8 consecutive rows of one 8-column chunk,
// which is what the in-register transpose needs. Every thread runs the same
// number of iterations (shuffles inside).
template <int D, bool NAT, bool TR>
__device__ __forceinline__ void gstage(const __hip_bfloat16* __restrict__ src,
                                       int64_t sl, int r0, int L, char* nat,
                                       char* tr, int tid,
                                       const bool* row_pad = nullptr) {
  const int lane = tid & 63;
  for (int idx = tid; idx < TILE * (D / 8); idx += 256) {
    int half = idx >> 9;          // 512 items per 64-column half
    int rem = idx & 511;
    int row = rem >> 3;
    int d0 = half * 64 + (rem & 7) * 8;
    int gi = r0 + row;
    bool live = gi < L;
    if (live && row_pad) live = !row_pad[gi];
    short8v val = load8(src, (int64_t)gi * sl + d0, live);
    if (NAT) tile_store(nat, row, d0, val, D * 2);
    if (TR) tile_store_tr(tr, row, d0, lane, val);
  }
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
