// Device helpers shared by the two conv families (conv.hip, conv3x3.hip):
// the kernel prefix, packed-bf16 bit helpers, the u8 input staging, the
// transposed LDS fragment read and the MFMA step over padded k-major tiles.
#pragma once

#include "drla_kernels.h"

// layer geometry, block size and tile sizes come from drla_common.h, where
// the launch code reads the same values
#define CONV_KERNEL \
  extern "C" __global__ __launch_bounds__(DRLA_CONV_BLOCK) void

// ---- two packed bf16 in one 32-bit word -----------------------------------

// max(x, 0) on both halves: a set sign bit clears its half
__device__ __forceinline__ unsigned int drla_bf16x2_relu(unsigned int v) {
  const unsigned int neg = (v >> 15) & 0x00010001u;
  return v & ~(neg * 0xFFFFu);
}
__device__ __forceinline__ float drla_bf16x2_lo(unsigned int v) {
  return __uint_as_float(v << 16);
}
__device__ __forceinline__ float drla_bf16x2_hi(unsigned int v) {
  return __uint_as_float(v & 0xFFFF0000u);
}

// ---- u8 input staging (8x8 stride-4 first layer, CI = 4 or 1) -------------
// A thread stages 16 consecutive k of one output row, k = (kh*8 + kw)*CI + ci
// starting at a multiple of 16. CI == 4: four pixels of one kernel row, 16
// contiguous 16 B-aligned bytes. CI == 1: two whole kernel rows of 8 bytes
// (4 B-aligned), WI bytes apart. p = the first of them. The 16 raw bytes
// travel in a bf16x8, the 16-byte register type of the bf16 layers' chunks,
// so a kernel keeps one set of prefetch registers for both input types.
typedef __attribute__((ext_vector_type(4))) unsigned int drla_u32x4;

template <int CI, int WI>
__device__ __forceinline__ bf16x8 drla_u8x16_load(const unsigned char* p) {
  static_assert(CI == 4 || CI == 1, "u8 layers have 4 or 1 channels");
  if constexpr (CI == 4) {
    return *reinterpret_cast<const bf16x8*>(p);
  } else {
    const unsigned int* r0 = reinterpret_cast<const unsigned int*>(p);
    const unsigned int* r1 = reinterpret_cast<const unsigned int*>(p + WI);
    return __builtin_bit_cast(bf16x8, drla_u32x4{r0[0], r0[1], r1[0], r1[1]});
  }
}

// 4 u8 -> 4 bf16 of (float)u * (1/255.f), round to nearest even. Written per
// element: with the two packed converts spelled out the compiler pairs bytes
// (0,2) and (1,3) for its packed multiply and re-interleaves the halves
// afterwards (6 more VALU ops per word on gfx950).
__device__ __forceinline__ uint2 drla_u8x4_norm_bf16x4(unsigned int u) {
  const float sc = 1.0f / 255.0f;
  ushort4v r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r[e] = drla_f32_to_bf16((float)((u >> (8 * e)) & 0xFF) * sc);
  }
  return __builtin_bit_cast(uint2, r);
}

// the 16 bytes of drla_u8x16_load -> 16 bf16 as two 16-byte chunks
__device__ __forceinline__ void drla_u8x16_norm_bf16x16(bf16x8 raw,
                                                        bf16x8& lo,
                                                        bf16x8& hi) {
  const drla_u32x4 u = __builtin_bit_cast(drla_u32x4, raw);
  const uint2 c0 = drla_u8x4_norm_bf16x4(u.x);
  const uint2 c1 = drla_u8x4_norm_bf16x4(u.y);
  const uint2 c2 = drla_u8x4_norm_bf16x4(u.z);
  const uint2 c3 = drla_u8x4_norm_bf16x4(u.w);
  lo = __builtin_bit_cast(bf16x8, drla_u32x4{c0.x, c0.y, c1.x, c1.y});
  hi = __builtin_bit_cast(bf16x8, drla_u32x4{c2.x, c2.y, c3.x, c3.y});
}

// ---- MFMA operands from LDS -------------------------------------------------

// one 16x16x32 operand (8 bf16 per lane) from a ROW-MAJOR LDS tile of
// row_bytes per row: two ds_read_b64_tr_b16, rows 8g..8g+3 at p and
// 8g+4..8g+7 four rows down.
// EXEC must be full here (the gather crosses lanes): callers keep uniform
// control flow around it.
__device__ __forceinline__ bf16x8 drla_lds_tr_frag(const unsigned char* p,
                                                   int row_bytes) {
  typedef __attribute__((ext_vector_type(4))) short s16x4;
  typedef __attribute__((address_space(3))) s16x4* lds_ptr;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p);
  const s16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p + 4 * row_bytes));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// one BK = 32 step of a wave's 32 rows x (16 * NFRAG) columns over k-major
// padded tiles At[row][32 + 8], Bt[col][32 + 8]:
//   acc[mi][ni] += At[wave*32 + mi*16 ..][0..31] . Bt[ni*16 ..][0..31].
// Bt is read as the MFMA B operand, which computes At @ Bt^T of the two LDS
// images (pinned by drla_mfma_probe and the tests).
//   A: lane l holds A[l&15][(l>>4)*8 + e], e = 0..7
//   B: lane l holds B[(l>>4)*8 + e][l&15] = Bt[l&15][(l>>4)*8 + e]
template <int NFRAG, int PITCH>
__device__ __forceinline__ void drla_mfma_step_kmajor(
    const bf16raw (*At)[PITCH], const bf16raw (*Bt)[PITCH], int wave,
    int lane, f32x4 (&acc)[2][NFRAG]) {
  for (int mi = 0; mi < 2; ++mi) {
    const bf16x8 a_frag = *reinterpret_cast<const bf16x8*>(
        &At[wave * 32 + mi * 16 + (lane & 15)][(lane >> 4) * 8]);
    for (int ni = 0; ni < NFRAG; ++ni) {
      const bf16x8 b_frag = *reinterpret_cast<const bf16x8*>(
          &Bt[ni * 16 + (lane & 15)][(lane >> 4) * 8]);
      acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_frag, b_frag, acc[mi][ni], 0, 0, 0);
    }
  }
}
