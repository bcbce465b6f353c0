// Common helpers for the drla gfx950 kernels.
// CDNA4: wave64, 256 CUs / 8 XCDs; memory-bound kernels follow the
// grid-stride + vectorized-access pattern (guide §6 G11/G13).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

// ---- types shared by the kernels and their launchers ----------------------
typedef unsigned short bf16raw;  // bf16 bit pattern
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) unsigned short ushort4v;

#define DRLA_WAVE 64
// squared-norm partials: 16 slots, each on its own 64 B cache line
// (buffer length = 16*16 floats; slot s lives at [s*16])
#define DRLA_NORM_SLOTS 16
// conv bias-grad partials: drla_relu_mask_bwd spreads its atomics over
// DRLA_DBIAS_SLOTS rows of DRLA_DBIAS_STRIDE (>= max CO) floats;
// drla_wgrad_finalize sums and re-zeroes them
#define DRLA_DBIAS_SLOTS 16
#define DRLA_DBIAS_STRIDE 64
#define DRLA_BLOCK 256

// ---- shapes the host launch code and the kernels must agree on ------------

// conv stack: one row per kernel family member (NHWC, VALID padding)
struct DrlaConvLayer { int ci, co, kh, kw, stride, hi, wi, ho, wo; };
constexpr DrlaConvLayer DRLA_CONV_LAYERS[4] = {
    {4, 32, 8, 8, 4, 84, 84, 20, 20},   // 0: l1 (u8 x4)
    {1, 32, 8, 8, 4, 84, 84, 20, 20},   // 1: l1_c1 (u8 x1)
    {32, 64, 4, 4, 2, 20, 20, 9, 9},    // 2: l2
    {64, 64, 3, 3, 1, 9, 9, 7, 7},      // 3: l3
};
// the nine template arguments of the conv_*_impl kernels for layer l
#define DRLA_CONV_GEOM(l)                                               \
  DRLA_CONV_LAYERS[l].ci, DRLA_CONV_LAYERS[l].co, DRLA_CONV_LAYERS[l].kh, \
      DRLA_CONV_LAYERS[l].kw, DRLA_CONV_LAYERS[l].stride,               \
      DRLA_CONV_LAYERS[l].hi, DRLA_CONV_LAYERS[l].wi,                   \
      DRLA_CONV_LAYERS[l].ho, DRLA_CONV_LAYERS[l].wo
#define DRLA_CONV_BLOCK 256    // threads per block, every conv kernel
#define DRLA_CONV_BM 128       // fwd/dgrad rows per block (grid.x = M / BM)
#define DRLA_CONV_WGRAD_BK 64  // wgrad k-rows per block (grid.x = K / BK)

// 3x3 / stride 1 / zero padding 1 family of the IMPALA ResNet torso
// (conv3x3.hip). The Python layer ids continue DRLA_CONV_LAYERS: id =
// DRLA_CONV3_FIRST + row. Square images, hw = H = W in and out.
struct DrlaConv3Layer { int ci, co, hw; };
#define DRLA_CONV3_FIRST 4
#define DRLA_CONV3_COUNT 5
constexpr DrlaConv3Layer DRLA_CONV3_LAYERS[DRLA_CONV3_COUNT] = {
    {4, 16, 84},   // 4: section 1 conv
    {16, 16, 42},  // 5: section 1 residual blocks
    {16, 32, 42},  // 6: section 2 conv
    {32, 32, 21},  // 7: section 2 residual blocks, section 3 conv
    {32, 32, 11},  // 8: section 3 residual blocks
};
#define DRLA_CONV3_WGRAD_ROWS 64  // wgrad m-rows per chunk
// wgrad scratch: [9*ci + 1][co] f32, the last row is the bias gradient
constexpr int DRLA_CONV3_SCRATCH_ELEMS = (9 * 32 + 1) * 32;

// fused V-trace loss: T sizes the LDS scan buffers, A is the softmax width
#define VT_MAX_T 128
#define VT_MAX_A 64

// fused MLP heads / action-embedding MLP: hidden width and rows per block
#define MH_HID 256
#define MH_BM 16
#define MH_MAX_A 32  // policy out layer is one padded 32-column tile

// dueling heads (r2d2_loss.hip): dim caps of the no-grad head, and the
// dynamic LDS of the no-grad / train-fwd kernels — bf16 Wt [MID][IN] and
// Wo [AO][MID], then f32 x [2][MID], h [2][IN], y [2][AO]
#define DHEAD_MAX_IN 256
#define DHEAD_MAX_MID 512
#define DHEAD_MAX_AO 64
#define DRLA_LDS_BUDGET (160 * 1024)
constexpr size_t drla_dhead_fwd_lds_bytes(int IN, int MID, int AO) {
  return (size_t)(MID * IN + AO * MID) * sizeof(bf16raw) +
         (size_t)(2 * MID + 2 * IN + 2 * AO) * sizeof(float);
}

// LSTM sequence kernels: blockDim = 4H gates, capped by the block size;
// static LDS = one f32 per gate; dynamic LDS = bf16 Wh [H][4H], then two
// f32 [H] carries (+16 B slack). drla_lstm_seq_fwd_gmem leaves Wh in global
// memory for a hidden size whose Wh does not fit.
#define LSTM_SEQ_MAX_GATES 1024
#define LSTM_SEQ_STATIC_LDS_BYTES (LSTM_SEQ_MAX_GATES * (int)sizeof(float))
constexpr int drla_lstm_seq_wh_elems(int H) { return H * 4 * H; }
constexpr int drla_lstm_seq_lds_bytes(int H, bool wh_in_lds = true) {
  return (wh_in_lds ? drla_lstm_seq_wh_elems(H) * (int)sizeof(bf16raw) : 0) +
         2 * H * (int)sizeof(float) + 16;
}
constexpr bool drla_lstm_seq_wh_fits_lds(int H) {
  return drla_lstm_seq_lds_bytes(H) + LSTM_SEQ_STATIC_LDS_BYTES <=
         DRLA_LDS_BUDGET;
}

// wide family (drla_lstm_seq_wide_*): fixed block, every thread strides over
// the gate columns, Wh streamed from global memory; dynamic LDS = f32 gate
// (backward: gate-grad) buffer [4H], then two f32 [H] carries
#define LSTM_SEQ_MAX_HIDDEN 512
#define LSTM_SEQ_WIDE_BLOCK 1024
constexpr int drla_lstm_seq_wide_lds_bytes(int H) {
  return (4 * H + 2 * H) * (int)sizeof(float);
}
static_assert(drla_lstm_seq_wide_lds_bytes(LSTM_SEQ_MAX_HIDDEN) <= 16 * 1024,
              "wide LSTM kernels keep only gates and carries in LDS");
// the LDS-resident train pair takes a size iff its block, Wh and the 120 KB
// Wh cap all fit (H <= 123); every other size goes to the wide pair
constexpr bool drla_lstm_seq_train_in_lds(int H) {
  return 4 * H <= LSTM_SEQ_MAX_GATES && drla_lstm_seq_wh_fits_lds(H) &&
         drla_lstm_seq_wh_elems(H) * (int)sizeof(bf16raw) <= 120 * 1024;
}
static_assert(drla_lstm_seq_train_in_lds(123) &&
                  !drla_lstm_seq_train_in_lds(124),
              "train-pair dispatch boundary");

// cap grids at ~8 blocks/CU x 256 CUs and grid-stride the rest
#define DRLA_MAX_BLOCKS 2048

static inline int drla_grid(long long work_items, int block = DRLA_BLOCK) {
  long long blocks = (work_items + block - 1) / block;
  if (blocks > DRLA_MAX_BLOCKS) blocks = DRLA_MAX_BLOCKS;
  if (blocks < 1) blocks = 1;
  return static_cast<int>(blocks);
}

// Defensive clamp for indices that arrive from EXTERNAL data (actor
// rings, replay payloads): an out-of-range action must not become a GPU
// aperture fault that takes the whole learner down — corrupt input
// yields a wrong-but-bounded read instead.
__device__ __forceinline__ int drla_clamp_idx(int a, int n) {
  return a < 0 ? 0 : (a >= n ? n - 1 : a);
}

// Double-buffered static inputs (runtime/graphed.py): a captured graph has
// fixed addresses, so a kernel that reads such an input takes the address of
// set 0, the element distance to set 1 and a device-side slot word (0 or 1)
// that the host writes before the replay. slot == null: the pointer as given.
// One uniform load per call; kernels call it once per input, at entry.
template <typename T>
__device__ __forceinline__ const T* drla_slot_base(const T* p,
                                                   const int* slot,
                                                   long long dist) {
  return slot ? p + (long long)(*slot != 0) * dist : p;
}

__device__ __forceinline__ float drla_sigmoid(float x) {
  return 1.0f / (1.0f + __expf(-x));
}

// bf16 raw bits -> f32 (exact: the bits become the high half)
__device__ __forceinline__ float drla_bf16_to_f32(bf16raw u) {
  unsigned int x = ((unsigned int)u) << 16;
  return __uint_as_float(x);
}

// round-to-nearest-even f32 -> bf16 raw bits. gfx950 has a hardware
// packed convert (v_cvt_pk_bf16_f32, 1 VALU op); the bit-math expansion
// costs ~6 ops per value and showed up in the staging-heavy kernels
// (PMC p31: conv_fwd_l1 at 3.7e8 VALU insts).
__device__ __forceinline__ unsigned short drla_f32_to_bf16(float f) {
  __hip_bfloat162 v = __float22bfloat162_rn(float2{f, f});
  return *reinterpret_cast<unsigned short*>(&v);
}

// packed pair -> one u32 (low = a, high = b); single v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned int drla_f32x2_to_bf16x2(float a,
                                                             float b) {
  __hip_bfloat162 v = __float22bfloat162_rn(float2{a, b});
  return *reinterpret_cast<unsigned int*>(&v);
}
