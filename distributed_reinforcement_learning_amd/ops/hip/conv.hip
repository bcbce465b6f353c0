// K1: hand-written implicit-GEMM conv stack for the Atari
// model on gfx950 — MFMA 16x16x32 bf16, LDS-tiled, NHWC, VALID padding.
//
// Forward kernels fuse: (layer 1) uint8 -> /255 normalize on load, and
// (all layers) bias + ReLU epilogue. Weights are consumed exactly as torch
// stores them channels_last: W[co][kh][kw][ci] == W[co][k] row-major with
// k = (kh*KW + kw)*CI + ci — each LDS B-tile row is one contiguous read.
//
// GEMM view per layer (reference model/impala_actor_critic.py:5-10):
//   L1: M = N*20*20, K = 8*8*C  (C=4: u8 input),  CO = 32
//   L2: M = N*9*9,   K = 4*4*32,                  CO = 64
//   L3: M = N*7*7,   K = 3*3*64,                  CO = 64
//
// Block: 256 threads (4 waves), BM = 128 rows x BN = CO cols, BK = 32.
// Per wave: 32 rows x CO cols as 2 x (CO/16) mfma_f32_16x16x32_bf16
// fragments. A-tile [128][32+8] and B-tile [CO][32+8] live in LDS with
// +8 bf16 row padding (conflict-free ds_read_b128, guide §6 G4).
//
// Fragment maps (verified on-box by drla_mfma_probe + the parity tests):
//   A: lane l holds A[l&15][(l>>4)*8 + e], e = 0..7   (8 bf16 = 4 VGPRs)
//   B: lane l holds B[(l>>4)*8 + e][l&15]             (8 bf16)
//   D: lane l, reg r -> row (l>>4)*4 + r, col l&15    (4 f32)
//
// Three bodies: conv_fwd_impl, conv_wgrad_impl and ONE conv_dgrad_impl for
// both strides (residue classes of the input pixel; stride 1 is the one-class
// case). Shared with conv3x3.hip through conv_tile.h: CONV_KERNEL, the u8
// load + normalize pair both u8 kernels stage with, the transposed LDS
// fragment read of the wgrad, and the MFMA step over the padded tiles that
// forward and dgrad run. The wgrad's LDS maps stay in conv_wgrad_lds.h.

#include "drla_kernels.h"
#include "conv_tile.h"
#include "conv_wgrad_lds.h"

// ---------------------------------------------------------------------------
// layout probe: D = A @ B for one 16x16x32 tile, used by tests to pin the
// fragment maps empirically (guide §3: check with ASYMMETRIC operands).
// A, B row-major [16][32] / [32][16] bf16; D [16][16] f32.
// ---------------------------------------------------------------------------
extern "C" __global__ void drla_mfma_probe(const bf16raw* __restrict__ A,
                                           const bf16raw* __restrict__ B,
                                           float* __restrict__ D) {
  const int l = threadIdx.x;
  bf16x8 a_frag, b_frag;
  for (int e = 0; e < 8; ++e) {
    a_frag[e] = (short)A[(l & 15) * 32 + ((l >> 4) * 8 + e)];
    b_frag[e] = (short)B[((l >> 4) * 8 + e) * 16 + (l & 15)];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag, b_frag, acc, 0, 0, 0);
  for (int r = 0; r < 4; ++r) {
    D[((l >> 4) * 4 + r) * 16 + (l & 15)] = acc[r];
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

template <typename IN_T, int CI, int CO, int KH, int KW, int STRIDE, int HI,
          int WI, int HO, int WO>
__device__ void conv_fwd_impl(const IN_T* __restrict__ in,
                              const bf16raw* __restrict__ w,   // [CO][K]
                              const bf16raw* __restrict__ bias,  // [CO]
                              bf16raw* __restrict__ out,       // [M][CO]
                              int batch,
                              IN_T* __restrict__ x_stash = nullptr,
                              long long out_n_stride = 0) {
  // out_n_stride != 0: sample n's HO*WO*CO outputs start at
  // out + n*out_n_stride (the leading columns of a wider row-major slab)
  // instead of being packed back to back
  constexpr int K = KH * KW * CI;
  constexpr int BM = DRLA_CONV_BM;
  constexpr int BK = 32;
  constexpr int APAD = 8;
  constexpr int NFRAG = CO / 16;
  const int M = batch * HO * WO;

  __shared__ bf16raw Abuf[BM][BK + APAD];
  __shared__ bf16raw Bbuf[CO][BK + APAD];
  __shared__ float BiasBuf[CO];

  const int tid = threadIdx.x;
  const int wave = tid / 64;
  const int lane = tid % 64;
  const int row0 = blockIdx.x * BM;

  if (tid < CO) BiasBuf[tid] = drla_bf16_to_f32(bias[tid]);

  f32x4 acc[2][NFRAG];
  for (int mi = 0; mi < 2; ++mi)
    for (int ni = 0; ni < NFRAG; ++ni)
      acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

  // per-thread A staging assignment: thread t fills row (t>>1),
  // k-halves (t&1)*16..+16 of the 128x32 tile
  const int a_row = tid >> 1;
  const int a_k0 = (tid & 1) * 16;
  const int gm = row0 + a_row;
  // decode output coordinate once
  const int n_idx = gm / (HO * WO);
  const int rem = gm - n_idx * (HO * WO);
  const int ho = rem / WO;
  const int wo = rem - ho * WO;
  const long long in_base =
      ((long long)n_idx * HI + ho * STRIDE) * WI + wo * STRIDE;

  // software-pipelined K-loop: chunk k0+BK's global loads issue into
  // registers while chunk k0's MFMA runs (same structure as the wgrad —
  // the per-chunk load-latency chain is what sets kernel time here)
  constexpr bool U8 = sizeof(IN_T) == 1;
  // u8: ra0 holds the 16 raw bytes
  bf16x8 ra0 = {0, 0, 0, 0, 0, 0, 0, 0}, ra1 = ra0;
  uint4 rbw4;
  uint2 rbw2;
  constexpr int THREADS_PER_CO = DRLA_CONV_BLOCK / CO;  // 8 (CO=32) or 4
  constexpr int KCHUNK = BK / THREADS_PER_CO;    // 4 or 8
  const int b_co = tid / THREADS_PER_CO;
  const int b_kpart = (tid % THREADS_PER_CO) * KCHUNK;

  auto load_chunk = [&](int k0) {
    if (gm < M) {
      // the thread's 16 k share kh (CI == 1: two kh rows) and are contiguous
      // in memory from (kh, kw, ci)
      const int kk = k0 + a_k0;
      const int kh = kk / (KW * CI);
      const int kwci = kk - kh * KW * CI;
      const int kw = kwci / CI;
      const int ci = kwci - kw * CI;
      const IN_T* src = in + (in_base + (long long)kh * WI + kw) * CI + ci;
      if constexpr (U8) {
        ra0 = drla_u8x16_load<CI, WI>(src);
      } else {
        ra0 = *reinterpret_cast<const bf16x8*>(src);
        ra1 = *reinterpret_cast<const bf16x8*>(src + 8);
      }
    }
    const bf16raw* src = w + (long long)b_co * K + k0 + b_kpart;
    if constexpr (KCHUNK == 8) {
      rbw4 = *reinterpret_cast<const uint4*>(src);
    } else {
      rbw2 = *reinterpret_cast<const uint2*>(src);
    }
  };

  auto store_chunk = [&]() {
    // rows past M are zeros. A branch, not a select of the two values: with
    // the select the bf16 layers allocate 70 + 32 registers instead of 48 + 48
    if (gm < M) {
      bf16x8 a0 = ra0, a1 = ra1;
      if constexpr (U8) drla_u8x16_norm_bf16x16(ra0, a0, a1);
      *reinterpret_cast<bf16x8*>(&Abuf[a_row][a_k0]) = a0;
      *reinterpret_cast<bf16x8*>(&Abuf[a_row][a_k0 + 8]) = a1;
    } else {
      for (int t = 0; t < 16; t += 8) {
        *reinterpret_cast<uint4*>(&Abuf[a_row][a_k0 + t]) = uint4{0, 0, 0, 0};
      }
    }
    if constexpr (KCHUNK == 8) {
      *reinterpret_cast<uint4*>(&Bbuf[b_co][b_kpart]) = rbw4;
    } else {
      *reinterpret_cast<uint2*>(&Bbuf[b_co][b_kpart]) = rbw2;
    }
  };

  // fully unrolled: every step's (kh, kw, ci) decode folds to constants
  load_chunk(0);
#pragma unroll
  for (int k0 = 0; k0 < K; k0 += BK) {
    store_chunk();
    __syncthreads();
    if (k0 + BK < K) load_chunk(k0 + BK);
    // wave covers rows [wave*32, wave*32+32) x CO
    drla_mfma_step_kmajor<NFRAG>(Abuf, Bbuf, wave, lane, acc);
    __syncthreads();
  }

  // ---- epilogue: bias + ReLU, bf16 NHWC store ----
  // one addressing path: packed output is the row stride HO*WO*CO
  if (out_n_stride == 0) out_n_stride = (long long)HO * WO * CO;
  for (int mi = 0; mi < 2; ++mi) {
    for (int r = 0; r < 4; ++r) {
      const int grow = row0 + wave * 32 + mi * 16 + (lane >> 4) * 4 + r;
      if (grow < M) {
        const int n = grow / (HO * WO);
        bf16raw* orow = out + (long long)n * out_n_stride +
                        (grow - n * (HO * WO)) * CO + (lane & 15);
        for (int ni = 0; ni < NFRAG; ++ni) {
          const float v =
              fmaxf(acc[mi][ni][r] + BiasBuf[ni * 16 + (lane & 15)], 0.0f);
          orow[ni * 16] = drla_f32_to_bf16(v);
        }
      }
    }
  }

  // pass-through input stash (graphed-IMPALA l1): the overlapped H2D of
  // the NEXT batch rewrites the static input during the backward, but
  // the l1 wgrad re-reads the input — stashing it here (bundled stores,
  // no extra launch) moves that read inside the forward for ~4 us
  // instead of a ~20 us standalone clone. Byte count is 16-divisible for
  // every supported geometry (binding checks).
  if (x_stash) {
    const long long n16 =
        (long long)batch * HI * WI * CI * (long long)sizeof(IN_T) / 16;
    const uint4* src = reinterpret_cast<const uint4*>(in);
    uint4* dst = reinterpret_cast<uint4*>(x_stash);
    const long long nthreads = gridDim.x * (long long)blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         i < n16; i += nthreads) {
      dst[i] = src[i];
    }
  }
}

CONV_KERNEL drla_conv_fwd_l1(
    const unsigned char* in, const bf16raw* w, const bf16raw* bias,
    bf16raw* out, int batch, unsigned char* x_stash, const int* slot,
    long long in_dist) {
  in = drla_slot_base(in, slot, in_dist);
  conv_fwd_impl<unsigned char, DRLA_CONV_GEOM(0)>(in, w, bias, out, batch,
                                                  x_stash);
}

CONV_KERNEL drla_conv_fwd_l1_c1(
    const unsigned char* in, const bf16raw* w, const bf16raw* bias,
    bf16raw* out, int batch, unsigned char* x_stash, const int* slot,
    long long in_dist) {
  in = drla_slot_base(in, slot, in_dist);
  // R2D2's single-channel POMDP frames: CI=1 -> K=64; stage per-tap scalars
  conv_fwd_impl<unsigned char, DRLA_CONV_GEOM(1)>(in, w, bias, out, batch,
                                                  x_stash);
}

CONV_KERNEL drla_conv_fwd_l2(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias, bf16raw* out,
    int batch, long long out_n_stride) {
  conv_fwd_impl<bf16raw, DRLA_CONV_GEOM(2)>(in, w, bias, out, batch, nullptr,
                                            out_n_stride);
}

CONV_KERNEL drla_conv_fwd_l3(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias, bf16raw* out,
    int batch, long long out_n_stride) {
  conv_fwd_impl<bf16raw, DRLA_CONV_GEOM(3)>(in, w, bias, out, batch, nullptr,
                                            out_n_stride);
}

// ---------------------------------------------------------------------------
// backward helpers
// ---------------------------------------------------------------------------

// dY_masked = dY * (Y > 0) with dbias partials FUSED into the same pass.
// Thread-to-column pinning: with blockDim (256) and the grid both multiples
// of CO (CO in {32,64}), a grid-stride walk keeps every thread on ONE co
// column — local accumulate, LDS-reduce per co, one atomicAdd per (block,
// co). 640 blocks adding the SAME [CO] addresses serialize (~10 us,
// r24/r25 — same pathology as sq_norm), so partials spread over 16 slots
// of a persistent [16][64] buffer; drla_wgrad_finalize (which always runs
// next in the conv backward) does the 16-way sum, emits bf16 dbias, and
// re-zeroes the slots.
// dy may be an N-strided view (a slice of the fused xh gradient):
// row_elems = elements per logical row, n_stride = elements between row
// starts; row_elems == n_stride means contiguous. Chunks never straddle
// rows (row_elems % 8 == 0).
extern "C" __global__ void drla_relu_mask_bwd(
    const bf16raw* __restrict__ dy, const bf16raw* __restrict__ y,
    bf16raw* __restrict__ out, float* __restrict__ dbias_slots,
    long long n, int CO, long long n_stride, long long row_elems,
    long long y_n_stride) {  // same treatment for y (a conv output that
                             // lives in the leading columns of the xh slab)
  // vectorized: each thread moves 8 bf16 per iteration (uint4), which pins
  // it to ONE 8-column group because stride*8 % CO == 0 (CO in {32,64},
  // blockDim 256). Per-thread acc[8] -> LDS -> one atomicAdd per (block,
  // column).
  const long long n8 = n / 8;
  const long long stride = gridDim.x * (long long)blockDim.x;
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const int tid = threadIdx.x;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint4* dy4 = reinterpret_cast<const uint4*>(dy);
  const uint4* y4 = reinterpret_cast<const uint4*>(y);
  uint4* out4 = reinterpret_cast<uint4*>(out);
  // named .x/.y/.z/.w only — a pointer into a local vector can force it
  // to scratch (guide §5.4 rule 20; cost measured on sq_norm_bf16)
#define DRLA_RM_LANE(dw, yw, ow, a0, a1)                              \
  {                                                                   \
    const bf16raw d0 = (bf16raw)((dw) & 0xFFFF);                      \
    const bf16raw d1 = (bf16raw)((dw) >> 16);                         \
    const bf16raw m0 =                                                \
        (drla_bf16_to_f32((bf16raw)((yw) & 0xFFFF)) > 0.0f) ? d0 : (bf16raw)0; \
    const bf16raw m1 =                                                \
        (drla_bf16_to_f32((bf16raw)((yw) >> 16)) > 0.0f) ? d1 : (bf16raw)0;    \
    (ow) = ((unsigned int)m1 << 16) | m0;                             \
    (a0) += drla_bf16_to_f32(m0);                                              \
    (a1) += drla_bf16_to_f32(m1);                                              \
  }
  const long long row8 = row_elems / 8;
  const bool strided = (n_stride != row_elems);
  const bool y_strided = (y_n_stride != row_elems);
  for (; i < n8; i += stride) {
    long long si = i, yi = i;
    if (strided || y_strided) {
      const long long r = i / row8;
      const long long c8 = i - r * row8;
      if (strided) si = (r * n_stride) / 8 + c8;
      if (y_strided) yi = (r * y_n_stride) / 8 + c8;
    }
    const uint4 dv = dy4[si];
    const uint4 yv = y4[yi];
    uint4 ov;
    DRLA_RM_LANE(dv.x, yv.x, ov.x, acc[0], acc[1]);
    DRLA_RM_LANE(dv.y, yv.y, ov.y, acc[2], acc[3]);
    DRLA_RM_LANE(dv.z, yv.z, ov.z, acc[4], acc[5]);
    DRLA_RM_LANE(dv.w, yv.w, ov.w, acc[6], acc[7]);
    out4[i] = ov;
  }
#undef DRLA_RM_LANE
  __shared__ float red[DRLA_BLOCK * 8];
  for (int e = 0; e < 8; ++e) red[tid * 8 + e] = acc[e];
  __syncthreads();
  // column j gets acc[j%8] of every thread whose group (tid*8)%CO == j-j%8
  if (tid < CO) {
    const int g = tid / 8;
    const int e = tid % 8;
    // threads with in-block index t where (t*8)%CO == g*8, i.e.
    // t = g + k*(CO/8)
    float s = 0.0f;
    for (int t = g; t < DRLA_BLOCK; t += CO / 8) s += red[t * 8 + e];
    atomicAdd(&dbias_slots[(blockIdx.x & (DRLA_DBIAS_SLOTS - 1)) *
                               DRLA_DBIAS_STRIDE +
                           tid], s);
  }
}

// cast + transpose the f32 [K][CO] wgrad scratch into bf16 [CO][K]
// (the channels_last weight-grad layout), re-zeroing the persistent
// scratch as it reads (zero-between-calls invariant, no fill kernel).
extern "C" __global__ void drla_wgrad_finalize(
    float* __restrict__ scratch, bf16raw* __restrict__ dw, int K,
    int CO, float* __restrict__ dbias_slots,
    bf16raw* __restrict__ dbias) {
  // bias-grad epilogue: 16-way slot sum from relu_mask_bwd, bf16 out,
  // slots re-zeroed (persistent zero-between-calls buffer)
  if (dbias_slots && blockIdx.x == 0 && (int)threadIdx.x < CO) {
    float s = 0.0f;
    for (int t = 0; t < DRLA_DBIAS_SLOTS; ++t) {
      s += dbias_slots[t * DRLA_DBIAS_STRIDE + threadIdx.x];
      dbias_slots[t * DRLA_DBIAS_STRIDE + threadIdx.x] = 0.0f;
    }
    dbias[threadIdx.x] = drla_f32_to_bf16(s);
  }
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long total = (long long)K * CO;
  const long long stride = gridDim.x * (long long)blockDim.x;
  for (; i < total; i += stride) {
    const int co = i / K;
    const int k = i - (long long)co * K;
    const long long si = (long long)k * CO + co;
    dw[i] = drla_f32_to_bf16(scratch[si]);
    scratch[si] = 0.0f;
  }
}

// ---------------------------------------------------------------------------
// wgrad: dW^T[k][co] = sum_m A_im2col[m][k] * dY[m][co]
// grid: (K/64, S); each block owns 64 k-rows x CO cols and a slice of
// M; partials atomicAdd into the f32 [K][CO] scratch. (A no-atomic
// [S][K][CO] slab variant measured WORSE across the board — the S-deep
// finalize reduce is the new bottleneck — so atomics stay; the real cost
// is the per-chunk global-load latency chain, hence the prefetch below.)
//
// drla_wgrad_finalize stays a launch of its own. Folding it in (a ticket per
// k-block after the atomics, the last block finalizing) needs an agent-scope
// release fence in every block before its ticket, and each such fence is an
// L2 write-back on gfx950: with one thread fencing, l1 (2048 blocks) went
// from 26.5 to 70 us and l2/l3 lost more than the 6 us launch they saved
// (profiles/wgrad_fold_r05.md).
// ---------------------------------------------------------------------------

template <typename IN_T, int CI, int CO, int KH, int KW, int STRIDE, int HI,
          int WI, int HO, int WO>
__device__ void conv_wgrad_impl(const IN_T* __restrict__ in,
                                const bf16raw* __restrict__ dy,  // [M][CO]
                                float* __restrict__ scratch,     // [K][CO]
                                int batch) {
  constexpr int K = KH * KW * CI;
  constexpr int BKM = DRLA_WG_ROWS;  // m-rows per chunk (2 MFMA k-steps)
  constexpr int BKK = DRLA_CONV_WGRAD_BK;  // k-cols per block
  constexpr int NFRAG = CO / 16;
  constexpr int A_ROWB = BKK * 2;  // bytes per LDS row of the A tile
  constexpr int B_ROWB = CO * 2;   // ... of the dY tile
  // dY staging: 8 co (one 16-byte chunk) per thread and pass
  constexpr int B_TPR = CO / 8;                          // threads per row
  constexpr int B_PASSES = BKM * B_TPR / DRLA_CONV_BLOCK;  // 1 or 2
  static_assert(K % BKK == 0, "k-blocks are full: no k range checks below");
  static_assert(BKK == 64 && DRLA_CONV_BLOCK == 256 &&
                    (B_PASSES == 1 || B_PASSES == 2),
                "the maps of conv_wgrad_lds.h assume these");
  const int M = batch * HO * WO;

  // Both tiles are staged ROW-MAJOR, as they come from memory, with 16-byte
  // stores, and read back column-major by ds_read_b64_tr_b16 (layout and
  // bank analysis: conv_wgrad_lds.h). SOFTWARE-PIPELINED: chunk m+1's
  // global loads issue into registers while chunk m's MFMA runs — the
  // per-chunk load-latency chain (time scaled with M/split, not with
  // atomics) overlaps compute.
  // DOUBLE-BUFFERED images: chunk t+1's LDS stores overlap chunk t's
  // MFMAs (different buffer), leaving ONE barrier per chunk instead of
  // two — with the register prefetch this removes the last serial
  // stage of the per-chunk latency chain.
  __shared__ __attribute__((aligned(16))) unsigned char
      Am[2][BKM * A_ROWB];  // A image: [m][k]
  __shared__ __attribute__((aligned(16))) unsigned char
      Bm[2][BKM * B_ROWB];  // dY image: [m][co]

  const int tid = threadIdx.x;

  const int wave = tid / 64;
  const int lane = tid % 64;
  const int k_row0 = blockIdx.x * BKK;

  f32x4 acc[NFRAG];
  for (int ni = 0; ni < NFRAG; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};

  const int m_per_split = (M + gridDim.y - 1) / gridDim.y;
  const int m_begin = blockIdx.y * m_per_split;
  const int m_end = min(M, m_begin + m_per_split);

  // staging assignment: thread t -> A row t>>2 with k-chunk (t&3)*16. The
  // element offset of a k from the row's first input element is m-invariant
  // and precomputed once: the u8 layers load their 16 k from a_off0 alone
  // (drla_u8x16_load), the bf16 layers as two 8-k chunks, which may lie on
  // different kernel rows
  const int a_m = tid >> 2;
  const int a_k = (tid & 3) * 16;
  constexpr bool U8 = sizeof(IN_T) == 1;
  auto k_off = [](int k) {
    const int kh = k / (KW * CI);
    return (long long)kh * WI * CI + (k - kh * KW * CI);
  };
  const long long a_off0 = k_off(k_row0 + a_k);
  const long long a_off1 = k_off(k_row0 + a_k + 8);
  const int b_lm0 = drla_wg_b_slot<CO>(tid, 0).row;
  const int b_ch = drla_wg_b_slot<CO>(tid, 0).ch;
  const int b_co0 = b_ch * 8;
  constexpr int B_PASS_ROWS = drla_wg_b_slot<CO>(0, 1).row;

  // LDS byte offsets (conv_wgrad_lds.h): the thread's store chunks, and its
  // transposed-read bases for the wave's 16 k and for each co tile
  const int a_st0 = drla_wg_chunk_off<A_ROWB>(drla_wg_a_slot(tid, 0).row,
                                              drla_wg_a_slot(tid, 0).ch);
  const int a_st1 = drla_wg_chunk_off<A_ROWB>(drla_wg_a_slot(tid, 1).row,
                                              drla_wg_a_slot(tid, 1).ch);
  const int b_st0 = drla_wg_chunk_off<B_ROWB>(b_lm0, b_ch);
  const int a_rd = drla_wg_tr_off<A_ROWB>(lane, wave);
  int b_rd[NFRAG];
#pragma unroll
  for (int ni = 0; ni < NFRAG; ++ni) {
    b_rd[ni] = drla_wg_tr_off<B_ROWB>(lane, ni);
  }

  // register prefetch state; u8: ra0 holds the 16 raw bytes
  bf16x8 ra0 = {0, 0, 0, 0, 0, 0, 0, 0}, ra1 = ra0;
  bf16x8 rb0 = ra0, rb1 = ra0;
  bool a_live = false, b_live0 = false, b_live1 = false;

  auto load_chunk = [&](int m0) {
    const int m = m0 + a_m;
    a_live = (m < m_end);
    if (a_live) {
      const int n_idx = m / (HO * WO);
      const int rem = m - n_idx * (HO * WO);
      const int ho = rem / WO;
      const int wo = rem - ho * WO;
      const IN_T* src =
          in + (((long long)n_idx * HI + ho * STRIDE) * WI + wo * STRIDE) * CI;
      if constexpr (U8) {
        ra0 = drla_u8x16_load<CI, WI>(src + a_off0);
      } else {
        ra0 = *reinterpret_cast<const bf16x8*>(src + a_off0);
        ra1 = *reinterpret_cast<const bf16x8*>(src + a_off1);
      }
    }
    const int mb0 = m0 + b_lm0;
    b_live0 = (mb0 < m_end);
    if (b_live0) {
      rb0 = *reinterpret_cast<const bf16x8*>(dy + (long long)mb0 * CO + b_co0);
    }
    if constexpr (B_PASSES == 2) {
      const int mb1 = m0 + b_lm0 + B_PASS_ROWS;
      b_live1 = (mb1 < m_end);
      if (b_live1) {
        rb1 = *reinterpret_cast<const bf16x8*>(dy + (long long)mb1 * CO +
                                              b_co0);
      }
    }
  };

  auto store_chunk = [&](int buf) {
    // the thread's 16 k as two 16-byte chunks; rows past m_end are zeros
    bf16x8 a0 = {0, 0, 0, 0, 0, 0, 0, 0}, a1 = a0;
    if (a_live) {
      if constexpr (U8) {
        drla_u8x16_norm_bf16x16(ra0, a0, a1);
      } else {
        a0 = ra0;
        a1 = ra1;
      }
    }
    *reinterpret_cast<bf16x8*>(&Am[buf][a_st0]) = a0;
    *reinterpret_cast<bf16x8*>(&Am[buf][a_st1]) = a1;
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    *reinterpret_cast<bf16x8*>(&Bm[buf][b_st0]) = b_live0 ? rb0 : z;
    if constexpr (B_PASSES == 2) {
      *reinterpret_cast<bf16x8*>(&Bm[buf][b_st0 + B_PASS_ROWS * B_ROWB]) =
          b_live1 ? rb1 : z;
    }
  };

  // ping-pong: store chunk t+1 into the other buffer while chunk t's
  // MFMAs read this one; ONE barrier per chunk
  load_chunk(m_begin);
  store_chunk(0);
  load_chunk(m_begin + BKM);
  __syncthreads();
  int nchunks = 0;
  for (int m0 = m_begin; m0 < m_end; m0 += BKM) ++nchunks;
  for (int t = 0; t < nchunks; ++t) {
    const int cur = t & 1;
    if (t + 1 < nchunks) {
      store_chunk(1 - cur);
      load_chunk(m_begin + (long long)(t + 2) * BKM);
    }
    // uniform control flow from here to the barrier: the transposed reads
    // need every lane (pad, don't mask)
#pragma unroll
    for (int kk = 0; kk < BKM; kk += 32) {
      const bf16x8 a_frag =
          drla_lds_tr_frag(&Am[cur][a_rd + kk * A_ROWB], A_ROWB);
#pragma unroll
      for (int ni = 0; ni < NFRAG; ++ni) {
        const bf16x8 b_frag =
            drla_lds_tr_frag(&Bm[cur][b_rd[ni] + kk * B_ROWB], B_ROWB);
        acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag, b_frag,
                                                          acc[ni], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // a block whose M-slice is empty adds nothing (block-uniform)
  if (nchunks > 0) {
    for (int ni = 0; ni < NFRAG; ++ni) {
      const int co = ni * 16 + (lane & 15);
      for (int r = 0; r < 4; ++r) {
        const int k = k_row0 + wave * 16 + (lane >> 4) * 4 + r;
        atomicAdd(&scratch[(long long)k * CO + co], acc[ni][r]);
      }
    }
  }
}

CONV_KERNEL drla_conv_wgrad_l1(
    const unsigned char* in, const bf16raw* dy, float* scratch, int batch) {
  conv_wgrad_impl<unsigned char, DRLA_CONV_GEOM(0)>(in, dy, scratch, batch);
}
CONV_KERNEL drla_conv_wgrad_l1_c1(
    const unsigned char* in, const bf16raw* dy, float* scratch, int batch) {
  conv_wgrad_impl<unsigned char, DRLA_CONV_GEOM(1)>(in, dy, scratch, batch);
}
CONV_KERNEL drla_conv_wgrad_l2(
    const bf16raw* in, const bf16raw* dy, float* scratch, int batch) {
  conv_wgrad_impl<bf16raw, DRLA_CONV_GEOM(2)>(in, dy, scratch, batch);
}
CONV_KERNEL drla_conv_wgrad_l3(
    const bf16raw* in, const bf16raw* dy, float* scratch, int batch) {
  conv_wgrad_impl<bf16raw, DRLA_CONV_GEOM(3)>(in, dy, scratch, batch);
}

// ---------------------------------------------------------------------------
// dgrad: dX[n,hi,wi,ci] = sum_{kh,kw,co valid} dY[n,ho',wo',co] *
//        W[co][(kh*KW+kw)*CI+ci],  ho' = (hi-kh)/STRIDE (when integral).
//
// Residue classes: for a fixed (ph, pw) = (hi % STRIDE, wi % STRIDE) only the
// taps kh = ph + STRIDE*i, kw = pw + STRIDE*j can contribute, and for those
// ho' = hi/STRIDE - i exactly. Blocks are grouped by class (blockIdx.y), so a
// block walks just the live taps and stages no zeros for dead ones: 4 of 16
// taps for the stride-2 layer, and for stride 1 the one class with every tap.
// Implicit GEMM per class: batch * (HI/STRIDE) * (WI/STRIDE) rows, CI cols,
// reduction over (live tap, co) in steps of one tap x 32 co.
// ---------------------------------------------------------------------------

template <int CI, int CO, int KH, int KW, int STRIDE, int HI, int WI, int HO,
          int WO>
__device__ void conv_dgrad_impl(const bf16raw* __restrict__ dy,  // [M][CO]
                                const bf16raw* __restrict__ w,   // [CO][K]
                                bf16raw* __restrict__ dx,  // [N][HI][WI][CI]
                                int batch) {
  constexpr int K = KH * KW * CI;
  constexpr int BM = DRLA_CONV_BM;
  constexpr int BK = 32;   // one tap x 32 co per step
  constexpr int PAD = 8;
  constexpr int NFRAG = CI / 16;
  constexpr int HC = HI / STRIDE, WC = WI / STRIDE;  // pixels of a class
  constexpr int TH = KH / STRIDE, TW = KW / STRIDE;  // live taps of a class
  constexpr int NSTEPS = TH * TW * (CO / BK);
  static_assert(KH % STRIDE == 0 && KW % STRIDE == 0 && HI % STRIDE == 0 &&
                    WI % STRIDE == 0,
                "every class has the same taps and the same pixel count");
  static_assert(CO % BK == 0, "a step is 32 co of one tap");
  const int ph = blockIdx.y / STRIDE, pw = blockIdx.y % STRIDE;
  const int Mc = batch * HC * WC;  // rows of this class

  __shared__ bf16raw Ad[BM][BK + PAD];    // dY gather: [row][co_local]
  __shared__ bf16raw Bd[CI][BK + PAD];    // W^T image: [ci][co_local]

  const int tid = threadIdx.x;
  const int wave = tid / 64;
  const int lane = tid % 64;
  const int row0 = blockIdx.x * BM;

  f32x4 acc[2][NFRAG];
  for (int mi = 0; mi < 2; ++mi)
    for (int ni = 0; ni < NFRAG; ++ni)
      acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

  // per-thread A staging: row = tid>>1, co-half = (tid&1)*16; the row is
  // pixel (hc*STRIDE + ph, wc*STRIDE + pw) of image n_idx
  const int a_row = tid >> 1;
  const int a_k0 = (tid & 1) * 16;
  const int mc = row0 + a_row;
  const int n_idx = mc / (HC * WC);
  const int rem = mc - n_idx * (HC * WC);
  const int hc = rem / WC;
  const int wc = rem - hc * WC;

  // software-pipelined: next step's globals prefetch into registers
  // during this step's MFMA (see wgrad note)
  uint4 rda0, rda1;
  bf16raw rbw[8];
  // 4 (CI=32) or 8 (CI=64)
  constexpr int CI_PER_T = (CI * BK) / DRLA_CONV_BLOCK;
  const int b_col = tid % BK;
  const int b_ci0 = (tid / BK) * CI_PER_T;

  auto load_chunk = [&](int step) {
    const int t = step / (CO / BK);  // live tap (i, j), row-major
    const int co0 = (step - t * (CO / BK)) * BK;
    const int i = t / TW;
    const int j = t - i * TW;
    const int ho = hc - i;
    const int wo = wc - j;
    if (mc < Mc && ho >= 0 && ho < HO && wo >= 0 && wo < WO) {
      const bf16raw* src =
          dy + ((long long)(n_idx * HO + ho) * WO + wo) * CO + co0 + a_k0;
      rda0 = *reinterpret_cast<const uint4*>(src);
      rda1 = *reinterpret_cast<const uint4*>(src + 8);
    } else {
      rda0 = uint4{0, 0, 0, 0};
      rda1 = uint4{0, 0, 0, 0};
    }
    const int tap = (ph + STRIDE * i) * KW + pw + STRIDE * j;
    const bf16raw* src = w + (long long)(co0 + b_col) * K + tap * CI + b_ci0;
#pragma unroll
    for (int e = 0; e < CI_PER_T; ++e) rbw[e] = src[e];
  };

  auto store_chunk = [&]() {
    *reinterpret_cast<uint4*>(&Ad[a_row][a_k0]) = rda0;
    *reinterpret_cast<uint4*>(&Ad[a_row][a_k0 + 8]) = rda1;
#pragma unroll
    for (int e = 0; e < CI_PER_T; ++e) Bd[b_ci0 + e][b_col] = rbw[e];
  };

  // fully unrolled: every step's tap and co block fold to constants
  load_chunk(0);
#pragma unroll
  for (int step = 0; step < NSTEPS; ++step) {
    store_chunk();
    __syncthreads();
    if (step + 1 < NSTEPS) load_chunk(step + 1);
    drla_mfma_step_kmajor<NFRAG>(Ad, Bd, wave, lane, acc);
    __syncthreads();
  }

  for (int mi = 0; mi < 2; ++mi) {
    for (int r = 0; r < 4; ++r) {
      const int grow = row0 + wave * 32 + mi * 16 + (lane >> 4) * 4 + r;
      if (grow < Mc) {
        long long pix = grow;  // STRIDE == 1: the one class is the image
        if constexpr (STRIDE > 1) {
          const int gn = grow / (HC * WC);
          const int grem = grow - gn * (HC * WC);
          const int ghc = grem / WC;
          pix = ((long long)gn * HI + ghc * STRIDE + ph) * WI +
                (grem - ghc * WC) * STRIDE + pw;
        }
        for (int ni = 0; ni < NFRAG; ++ni) {
          dx[pix * CI + ni * 16 + (lane & 15)] =
              drla_f32_to_bf16(acc[mi][ni][r]);
        }
      }
    }
  }
}

CONV_KERNEL drla_conv_dgrad_l2(
    const bf16raw* dy, const bf16raw* w, bf16raw* dx, int batch) {
  conv_dgrad_impl<DRLA_CONV_GEOM(2)>(dy, w, dx, batch);
}
CONV_KERNEL drla_conv_dgrad_l3(
    const bf16raw* dy, const bf16raw* w, bf16raw* dx, int batch) {
  conv_dgrad_impl<DRLA_CONV_GEOM(3)>(dy, w, dx, batch);
}
