// 3x3, stride-1, zero-padding-1 conv family of the IMPALA ResNet torso on
// gfx950: MFMA 16x16x32 bf16, NHWC, f32 accumulation. Geometries are the rows
// of DRLA_CONV3_LAYERS (drla_common.h); the weight is the channels_last flat
// view W[co][(kh*3+kw)*CI + ci] of nn.Conv2d, as in conv.hip.
//
// Forward and dgrad are ONE implicit-GEMM body (c3_gemm_impl): rows are the
// N*H*W pixels, the reduction runs over (tap, input channel) and the columns
// are the output channels. dgrad is the same same-padding convolution of dY
// with the weight read as W[co][8 - tap][ci] and the channel roles swapped;
// that indexing happens while the weight is staged into LDS (FLIP).
//
//   k-steps: one MFMA reduces 32 k = 32/CIN taps x CIN channels. 9 taps are
//   9 (CIN=32), 5 (CIN=16) or 2 (CIN=4) steps; taps past the ninth have zero
//   weights AND zero A columns, so no weight row is read past its end.
//   borders: a tap outside the image stages zeros into the A tile. The pixel
//   (n, h, w) is decoded per row, so a row block that spans images is fine.
//   operands: the weight image is the MFMA "A" operand and the pixel tile
//   the "B" operand, D[co][pixel]: a lane ends up with 4 CONSECUTIVE output
//   channels of one pixel, so the epilogue moves 8 bytes per access (output,
//   mask and residual alike).
//   epilogue: v = (acc + bias) * (mask > 0) + residual in f32, one rounding
//   to bf16. Absent terms are the exact identities (+0, *1), so forward
//   (bias, residual) and dgrad (mask, addend) share it.
//
// wgrad (c3_wgrad_impl): dW[k][co] = sum_m im2col(act)[m][k] * dY[m][co]. A
// block owns all of K x CO for a slice of M, stages 64-row im2col and dY
// tiles row-major in padded LDS and reads them back column-major with
// ds_read_b64_tr_b16 (the operand map of conv_wgrad_lds.h, without its XOR
// swizzle: these rows are not 64 or 128 bytes, so that header's checks do not
// apply). Column K of the A tile is the constant 1.0, which makes row K of
// the result the bias gradient sum_m dY[m][co] - same pass, same MFMAs.
// Partials go to a persistent f32 scratch [K+1][CO] by atomicAdd;
// drla_c3_wgrad_finalize casts it to bf16 [CO][K] + [CO] and re-zeroes it.
//
// CONV_KERNEL, the packed-bf16 helpers (drla_bf16x2_*) and the transposed
// fragment read (drla_lds_tr_frag) come from conv_tile.h, shared with
// conv.hip. The MFMA step of c3_gemm_impl stays written out here: its
// operand roles are swapped and the weight fragments are held across both
// row tiles, which drla_mfma_step_kmajor does not do.

#include "drla_kernels.h"
#include "conv_tile.h"

namespace {

// ---------------------------------------------------------------------------
// forward / dgrad
// ---------------------------------------------------------------------------
template <int CIN, int COUT, int HW, bool FLIP>
__device__ void c3_gemm_impl(const bf16raw* __restrict__ in,    // [M][CIN]
                             const bf16raw* __restrict__ w,
                             const bf16raw* __restrict__ bias,  // [COUT] / null
                             const bf16raw* __restrict__ mask,  // [M][COUT] / null
                             const bf16raw* __restrict__ res,   // [M][COUT] / null
                             bf16raw* __restrict__ out,         // [M][COUT]
                             int batch, int relu_in) {
  constexpr int BM = DRLA_CONV_BM;
  constexpr int BK = 32;
  constexpr int PAD = 8;
  constexpr int K = 9 * CIN;
  constexpr int NSTEPS = (K + BK - 1) / BK;
  constexpr int KTOT = NSTEPS * BK;
  constexpr int NFRAG = COUT / 16;
  // A staging: a thread owns 16 k of one row = NU units of UE channels
  constexpr int UE = CIN < 16 ? CIN : 16;
  constexpr int NU = 16 / UE;
  static_assert(CIN == 4 || CIN == 16 || CIN == 32, "unit maps below");
  static_assert(COUT == 16 || COUT == 32, "one or two 16-column tiles");
  const int M = batch * HW * HW;

  __shared__ __attribute__((aligned(16))) bf16raw As[BM][BK + PAD];
  __shared__ __attribute__((aligned(16))) bf16raw Bs[COUT][KTOT + PAD];
  __shared__ float BiasBuf[COUT];

  const int tid = threadIdx.x;
  const int wave = tid / 64;
  const int lane = tid % 64;

  // ---- whole weight -> LDS, once per block: Bs[col][tap*CIN + c] ----------
  if (tid < COUT) {
    BiasBuf[tid] = bias ? drla_bf16_to_f32(bias[tid]) : 0.0f;
  }
  if constexpr (!FLIP) {
    // col = co, the row of W as it lies in memory; 4 k per 8-byte load
    for (int i = tid; i < COUT * (KTOT / 4); i += DRLA_CONV_BLOCK) {
      const int col = i / (KTOT / 4);
      const int k = (i - col * (KTOT / 4)) * 4;
      uint2 v = {0u, 0u};
      if (k < K) {  // K % 4 == 0: a unit is all inside or all outside
        v = *reinterpret_cast<const uint2*>(w + (long long)col * K + k);
      }
      *reinterpret_cast<uint2*>(&Bs[col][k]) = v;
    }
  } else {
    // the conv has CI = COUT and CO = CIN: Bs[ci][tap*CIN + co] =
    // W[co][(8 - tap)*COUT + ci]; 4 ci per 8-byte load, scattered to 4 rows
    constexpr int WROW = 9 * COUT;
    for (int i = tid; i < KTOT * (COUT / 4); i += DRLA_CONV_BLOCK) {
      const int k = i / (COUT / 4);
      const int ci0 = (i - k * (COUT / 4)) * 4;
      const int tap = k / CIN;
      const int co = k - tap * CIN;
      uint2 v = {0u, 0u};
      if (tap < 9) {
        v = *reinterpret_cast<const uint2*>(w + (long long)co * WROW +
                                            (8 - tap) * COUT + ci0);
      }
      Bs[ci0 + 0][k] = (bf16raw)(v.x & 0xFFFFu);
      Bs[ci0 + 1][k] = (bf16raw)(v.x >> 16);
      Bs[ci0 + 2][k] = (bf16raw)(v.y & 0xFFFFu);
      Bs[ci0 + 3][k] = (bf16raw)(v.y >> 16);
    }
  }
  // the first barrier of the k-loop below orders these stores before any read

  const int a_row = tid >> 1;
  const int a_half = tid & 1;
  const int ntiles = (M + BM - 1) / BM;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * BM;
    const int gm = row0 + a_row;
    const bool row_live = gm < M;
    const int n_idx = gm / (HW * HW);
    const int rem = gm - n_idx * (HW * HW);
    const int ph = rem / HW;
    const int pw = rem - ph * HW;

    f32x4 acc[2][NFRAG];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < NFRAG; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

    // register prefetch: step s+1's global loads fly during step s's MFMAs
    uint4 ra0, ra1;

    auto load_step = [&](int s) {
      ra0 = uint4{0u, 0u, 0u, 0u};
      ra1 = uint4{0u, 0u, 0u, 0u};
      const int k0 = s * BK + a_half * 16;
      if constexpr (NU == 1) {
        const int tap = k0 / CIN;
        const int c0 = k0 - tap * CIN;
        const int hh = ph + tap / 3 - 1;
        const int ww = pw + tap % 3 - 1;
        if (row_live && tap < 9 && hh >= 0 && hh < HW && ww >= 0 && ww < HW) {
          const bf16raw* src =
              in + (((long long)n_idx * HW + hh) * HW + ww) * CIN + c0;
          ra0 = *reinterpret_cast<const uint4*>(src);
          ra1 = *reinterpret_cast<const uint4*>(src + 8);
        }
      } else {
        // CIN == 4: four taps of 4 channels (8 bytes) each
        uint2 u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int tap = k0 / CIN + j;
          const int hh = ph + tap / 3 - 1;
          const int ww = pw + tap % 3 - 1;
          u[j] = uint2{0u, 0u};
          if (row_live && tap < 9 && hh >= 0 && hh < HW && ww >= 0 &&
              ww < HW) {
            u[j] = *reinterpret_cast<const uint2*>(
                in + (((long long)n_idx * HW + hh) * HW + ww) * CIN);
          }
        }
        ra0 = uint4{u[0].x, u[0].y, u[1].x, u[1].y};
        ra1 = uint4{u[2].x, u[2].y, u[3].x, u[3].y};
      }
      if (relu_in) {
        ra0.x = drla_bf16x2_relu(ra0.x); ra0.y = drla_bf16x2_relu(ra0.y);
        ra0.z = drla_bf16x2_relu(ra0.z); ra0.w = drla_bf16x2_relu(ra0.w);
        ra1.x = drla_bf16x2_relu(ra1.x); ra1.y = drla_bf16x2_relu(ra1.y);
        ra1.z = drla_bf16x2_relu(ra1.z); ra1.w = drla_bf16x2_relu(ra1.w);
      }
    };

    load_step(0);
#pragma unroll 1
    for (int s = 0; s < NSTEPS; ++s) {
      *reinterpret_cast<uint4*>(&As[a_row][a_half * 16]) = ra0;
      *reinterpret_cast<uint4*>(&As[a_row][a_half * 16 + 8]) = ra1;
      __syncthreads();
      if (s + 1 < NSTEPS) load_step(s + 1);
      bf16x8 wf[NFRAG];
#pragma unroll
      for (int ni = 0; ni < NFRAG; ++ni) {
        wf[ni] = *reinterpret_cast<const bf16x8*>(
            &Bs[ni * 16 + (lane & 15)][s * BK + (lane >> 4) * 8]);
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(
            &As[wave * 32 + mi * 16 + (lane & 15)][(lane >> 4) * 8]);
#pragma unroll
        for (int ni = 0; ni < NFRAG; ++ni) {
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              wf[ni], xf, acc[mi][ni], 0, 0, 0);
        }
      }
      __syncthreads();
    }

    // ---- epilogue: lane holds channels c0..c0+3 of pixel gr ----
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int gr = row0 + wave * 32 + mi * 16 + (lane & 15);
      if (gr < M) {
#pragma unroll
        for (int ni = 0; ni < NFRAG; ++ni) {
          const int c0 = ni * 16 + (lane >> 4) * 4;
          const long long off = (long long)gr * COUT + c0;
          float v0 = acc[mi][ni][0] + BiasBuf[c0 + 0];
          float v1 = acc[mi][ni][1] + BiasBuf[c0 + 1];
          float v2 = acc[mi][ni][2] + BiasBuf[c0 + 2];
          float v3 = acc[mi][ni][3] + BiasBuf[c0 + 3];
          if (mask) {
            const uint2 mv = *reinterpret_cast<const uint2*>(mask + off);
            v0 *= (drla_bf16x2_lo(mv.x) > 0.0f) ? 1.0f : 0.0f;
            v1 *= (drla_bf16x2_hi(mv.x) > 0.0f) ? 1.0f : 0.0f;
            v2 *= (drla_bf16x2_lo(mv.y) > 0.0f) ? 1.0f : 0.0f;
            v3 *= (drla_bf16x2_hi(mv.y) > 0.0f) ? 1.0f : 0.0f;
          }
          if (res) {
            const uint2 rv = *reinterpret_cast<const uint2*>(res + off);
            v0 += drla_bf16x2_lo(rv.x);
            v1 += drla_bf16x2_hi(rv.x);
            v2 += drla_bf16x2_lo(rv.y);
            v3 += drla_bf16x2_hi(rv.y);
          }
          uint2 o;
          o.x = drla_f32x2_to_bf16x2(v0, v1);
          o.y = drla_f32x2_to_bf16x2(v2, v3);
          *reinterpret_cast<uint2*>(out + off) = o;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad + bias gradient
// ---------------------------------------------------------------------------

template <int CI, int CO, int HW>
__device__ void c3_wgrad_impl(const bf16raw* __restrict__ in,   // [M][CI]
                              const bf16raw* __restrict__ dy,   // [M][CO]
                              float* __restrict__ scratch,      // [K+1][CO]
                              int batch, int relu_in) {
  constexpr int K = 9 * CI;
  constexpr int KP = ((K + 1 + 15) / 16) * 16;  // + the ones column, padded
  constexpr int KT = KP / 16;                   // 16-wide k tiles
  constexpr int TPW = (KT + 3) / 4;             // k tiles per wave
  constexpr int NFRAG = CO / 16;
  constexpr int BKM = DRLA_CONV3_WGRAD_ROWS;    // m rows per chunk
  constexpr int APITCH = KP * 2 + 16;           // bytes; rows stay 16 B aligned
  constexpr int BPITCH = CO * 2 + 16;
  constexpr int EL = CI < 8 ? CI : 8;           // channels per staging unit
  constexpr int UPT = CI / EL;                  // units per tap
  constexpr int UPR = 9 * UPT;                  // units per row
  constexpr int BUPR = CO / 8;                  // dY 16-byte units per row
  static_assert(BKM == 64, "two 32-row MFMA k-steps per chunk");
  const int M = batch * HW * HW;

  __shared__ __attribute__((aligned(16))) unsigned char Am[BKM * APITCH];
  __shared__ __attribute__((aligned(16))) unsigned char Bm[BKM * BPITCH];

  const int tid = threadIdx.x;
  const int wave = tid / 64;
  const int lane = tid % 64;

  const int m_per_split = (M + gridDim.x - 1) / gridDim.x;
  const long long m_begin_ll = (long long)blockIdx.x * m_per_split;
  if (m_begin_ll >= M) return;  // block-uniform: an empty slice adds nothing
  const int m_begin = (int)m_begin_ll;
  const int m_end = min(M, m_begin + m_per_split);

  // columns K.. of the A tile never change: 1.0 at K (bias gradient), zeros
  // after it. dY rows past m_end are staged as zeros, so the ones need no
  // row mask.
  for (int i = tid; i < BKM * (KP - K); i += DRLA_CONV_BLOCK) {
    const int row = i / (KP - K);
    const int c = K + (i - row * (KP - K));
    *reinterpret_cast<bf16raw*>(&Am[row * APITCH + c * 2]) =
        (c == K) ? (bf16raw)0x3F80 : (bf16raw)0;
  }

  f32x4 acc[TPW][NFRAG];
#pragma unroll
  for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
    for (int ni = 0; ni < NFRAG; ++ni) acc[ti][ni] = {0.f, 0.f, 0.f, 0.f};

  // transposed-read base of this lane: row 8g + q, columns 4p..4p+3 of a tile
  const int tr_row = 8 * (lane >> 4) + ((lane >> 2) & 3);
  const int tr_col = 8 * (lane & 3);  // bytes

#pragma unroll 1
  for (int m0 = m_begin; m0 < m_end; m0 += BKM) {
    // ---- stage im2col(act) rows m0..m0+63, columns 0..K-1 ----
    for (int u = tid; u < BKM * UPR; u += DRLA_CONV_BLOCK) {
      const int row = u / UPR;
      const int r = u - row * UPR;
      const int tap = r / UPT;
      const int c0 = (r - tap * UPT) * EL;
      const int m = m0 + row;
      uint4 v = {0u, 0u, 0u, 0u};
      if (m < m_end) {
        const int n_idx = m / (HW * HW);
        const int rem = m - n_idx * (HW * HW);
        const int ph = rem / HW;
        const int hh = ph + tap / 3 - 1;
        const int ww = rem - ph * HW + tap % 3 - 1;
        if (hh >= 0 && hh < HW && ww >= 0 && ww < HW) {
          const bf16raw* src =
              in + (((long long)n_idx * HW + hh) * HW + ww) * CI + c0;
          if constexpr (EL == 8) {
            v = *reinterpret_cast<const uint4*>(src);
          } else {
            const uint2 t = *reinterpret_cast<const uint2*>(src);
            v.x = t.x;
            v.y = t.y;
          }
        }
      }
      if (relu_in) {
        v.x = drla_bf16x2_relu(v.x); v.y = drla_bf16x2_relu(v.y);
        v.z = drla_bf16x2_relu(v.z); v.w = drla_bf16x2_relu(v.w);
      }
      unsigned char* dst = &Am[row * APITCH + (tap * CI + c0) * 2];
      if constexpr (EL == 8) {
        *reinterpret_cast<uint4*>(dst) = v;
      } else {
        *reinterpret_cast<uint2*>(dst) = uint2{v.x, v.y};
      }
    }
    // ---- stage dY rows ----
    for (int u = tid; u < BKM * BUPR; u += DRLA_CONV_BLOCK) {
      const int row = u / BUPR;
      const int ch = u - row * BUPR;
      const int m = m0 + row;
      uint4 v = {0u, 0u, 0u, 0u};
      if (m < m_end) {
        v = *reinterpret_cast<const uint4*>(dy + (long long)m * CO + ch * 8);
      }
      *reinterpret_cast<uint4*>(&Bm[row * BPITCH + ch * 16]) = v;
    }
    __syncthreads();
    // uniform control flow from here to the barrier (transposed reads)
#pragma unroll
    for (int ks = 0; ks < BKM / 32; ++ks) {
      bf16x8 yf[NFRAG];
#pragma unroll
      for (int ni = 0; ni < NFRAG; ++ni) {
        yf[ni] = drla_lds_tr_frag(
            &Bm[(ks * 32 + tr_row) * BPITCH + ni * 32 + tr_col], BPITCH);
      }
#pragma unroll
      for (int ti = 0; ti < TPW; ++ti) {
        const int t = wave + 4 * ti;  // wave-uniform
        if (t < KT) {
          const bf16x8 af = drla_lds_tr_frag(
              &Am[(ks * 32 + tr_row) * APITCH + t * 32 + tr_col], APITCH);
#pragma unroll
          for (int ni = 0; ni < NFRAG; ++ni) {
            acc[ti][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af, yf[ni], acc[ti][ni], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  // D[k][co]: lane l, reg r -> k = 16 t + (l>>4)*4 + r, co = 16 ni + (l&15)
#pragma unroll
  for (int ti = 0; ti < TPW; ++ti) {
    const int t = wave + 4 * ti;
    if (t < KT) {
#pragma unroll
      for (int ni = 0; ni < NFRAG; ++ni) {
        const int co = ni * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = t * 16 + (lane >> 4) * 4 + r;
          if (k <= K) atomicAdd(&scratch[k * CO + co], acc[ti][ni][r]);
        }
      }
    }
  }
}

}  // namespace

// f32 scratch [K+1][CO] -> bf16 dW [CO][K] and dbias [CO] (row K), re-zeroing
// the scratch as it reads: every wgrad call leaves it zero for the next
// layer, which shares it.
extern "C" __global__ void drla_c3_wgrad_finalize(
    float* __restrict__ scratch, bf16raw* __restrict__ dw,
    bf16raw* __restrict__ dbias, int K, int CO) {
  const int total = (K + 1) * CO;
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    if (i < K * CO) {
      const int co = i / K;
      const int k = i - co * K;
      const int si = k * CO + co;
      dw[i] = drla_f32_to_bf16(scratch[si]);
      scratch[si] = 0.0f;
    } else {
      dbias[i - K * CO] = drla_f32_to_bf16(scratch[i]);
      scratch[i] = 0.0f;
    }
  }
}

#define C3_G(l) \
  DRLA_CONV3_LAYERS[l].ci, DRLA_CONV3_LAYERS[l].co, DRLA_CONV3_LAYERS[l].hw
// dgrad of geometry l: channel roles swapped
#define C3_GT(l) \
  DRLA_CONV3_LAYERS[l].co, DRLA_CONV3_LAYERS[l].ci, DRLA_CONV3_LAYERS[l].hw

// one kernel per geometry and role, named <role>_<ci>_<co>_<h> of the conv;
// order = DRLA_CONV3_LAYERS. The first layer needs no dgrad.

CONV_KERNEL drla_c3_fwd_4_16_84(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias,
    const bf16raw* mask, const bf16raw* res, bf16raw* out, int batch,
    int relu_in) {
  c3_gemm_impl<C3_G(0), false>(in, w, bias, mask, res, out, batch, relu_in);
}

CONV_KERNEL drla_c3_fwd_16_16_42(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias,
    const bf16raw* mask, const bf16raw* res, bf16raw* out, int batch,
    int relu_in) {
  c3_gemm_impl<C3_G(1), false>(in, w, bias, mask, res, out, batch, relu_in);
}

CONV_KERNEL drla_c3_fwd_16_32_42(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias,
    const bf16raw* mask, const bf16raw* res, bf16raw* out, int batch,
    int relu_in) {
  c3_gemm_impl<C3_G(2), false>(in, w, bias, mask, res, out, batch, relu_in);
}

CONV_KERNEL drla_c3_fwd_32_32_21(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias,
    const bf16raw* mask, const bf16raw* res, bf16raw* out, int batch,
    int relu_in) {
  c3_gemm_impl<C3_G(3), false>(in, w, bias, mask, res, out, batch, relu_in);
}

CONV_KERNEL drla_c3_fwd_32_32_11(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias,
    const bf16raw* mask, const bf16raw* res, bf16raw* out, int batch,
    int relu_in) {
  c3_gemm_impl<C3_G(4), false>(in, w, bias, mask, res, out, batch, relu_in);
}

CONV_KERNEL drla_c3_dgrad_16_16_42(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias,
    const bf16raw* mask, const bf16raw* res, bf16raw* out, int batch,
    int relu_in) {
  c3_gemm_impl<C3_GT(1), true>(in, w, bias, mask, res, out, batch, relu_in);
}

CONV_KERNEL drla_c3_dgrad_16_32_42(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias,
    const bf16raw* mask, const bf16raw* res, bf16raw* out, int batch,
    int relu_in) {
  c3_gemm_impl<C3_GT(2), true>(in, w, bias, mask, res, out, batch, relu_in);
}

CONV_KERNEL drla_c3_dgrad_32_32_21(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias,
    const bf16raw* mask, const bf16raw* res, bf16raw* out, int batch,
    int relu_in) {
  c3_gemm_impl<C3_GT(3), true>(in, w, bias, mask, res, out, batch, relu_in);
}

CONV_KERNEL drla_c3_dgrad_32_32_11(
    const bf16raw* in, const bf16raw* w, const bf16raw* bias,
    const bf16raw* mask, const bf16raw* res, bf16raw* out, int batch,
    int relu_in) {
  c3_gemm_impl<C3_GT(4), true>(in, w, bias, mask, res, out, batch, relu_in);
}

CONV_KERNEL drla_c3_wgrad_4_16_84(
    const bf16raw* in, const bf16raw* dy, float* scratch, int batch,
    int relu_in) {
  c3_wgrad_impl<C3_G(0)>(in, dy, scratch, batch, relu_in);
}

CONV_KERNEL drla_c3_wgrad_16_16_42(
    const bf16raw* in, const bf16raw* dy, float* scratch, int batch,
    int relu_in) {
  c3_wgrad_impl<C3_G(1)>(in, dy, scratch, batch, relu_in);
}

CONV_KERNEL drla_c3_wgrad_16_32_42(
    const bf16raw* in, const bf16raw* dy, float* scratch, int batch,
    int relu_in) {
  c3_wgrad_impl<C3_G(2)>(in, dy, scratch, batch, relu_in);
}

CONV_KERNEL drla_c3_wgrad_32_32_21(
    const bf16raw* in, const bf16raw* dy, float* scratch, int batch,
    int relu_in) {
  c3_wgrad_impl<C3_G(3)>(in, dy, scratch, batch, relu_in);
}

CONV_KERNEL drla_c3_wgrad_32_32_11(
    const bf16raw* in, const bf16raw* dy, float* scratch, int batch,
    int relu_in) {
  c3_wgrad_impl<C3_G(4)>(in, dy, scratch, batch, relu_in);
}
