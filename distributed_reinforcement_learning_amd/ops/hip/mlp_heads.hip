// K4 fused: BOTH IMPALA heads — policy (256->256->256->A)
// and value (256->256->256->1) — in ONE kernel each way.
//
// The heads are tiny (M = B*T = 640 rows, K = 256): every torch layer is a
// latency-bound ~5 us launch, and fwd+bwd spend ~200 us/step in ~30 small
// kernels (profiles r17). Rows are independent, so one block walks its 32
// rows through all six layers.
//
// Formulation: TRANSPOSED OUTPUT (D[out][row]) so both MFMA operands are
// vector loads —
//   A_op[m=out][k] = W[out][k]  (torch [out,in] rows, straight from global:
//                                each W element is used once per block, so
//                                LDS staging buys nothing — guide §5 "GEMV /
//                                decode weights" row)
//   B_op[k][col=row] = act[row][k]  (row-major LDS act image, vec8)
// The epilogue un-transposes with scalar LDS writes (once per layer, not
// per k-chunk). The backward dgrad chain uses the same shape on
// Pre-TRANSPOSED weights (built by the autograd wrapper: 4 small .t()
// copies), fusing ReLU masks and bias gradients; only the six
// MFMA-efficient wgrad GEMMs stay on hipBLASLt.

#include "drla_kernels.h"

// MH_HID (hidden width) and MH_BM (rows per block) are in drla_common.h:
// the launch grids are computed from them
#define MH_PAD 8
#define MH_LD (MH_HID + MH_PAD)

// One dense pass: out[r][o] = in[r][:] . M[o][:] (+bias, ReLU / mask),
// M [nout][kdim] row-major global, kdim = KCH * 32; rows of M at or beyond
// nout are never read. act images [MH_BM][MH_LD] bf16.
// Precondition: N >= 1 and nout >= 1. Row and column indices past the end
// are clamped to N - 1 / nout - 1 for the load and the value dropped
// afterwards; the launchers never launch an empty grid.
//
// A pass is three steps so that its callers can place the loads:
//   mh_load      request ALL of a wave's A fragments of the pass (KCH chunks
//                x 4 sixteen-row operands, 4 VGPRs each: 128 VGPRs at
//                kdim 256). These kernels run 40-80 workgroups, one per CU at
//                most, and the weights are cold in every XCD's L2 (the
//                optimizer has just rewritten them, the W^T pack comes from
//                other workgroups): with the chunks requested one ahead, each
//                of the 8 chunks paid a full miss before its four MFMAs. In
//                flight together, a pass pays one. The weights do not depend
//                on the activations, so a chained kernel requests the later
//                passes' fragments before the first pass's MFMAs as well.
//                The loads are unconditional (a row index past nout is
//                clamped and the operand zeroed in mh_mma), so nothing
//                branches between them
//   mh_load_bias / mh_load_mask
//                the 16 values per lane the epilogue adds or masks with,
//                requested with the weights: read in the epilogue, each was
//                a dependent 2-byte load with its own wait
//   mh_mma       the MFMAs: k ascending, ni 0..3 per chunk
//   mh_epilogue  un-transpose, bias / ReLU / mask, side outputs
//
// SIDE == MH_MASK: v *= (stash > 0), dz-global write + colsum bias partials
// (backward layers). SIDE == MH_BIAS: v += bias, RELU applies (forward
// layers). DH != null: terminal f32 row-grad output, added atomically.
template <int KCH>
struct MhFrags {
  bf16x8 a[KCH][4];
};

struct MhSide {
  bf16raw v[4][4];  // [ni][r], the epilogue's (ni, r) walk
};

enum { MH_NONE = 0, MH_BIAS = 1, MH_MASK = 2 };

// this wave's 64 output columns start here (wave-uniform, and known to be)
__device__ __forceinline__ int mh_out0() {
  return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * 64;
}

template <int KCH>
__device__ __forceinline__ void mh_load(MhFrags<KCH>& f,
                                        const bf16raw* __restrict__ M,
                                        int nout) {
  const int lane = threadIdx.x % 64;
  const int out0 = mh_out0();
  const int kf = (lane >> 4) * 8;
  if (out0 < nout) {
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int orow = min(out0 + ni * 16 + (lane & 15), nout - 1);
        f.a[kc][ni] = *reinterpret_cast<const bf16x8*>(
            M + (long long)orow * (KCH * 32) + kc * 32 + kf);
      }
    }
  }
}

__device__ __forceinline__ void mh_load_bias(MhSide& s,
                                             const bf16raw* __restrict__ bias,
                                             int nout) {
  const int lane = threadIdx.x % 64;
  const int out0 = mh_out0();
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int oc = out0 + ni * 16 + (lane >> 4) * 4 + r;
      s.v[ni][r] = bias[min(oc, nout - 1)];
    }
  }
}

// mask_stash [N, MH_HID]; the masked passes all have nout == MH_HID
__device__ __forceinline__ void mh_load_mask(
    MhSide& s, const bf16raw* __restrict__ mask_stash, int row0, int N) {
  const int lane = threadIdx.x % 64;
  const int out0 = mh_out0();
  const long long grow = min(row0 + (lane & 15), N - 1);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int oc = out0 + ni * 16 + (lane >> 4) * 4 + r;
      s.v[ni][r] = mask_stash[grow * MH_HID + oc];
    }
  }
}

template <int KCH>
__device__ __forceinline__ void mh_mma(f32x4 (&acc)[4],
                                       const MhFrags<KCH>& f,
                                       const bf16raw (*act_in)[MH_LD],
                                       int nout) {
  const int lane = threadIdx.x % 64;
  const int out0 = mh_out0();
  const int kf = (lane >> 4) * 8;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};
  if (out0 < nout) {
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc) {
      const bf16x8 b_frag = *reinterpret_cast<const bf16x8*>(
          &act_in[lane & 15][kc * 32 + kf]);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int orow = out0 + ni * 16 + (lane & 15);
        const bf16x8 a_frag =
            (nout == MH_HID || orow < nout) ? f.a[kc][ni] : zero8;
        acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag, b_frag, acc[ni], 0, 0, 0);
      }
    }
  }
}

template <bool RELU, int SIDE>
__device__ __forceinline__ void mh_epilogue(
    const f32x4 (&acc)[4], bf16raw (*act_out)[MH_LD],
    const MhSide& side,                      // bias or mask values, per SIDE
    bf16raw* __restrict__ dz_global,         // [N,256]
    float* __restrict__ colsum,              // [256]
    bf16raw* __restrict__ stash,             // [N,nout] or null
    float* __restrict__ dh_global,           // [N,256] or null
    int row0, int N, int nout) {
  const int lane = threadIdx.x % 64;
  const int out0 = mh_out0();
  const bool live = out0 < nout;
  __syncthreads();
  // epilogue: D[out][row] un-transpose -> act_out[row][out] (+stash/dz/dh);
  // per (ni, r) the lane touches ONE output column across its two rows, so
  // bias partials need one LDS atomic per (ni, r).
  if (live) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oc = out0 + ni * 16 + (lane >> 4) * 4 + r;
        const int lrow = lane & 15;
        const int grow = row0 + lrow;
        float v = acc[ni][r];
        if (SIDE == MH_BIAS) {
          v += (oc < nout) ? drla_bf16_to_f32(side.v[ni][r]) : 0.0f;
        }
        if (RELU) v = fmaxf(v, 0.0f);
        if (SIDE == MH_MASK) {
          const float a = (grow < N) ? drla_bf16_to_f32(side.v[ni][r]) : 0.0f;
          v = (a > 0.0f) ? v : 0.0f;
        }
        if (dh_global) {
          // both head chains land here concurrently (blockIdx.y split):
          // accumulate atomically into the zeroed dh buffer
          if (grow < N && oc < nout) {
            atomicAdd(&dh_global[(long long)grow * MH_HID + oc], v);
          }
        } else {
          const bf16raw bv = drla_f32_to_bf16(v);
          act_out[lrow][oc] = bv;
          if (stash && grow < N && oc < nout) {
            stash[(long long)grow * nout + oc] = bv;
          }
          if (dz_global && grow < N && oc < nout) {
            dz_global[(long long)grow * MH_HID + oc] = bv;
          }
          if (colsum && oc < nout && grow < N) {
            atomicAdd(&colsum[oc], v);
          }
        }
      }
    }
  }
  __syncthreads();
}

// Transposed-weight side output of the forward kernels: the backward dgrad
// chains want W^T, and the weights do not change between a step's forward
// and backward, so the forward (which streams every W anyway) emits it and
// the separate pack launch disappears. One "unit" is 8 consecutive k of one
// W row: a 16 B load, then 8 stores that are coalesced across the lanes
// (consecutive lanes = consecutive rows r = consecutive out columns).
// Units u in [0, 8192) cover one [256,256] matrix exactly once.
__device__ __forceinline__ void mh_wt_unit(const bf16raw* __restrict__ w,
                                           bf16raw* __restrict__ out,
                                           int u) {
  const int r = u & 255;
  const int k0 = (u >> 8) * 8;
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(w + r * 256 + k0);
#pragma unroll
  for (int j = 0; j < 8; ++j) out[(k0 + j) * 256 + r] = (bf16raw)v[j];
}

// wt_pack != null: additionally write the packed transposed weights in the
// drla_heads_wt_pack layout (below), each block its own share (thread gt of
// nt strides over the units, so no element is written twice).
// ws != null: zero the backward's f32 workspace ([N,256] dh ++ 4*256+A+1
// bias partials) — policy block x its own 16 dh rows, block (0,0) the tail —
// so the backward needs no fill launch in front of its atomics.
extern "C" __global__ __launch_bounds__(256) void drla_mlp_heads_fwd(
    const float* __restrict__ h,        // [N,256]
    const bf16raw* __restrict__ W1p, const bf16raw* __restrict__ b1p,
    const bf16raw* __restrict__ W2p, const bf16raw* __restrict__ b2p,
    const bf16raw* __restrict__ W3p, const bf16raw* __restrict__ b3p,
    const bf16raw* __restrict__ W1v, const bf16raw* __restrict__ b1v,
    const bf16raw* __restrict__ W2v, const bf16raw* __restrict__ b2v,
    const bf16raw* __restrict__ W3v, const bf16raw* __restrict__ b3v,
    bf16raw* __restrict__ logits,       // [N,A]
    float* __restrict__ value,          // [N]
    bf16raw* __restrict__ stash,    // [N,5*256]: a1p,a2p,a1v,a2v,h_bf16
    int N, int A,
    bf16raw* __restrict__ wt_pack,  // [270592] (nullable)
    float* __restrict__ ws) {       // [N*256 + 4*256 + A + 1] (nullable)
  // grid: (ceil(N/16), 2) — blockIdx.y 0 = policy chain, 1 = value chain
  __shared__ bf16raw hb[MH_BM][MH_LD];
  __shared__ bf16raw acta[MH_BM][MH_LD];
  __shared__ bf16raw actb[MH_BM][MH_LD];

  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * MH_BM;
  const bool policy = blockIdx.y == 0;
  const long long soff = (long long)N * MH_HID;

  // the chain's operands; both chains run the same three passes
  const bf16raw* W1 = policy ? W1p : W1v;
  const bf16raw* W2 = policy ? W2p : W2v;
  const bf16raw* W3 = policy ? W3p : W3v;
  const bf16raw* b1 = policy ? b1p : b1v;
  const bf16raw* b2 = policy ? b2p : b2v;
  const bf16raw* b3 = policy ? b3p : b3v;
  const int n3 = policy ? A : 1;
  bf16raw* stash1 = stash + (policy ? 0 : 2 * soff);
  bf16raw* stash2 = stash1 + soff;

  // layers 1 and 2 entirely in flight before anything else happens (256
  // VGPRs of fragments; one workgroup per CU, so they are there to use)
  MhFrags<MH_HID / 32> fa, fb;
  MhSide s1, s2, s3;
  mh_load(fa, W1, MH_HID);
  mh_load_bias(s1, b1, MH_HID);
  mh_load(fb, W2, MH_HID);
  mh_load_bias(s2, b2, MH_HID);
  mh_load_bias(s3, b3, n3);

  if (wt_pack) {
    const int gt = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid;
    const int nt = gridDim.x * gridDim.y * 256;
    // four [256,256] transposes: wT1p@0, wT2p@65536, wT1v@139264,
    // wT2v@204800
    for (int u = gt; u < 4 * 8192; u += nt) {
      const int m = u >> 13;
      const bf16raw* w = (m == 0) ? W1p : (m == 1) ? W2p
                       : (m == 2) ? W1v : W2v;
      const int off = (m == 0) ? 0 : (m == 1) ? 65536
                    : (m == 2) ? 139264 : 204800;
      mh_wt_unit(w, wt_pack + off, u & 8191);
    }
    // wT3p [256,32] @131072 (cols >= A zero), W3v copy @270336
    for (int e = gt; e < 8192 + 256; e += nt) {
      if (e < 8192) {
        const int c = e & 31;
        wt_pack[131072 + e] =
            (c < A) ? W3p[c * 256 + (e >> 5)] : (bf16raw)0;
      } else {
        wt_pack[270336 + (e - 8192)] = W3v[e - 8192];
      }
    }
  }
  if (ws && policy) {
    const int r = tid >> 4;
    const int c0 = (tid & 15) * 16;
    const int grow = row0 + r;
    if (grow < N) {
      float4* p = reinterpret_cast<float4*>(
          ws + (long long)grow * MH_HID + c0);
      const float4 z4 = {0.f, 0.f, 0.f, 0.f};
      p[0] = z4; p[1] = z4; p[2] = z4; p[3] = z4;
    }
    if (blockIdx.x == 0) {
      const int tail = 4 * MH_HID + A + 1;
      for (int i = tid; i < tail; i += 256) ws[soff + i] = 0.0f;
    }
  }

  // load h (f32 -> bf16); the policy block stashes the bf16 copy
  {
    const int r = tid >> 4;
    const int c0 = (tid & 15) * 16;
    const int grow = row0 + r;
    // all 16 requested before the first is used (a load inside the store
    // loop below waits for itself every time round)
    // (and unconditionally, from a clamped row: a predicated load is a
    // branch, and the wait comes back with it)
    float hv[16];
    const long long crow = min(grow, N - 1);
#pragma unroll
    for (int c = 0; c < 16; ++c) hv[c] = h[crow * MH_HID + c0 + c];
#pragma unroll
    for (int c = 0; c < 16; ++c) hv[c] = (grow < N) ? hv[c] : 0.0f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const bf16raw bv = drla_f32_to_bf16(hv[c]);
      hb[r][c0 + c] = bv;
      if (policy && grow < N) {
        stash[4 * soff + (long long)grow * MH_HID + c0 + c] = bv;
      }
    }
  }
  __syncthreads();

  f32x4 acc[4];
  mh_mma(acc, fa, hb, MH_HID);
  // layer 3 takes layer 1's registers as soon as its MFMAs have them
  mh_load(fa, W3, n3);
  mh_epilogue<true, MH_BIAS>(acc, acta, s1, nullptr, nullptr, stash1,
                             nullptr, row0, N, MH_HID);
  mh_mma(acc, fb, acta, MH_HID);
  mh_epilogue<true, MH_BIAS>(acc, actb, s2, nullptr, nullptr, stash2,
                             nullptr, row0, N, MH_HID);
  mh_mma(acc, fa, actb, n3);
  mh_epilogue<false, MH_BIAS>(acc, acta, s3, nullptr, nullptr, nullptr,
                              nullptr, row0, N, n3);
  if (policy) {
    const int r = tid >> 3;
    const int c = tid & 7;
    if (r < MH_BM) {
      for (int cc = c; cc < A; cc += 8) {
        if (row0 + r < N) {
          logits[(long long)(row0 + r) * A + cc] = acta[r][cc];
        }
      }
    }
  } else {
    if (tid < MH_BM && row0 + tid < N) {
      value[row0 + tid] = drla_bf16_to_f32(acta[tid][0]);
    }
  }
}

// The one-chunk-ahead form of the same pass in one function:
// drla_mlp_heads_bwd keeps it, since requesting its chains' operands whole
// buys that kernel nothing (KERNELS.md) and costs it a full register file.
// Only the k-loop differs: the next chunk's fragments load while this
// chunk's MFMAs run; the side values are requested behind the loop and the
// epilogue is the shared one. M [nout][kdim] row-major, kdim a multiple of
// 32; side_src: mask_stash [N,256] (MH_MASK), bias [nout] (MH_BIAS) or
// unused (MH_NONE).
template <bool RELU, int SIDE>
__device__ void mh_pass(const bf16raw (*act_in)[MH_LD],
                        bf16raw (*act_out)[MH_LD],
                        const bf16raw* __restrict__ M,   // [nout][kdim]
                        const bf16raw* __restrict__ side_src,
                        bf16raw* __restrict__ dz_global,         // [N,256]
                        float* __restrict__ colsum,              // [256]
                        bf16raw* __restrict__ stash,     // [N,nout] or null
                        float* __restrict__ dh_global,   // [N,256] or null
                        int row0, int N, int nout, int kdim) {
  const int lane = threadIdx.x % 64;
  const int out0 = mh_out0();

  f32x4 acc[4];
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};

  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  if (out0 < nout) {
    bf16x8 a_cur0, a_cur1, a_cur2, a_cur3;
    const int kf = (lane >> 4) * 8;
#define DRLA_MH_LOAD(ni, dst, k0)                                       \
    {                                                                   \
      const int orow = out0 + (ni) * 16 + (lane & 15);                  \
      dst = (orow < nout)                                               \
          ? *reinterpret_cast<const bf16x8*>(                           \
                M + (long long)orow * kdim + (k0) + kf)                 \
          : zero8;                                                      \
    }
    DRLA_MH_LOAD(0, a_cur0, 0); DRLA_MH_LOAD(1, a_cur1, 0);
    DRLA_MH_LOAD(2, a_cur2, 0); DRLA_MH_LOAD(3, a_cur3, 0);
    for (int k0 = 0; k0 < kdim; k0 += 32) {
      bf16x8 a_nxt0, a_nxt1, a_nxt2, a_nxt3;
      if (k0 + 32 < kdim) {
        DRLA_MH_LOAD(0, a_nxt0, k0 + 32); DRLA_MH_LOAD(1, a_nxt1, k0 + 32);
        DRLA_MH_LOAD(2, a_nxt2, k0 + 32); DRLA_MH_LOAD(3, a_nxt3, k0 + 32);
      }
      const bf16x8 b_frag =
          *reinterpret_cast<const bf16x8*>(&act_in[lane & 15][k0 + kf]);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_cur0, b_frag,
                                                       acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_cur1, b_frag,
                                                       acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_cur2, b_frag,
                                                       acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_cur3, b_frag,
                                                       acc[3], 0, 0, 0);
      a_cur0 = a_nxt0; a_cur1 = a_nxt1; a_cur2 = a_nxt2; a_cur3 = a_nxt3;
    }
#undef DRLA_MH_LOAD
  }
  MhSide side;
  if (SIDE == MH_MASK) mh_load_mask(side, side_src, row0, N);
  if (SIDE == MH_BIAS) mh_load_bias(side, side_src, nout);
  mh_epilogue<RELU, SIDE>(acc, act_out, side, dz_global, colsum, stash,
                          dh_global, row0, N, nout);
}

// backward: takes PRE-TRANSPOSED weights (wrapper-built):
//   wT3p [256,32] = pad(W3p^T), wT2p/wT1p/wT2v/wT1v [256,256] = W^T,
//   W3v [1,256] as-is (value out layer backward is an outer product).
extern "C" __global__ __launch_bounds__(256) void drla_mlp_heads_bwd(
    const bf16raw* __restrict__ dlogits,   // [N,A]
    const float* __restrict__ dvalue,      // [N]
    const bf16raw* __restrict__ stash,     // [N,5*256]
    const bf16raw* __restrict__ wT1p, const bf16raw* __restrict__ wT2p,
    const bf16raw* __restrict__ wT3p,      // [256,32] padded
    const bf16raw* __restrict__ wT1v, const bf16raw* __restrict__ wT2v,
    const bf16raw* __restrict__ W3v,       // [1,256]
    bf16raw* __restrict__ dz1p, bf16raw* __restrict__ dz2p,  // [N,256]
    bf16raw* __restrict__ dz1v, bf16raw* __restrict__ dz2v,  // [N,256]
    float* __restrict__ dh,                // [N,256], ZEROED (atomics)
    float* __restrict__ db1p, float* __restrict__ db2p,
    float* __restrict__ db3p,              // [A]
    float* __restrict__ db1v, float* __restrict__ db2v,
    float* __restrict__ db3v,              // [1]
    int N, int A) {
  // grid: (ceil(N/16), 2) — blockIdx.y 0 = policy chain, 1 = value chain;
  // both accumulate dh atomically.
  __shared__ bf16raw dza[MH_BM][MH_LD];
  __shared__ bf16raw dzb[MH_BM][MH_LD];
  __shared__ float colsum[MH_HID];

  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * MH_BM;
  const long long soff = (long long)N * MH_HID;
  const bf16raw* a1p = stash;
  const bf16raw* a2p = stash + soff;
  const bf16raw* a1v = stash + 2 * soff;
  const bf16raw* a2v = stash + 3 * soff;

  if (tid < MH_HID) colsum[tid] = 0.0f;

  if (blockIdx.y == 0) {
    // ---- policy chain ----
    {
      const int r = tid >> 4;
      const int c = tid & 15;
      for (int cc = c; cc < 32; cc += 16) {
        const int grow = row0 + r;
        bf16raw v = 0;
        if (cc < A && grow < N) v = dlogits[(long long)grow * A + cc];
        dza[r][cc] = v;
      }
    }
    __syncthreads();
    if (tid < A) {
      float s = 0.0f;
      for (int r = 0; r < MH_BM; ++r) {
        if (row0 + r < N) s += drla_bf16_to_f32(dza[r][tid]);
      }
      atomicAdd(&db3p[tid], s);
    }
    __syncthreads();
    mh_pass<false, MH_MASK>(dza, dzb, wT3p, a2p, dz2p, colsum, nullptr,
                            nullptr, row0, N, MH_HID, 32);
    if (tid < MH_HID) {
      atomicAdd(&db2p[tid], colsum[tid]);
      colsum[tid] = 0.0f;
    }
    __syncthreads();
    mh_pass<false, MH_MASK>(dzb, dza, wT2p, a1p, dz1p, colsum, nullptr,
                            nullptr, row0, N, MH_HID, MH_HID);
    if (tid < MH_HID) atomicAdd(&db1p[tid], colsum[tid]);
    __syncthreads();
    mh_pass<false, MH_NONE>(dza, dzb, wT1p, nullptr, nullptr, nullptr,
                            nullptr, dh, row0, N, MH_HID, MH_HID);
  } else {
    // ---- value chain ----
    // da2v[r][i] = dvalue[r] * W3v[i], masked by a2v
    {
      const int r = tid >> 4;
      const int c0 = (tid & 15) * 16;
      const int grow = row0 + r;
      const float dv = (grow < N) ? dvalue[grow] : 0.0f;
      for (int c = 0; c < 16; ++c) {
        const int ic = c0 + c;
        float v = dv * drla_bf16_to_f32(W3v[ic]);
        if (grow < N) {
          const float a = drla_bf16_to_f32(a2v[(long long)grow * MH_HID + ic]);
          v = (a > 0.0f) ? v : 0.0f;
        } else {
          v = 0.0f;
        }
        const bf16raw bv = drla_f32_to_bf16(v);
        dza[r][ic] = bv;
        if (grow < N) dz2v[(long long)grow * MH_HID + ic] = bv;
        atomicAdd(&colsum[ic], v);
      }
    }
    __syncthreads();
    if (tid < MH_HID) {
      atomicAdd(&db2v[tid], colsum[tid]);
      colsum[tid] = 0.0f;
    }
    if (tid == 0) {
      float s = 0.0f;
      for (int r = 0; r < MH_BM && row0 + r < N; ++r) s += dvalue[row0 + r];
      atomicAdd(&db3v[0], s);
    }
    __syncthreads();
    mh_pass<false, MH_MASK>(dza, dzb, wT2v, a1v, dz1v, colsum, nullptr,
                            nullptr, row0, N, MH_HID, MH_HID);
    if (tid < MH_HID) atomicAdd(&db1v[tid], colsum[tid]);
    __syncthreads();
    mh_pass<false, MH_NONE>(dzb, dza, wT1v, nullptr, nullptr, nullptr,
                            nullptr, dh, row0, N, MH_HID, MH_HID);
  }
}

// ---------------------------------------------------------------------------
// Weight-transpose pack: the dgrad kernel above wants W^T operands, which
// the wrapper used to build with 5 .t().contiguous() copies + an F.pad —
// ~7 eager launches per step at the ~4.5 us small-kernel floor (profile
// r23). One kernel writes the whole packed buffer instead.
// Layout (bf16 elements): wT1p@0, wT2p@65536, wT3p@131072 ([256,32],
// cols >= A zero), wT1v@139264, wT2v@204800, W3v copy @270336; total 270592.
extern "C" __global__ void drla_heads_wt_pack(
    const bf16raw* __restrict__ w1p, const bf16raw* __restrict__ w2p,
    const bf16raw* __restrict__ w3p, const bf16raw* __restrict__ w1v,
    const bf16raw* __restrict__ w2v, const bf16raw* __restrict__ w3v,
    bf16raw* __restrict__ out, int A) {
  const int total = 4 * 65536 + 256 * 32 + 256;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    bf16raw v;
    if (i < 65536) {
      v = w1p[(i & 255) * 256 + (i >> 8)];
    } else if (i < 131072) {
      const int j = i - 65536;
      v = w2p[(j & 255) * 256 + (j >> 8)];
    } else if (i < 139264) {
      const int j = i - 131072;
      const int c = j & 31;
      v = (c < A) ? w3p[c * 256 + (j >> 5)] : (bf16raw)0;
    } else if (i < 204800) {
      const int j = i - 139264;
      v = w1v[(j & 255) * 256 + (j >> 8)];
    } else if (i < 270336) {
      const int j = i - 204800;
      v = w2v[(j & 255) * 256 + (j >> 8)];
    } else {
      v = w3v[i - 270336];
    }
    out[i] = v;
  }
}

// ---------------------------------------------------------------------------
// All six head wgrads in ONE launch: dW = dz^T @ act with K = N rows.
// Replaces 6 hipBLASLt GEMM dispatches (~5/step at ~13 us each, r23).
//
// Jobs (all outputs [M,256] bf16):
//   0: dW1p = dz1p^T @ hb     M=256      3: dW2v = dz2v^T @ a1v  M=256
//   1: dW2p = dz2p^T @ a1p    M=256      4: dW3p = dlogits^T @ a2p  M=A
//   2: dW1v = dz1v^T @ hb     M=256      5: dW3v = dvalue^T @ a2v   M=1
//
// Both MFMA operands are k-major in global (dz[k][m], act[k][n]), so each
// 32k-chunk is staged TRANSPOSED into padded LDS (vec8 global row loads,
// scalar LDS writes) and the fragments read back as vec8 ds_read_b128
// (row stride 40 elems = 80 B keeps 16 B alignment).
#define HW_LDK 40  // 32 + 8 pad

extern "C" __global__ __launch_bounds__(256) void drla_heads_wgrad(
    const bf16raw* __restrict__ dz1p, const bf16raw* __restrict__ dz2p,
    const bf16raw* __restrict__ dz1v, const bf16raw* __restrict__ dz2v,
    const bf16raw* __restrict__ dlogits,  // [N,A]
    const float* __restrict__ dvalue,     // [N]
    const bf16raw* __restrict__ stash,    // [N,5*256]
    bf16raw* __restrict__ dw1p, bf16raw* __restrict__ dw2p,
    bf16raw* __restrict__ dw3p,           // [A,256]
    bf16raw* __restrict__ dw1v, bf16raw* __restrict__ dw2v,
    bf16raw* __restrict__ dw3v,           // [1,256]
    const float* __restrict__ ws_tail,    // f32 bias partials from heads_bwd
    bf16raw* __restrict__ db1p, bf16raw* __restrict__ db2p,
    bf16raw* __restrict__ db3p, bf16raw* __restrict__ db1v,
    bf16raw* __restrict__ db2v, bf16raw* __restrict__ db3v,
    int N, int A) {
  // grid.x = 73: jobs 0-3 are 4x4 tiles of 64x64 (blocks 0..63), job 4 is
  // blocks 64..67 (one m-tile, A <= 32), job 5 blocks 68..71; block 72
  // converts the f32 bias-grad partials to six contiguous bf16 tensors
  // (contiguous outputs avoid AccumulateGrad's clone-a-view kernels).
  const int bid = blockIdx.x;
  if (bid == 72) {
    const int tid = threadIdx.x;
    const int total = 4 * 256 + A + 1;
    for (int i = tid; i < total; i += 256) {
      const bf16raw v = drla_f32_to_bf16(ws_tail[i]);
      if (i < 256)            db1p[i] = v;
      else if (i < 512)       db2p[i - 256] = v;
      else if (i < 512 + A)   db3p[i - 512] = v;
      else if (i < 768 + A)   db1v[i - 512 - A] = v;
      else if (i < 1024 + A)  db2v[i - 768 - A] = v;
      else                    db3v[0] = v;
    }
    return;
  }
  int job, mt, nt;
  if (bid < 64) {
    job = bid >> 4;
    mt = (bid >> 2) & 3;
    nt = bid & 3;
  } else if (bid < 68) {
    job = 4; mt = 0; nt = bid - 64;
  } else {
    job = 5; mt = 0; nt = bid - 68;
  }
  const long long soff = (long long)N * MH_HID;
  const bf16raw* dz;
  const bf16raw* act;
  bf16raw* out;
  int M;
  switch (job) {
    case 0: dz = dz1p; act = stash + 4 * soff; out = dw1p; M = 256; break;
    case 1: dz = dz2p; act = stash;            out = dw2p; M = 256; break;
    case 2: dz = dz1v; act = stash + 4 * soff; out = dw1v; M = 256; break;
    case 3: dz = dz2v; act = stash + 2 * soff; out = dw2v; M = 256; break;
    case 4: dz = dlogits; act = stash + soff;  out = dw3p; M = A;   break;
    default: dz = nullptr; act = stash + 3 * soff; out = dw3v; M = 1;
  }
  const int m0 = mt * 64;
  const int n0 = nt * 64;

  __shared__ bf16raw dzT[64][HW_LDK];   // [m_local][k_local]
  __shared__ bf16raw actT[64][HW_LDK];  // [n_local][k_local]

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;

  f32x4 acc[4];
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};

  // software-pipelined K(=N)-loop: next chunk's globals prefetch into
  // registers during this chunk's MFMA (same pattern as the conv wgrad)
  const int st_kk = tid >> 3;
  const int st_c0 = (tid & 7) * 8;
  const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 r_act = z8, r_dz = z8;

  auto load_chunk = [&](int k0) {
    const int k = k0 + st_kk;
    r_act = z8;
    if (k < N) {
      r_act = *reinterpret_cast<const bf16x8*>(
          act + (long long)k * MH_HID + n0 + st_c0);
    }
    if (job < 4) {           // dz [N,256] bf16, vec8
      r_dz = z8;
      if (k < N) {
        r_dz = *reinterpret_cast<const bf16x8*>(
            dz + (long long)k * MH_HID + m0 + st_c0);
      }
    } else if (job == 4) {   // dlogits [N,A], scalar predicated
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = st_c0 + e;
        r_dz[e] = (k < N && m < A)
            ? (short)dlogits[(long long)k * A + m] : (short)0;
      }
    } else {                 // dvalue [N] f32, M = 1
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = st_c0 + e;
        r_dz[e] = (k < N && m == 0)
            ? (short)drla_f32_to_bf16(dvalue[k]) : (short)0;
      }
    }
  };

  auto store_chunk = [&]() {
    actT[st_c0 + 0][st_kk] = r_act[0]; actT[st_c0 + 1][st_kk] = r_act[1];
    actT[st_c0 + 2][st_kk] = r_act[2]; actT[st_c0 + 3][st_kk] = r_act[3];
    actT[st_c0 + 4][st_kk] = r_act[4]; actT[st_c0 + 5][st_kk] = r_act[5];
    actT[st_c0 + 6][st_kk] = r_act[6]; actT[st_c0 + 7][st_kk] = r_act[7];
    dzT[st_c0 + 0][st_kk] = r_dz[0]; dzT[st_c0 + 1][st_kk] = r_dz[1];
    dzT[st_c0 + 2][st_kk] = r_dz[2]; dzT[st_c0 + 3][st_kk] = r_dz[3];
    dzT[st_c0 + 4][st_kk] = r_dz[4]; dzT[st_c0 + 5][st_kk] = r_dz[5];
    dzT[st_c0 + 6][st_kk] = r_dz[6]; dzT[st_c0 + 7][st_kk] = r_dz[7];
  };

  load_chunk(0);
  for (int k0 = 0; k0 < N; k0 += 32) {
    store_chunk();
    __syncthreads();
    if (k0 + 32 < N) load_chunk(k0 + 32);
    // wave w: m rows [w*16, w*16+16); frags vec8 from LDS
    const bf16x8 a_frag = *reinterpret_cast<const bf16x8*>(
        &dzT[wave * 16 + (lane & 15)][(lane >> 4) * 8]);
    for (int ni = 0; ni < 4; ++ni) {
      const bf16x8 b_frag = *reinterpret_cast<const bf16x8*>(
          &actT[ni * 16 + (lane & 15)][(lane >> 4) * 8]);
      acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_frag, b_frag, acc[ni], 0, 0, 0);
    }
    __syncthreads();
  }
  // D: lane l reg r -> row (l>>4)*4+r (m), col l&15 (n)
  for (int ni = 0; ni < 4; ++ni) {
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wave * 16 + (lane >> 4) * 4 + r;
      const int n = n0 + ni * 16 + (lane & 15);
      if (m < M) out[(long long)m * MH_HID + n] = drla_f32_to_bf16(acc[ni][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// K2 fused action-embedding MLP: one-hot(prev_action) -> 256 (+bias, ReLU)
// -> 256 (+bias, ReLU), reference model/impala_actor_critic.py:12-16.
// The torch composition (lookup, add, relu, linear, relu + their backwards,
// two bias column-reduces and an embedding scatter) costs ~70 us/step in
// ~12 launches at [640]; these kernels do it in 1 fwd + 3 bwd launches.
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(256) void drla_embed_mlp_fwd(
    const long long* __restrict__ pa,     // [N]
    const bf16raw* __restrict__ table,    // [A,256]
    const bf16raw* __restrict__ b1,       // [256]
    const bf16raw* __restrict__ W2,       // [256,256] (nn.Linear [out,in])
    const bf16raw* __restrict__ b2,       // [256]
    bf16raw* __restrict__ out,            // [N,256] (post-ReLU2)
    bf16raw* __restrict__ a1stash,        // [N,256] (post-ReLU1)
    int N, int A,
    long long* __restrict__ idx_stash,    // [N] clamped pa copy (nullable)
    bf16raw* __restrict__ w2t,            // [256,256] W2^T out (nullable)
    long long slab_stride,                // 0: out is [N,256] contiguous
    const float* __restrict__ h_src,      // [N,H] f32 (slab mode)
    int H,
    const int* __restrict__ slot,         // drla_slot_base (nullable)
    long long pa_dist, long long h_dist) {
  pa = drla_slot_base(pa, slot, pa_dist);
  h_src = drla_slot_base(h_src, slot, h_dist);
  // slab mode (slab_stride != 0): out points at the embedding columns of a
  // row-major [N, slab_stride] bf16 slab — the gate-GEMM input, assembled in
  // place. The block's 16 rows also get h (f32 -> bf16, the rounding of
  // .to(bf16)) in the H columns after the embedding and the 8 pad columns
  // (1, 0 x 7) after those; 16 B stores, H % 8 == 0.
  __shared__ bf16raw a1img[MH_BM][MH_LD];
  __shared__ bf16raw outimg[MH_BM][MH_LD];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * MH_BM;
  // W2 in flight under the table gather and the layer-1 epilogue below
  MhFrags<MH_HID / 32> fw;
  MhSide sb;
  mh_load(fw, W2, MH_HID);
  mh_load_bias(sb, b2, MH_HID);
  {
    const int r = tid >> 4;
    const int c0 = (tid & 15) * 16;
    const int grow = row0 + r;
    // clamp: pa arrives from external actor data — an out-of-range
    // index must not become an aperture fault (drla_common.h)
    const long long idx =
        (grow < N) ? drla_clamp_idx((int)pa[grow], A) : 0;
    // the backward scatter reads this copy, never the caller's buffer
    if (idx_stash && grow < N && (tid & 15) == 0) idx_stash[grow] = idx;
    const bf16raw* trow = table + idx * MH_HID + c0;
    // requested together, ahead of the store loop
    bf16raw tv[16], bv1[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      tv[c] = trow[c];
      bv1[c] = b1[c0 + c];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const float v = fmaxf(drla_bf16_to_f32(tv[c]) + drla_bf16_to_f32(bv1[c]), 0.0f);
      const bf16raw bv = drla_f32_to_bf16(v);
      a1img[r][c0 + c] = bv;
      if (grow < N) a1stash[(long long)grow * MH_HID + c0 + c] = bv;
    }
  }
  __syncthreads();
  f32x4 acc[4];
  mh_mma(acc, fw, a1img, MH_HID);
  mh_epilogue<true, MH_BIAS>(acc, outimg, sb, nullptr, nullptr,
                             slab_stride ? nullptr : out, nullptr, row0, N,
                             MH_HID);
  // the side outputs come AFTER the pass: nothing of theirs is live while
  // the pass holds its weight fragments
  if (slab_stride != 0) {
    const int r = tid >> 4;
    const int c0 = (tid & 15) * 16;
    const int grow = row0 + r;
    if (grow < N) {
      // the post-ReLU2 image mh_pass left in LDS -> the slab's embedding
      // columns, two 16 B stores per thread (mh_pass ends on a barrier)
      bf16raw* orow = out + (long long)grow * slab_stride;
      *reinterpret_cast<uint4*>(orow + c0) =
          *reinterpret_cast<const uint4*>(&outimg[r][c0]);
      *reinterpret_cast<uint4*>(orow + c0 + 8) =
          *reinterpret_cast<const uint4*>(&outimg[r][c0 + 8]);
      // h (f32 -> bf16) and the pad columns behind it
      bf16raw* hrow = orow + MH_HID;
#pragma unroll 1  // short trip count; unrolled it costs VGPRs
      for (int c = (tid & 15) * 8; c < H; c += 128) {
        const float4 v0 = *reinterpret_cast<const float4*>(
            h_src + (long long)grow * H + c);
        const float4 v1 = *reinterpret_cast<const float4*>(
            h_src + (long long)grow * H + c + 4);
        uint4 p;
        p.x = drla_f32x2_to_bf16x2(v0.x, v0.y);
        p.y = drla_f32x2_to_bf16x2(v0.z, v0.w);
        p.z = drla_f32x2_to_bf16x2(v1.x, v1.y);
        p.w = drla_f32x2_to_bf16x2(v1.z, v1.w);
        *reinterpret_cast<uint4*>(hrow + c) = p;
      }
      if ((tid & 15) == 0) {
        // bf16 1.0 = 0x3F80 in column 0, zeros in columns 1..7
        *reinterpret_cast<uint4*>(hrow + H) = uint4{0x3F80u, 0u, 0u, 0u};
      }
    }
  }
  if (w2t) {
    // W2^T for the backward's dgrad pass, each block its share of the units
    for (int u = blockIdx.x * 256 + tid; u < 8192; u += gridDim.x * 256) {
      mh_wt_unit(W2, w2t, u);
    }
  }
}

// [256,256] transpose pack for the dgrad pass below
extern "C" __global__ void drla_embed_w2t_pack(
    const bf16raw* __restrict__ w2, bf16raw* __restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 65536;
       i += gridDim.x * blockDim.x) {
    out[i] = w2[(i & 255) * 256 + (i >> 8)];
  }
}

// backward: dz2 = dy * (out>0) (written for the dW2 GEMM), db2 = colsum,
// da1 = (dz2 @ W2) * (a1>0) (written for the table scatter), db1 = colsum.
// dy may be N-strided (a slice of the fused xh gradient). bias_ws: f32
// [2*256] ZERO on entry (atomic partials; db1 at [0:256], db2 at [256:]).
extern "C" __global__ __launch_bounds__(256) void drla_embed_mlp_bwd(
    const bf16raw* __restrict__ dy, long long dy_stride,
    const bf16raw* __restrict__ out, const bf16raw* __restrict__ a1stash,
    const bf16raw* __restrict__ W2T,  // [256,256] pre-transposed
    bf16raw* __restrict__ dz2,        // [N,256]
    bf16raw* __restrict__ da1,        // [N,256] (null with scat_idx)
    float* __restrict__ bias_ws, int N,
    const long long* __restrict__ scat_idx,  // [N] table rows (nullable)
    float* __restrict__ scat,                // [A,256] f32 table-grad sums
    int A,
    long long out_stride) {  // elements between rows of out (256: packed;
                             // wider: out lives in the xh slab)
  __shared__ bf16raw dz2img[MH_BM][MH_LD];
  __shared__ bf16raw da1img[MH_BM][MH_LD];
  __shared__ float colsum[MH_HID];
  __shared__ int srow[MH_BM];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * MH_BM;
  // W2^T in flight under the dz2 prologue below
  MhFrags<MH_HID / 32> fw;
  MhSide sm;
  mh_load(fw, W2T, MH_HID);
  if (scat_idx && tid < MH_BM) {
    srow[tid] = (row0 + tid < N)
        ? drla_clamp_idx((int)scat_idx[row0 + tid], A) : -1;
  }
  if (tid < MH_HID) colsum[tid] = 0.0f;
  __syncthreads();
  {
    const int r = tid >> 4;
    const int c0 = (tid & 15) * 16;
    const int grow = row0 + r;
    float part[16];
    // requested together, ahead of the store loop
    // (from a clamped row: rows past N are zeroed below)
    bf16raw ov[16], dv[16];
    const long long crow = min(grow, N - 1);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      ov[c] = out[crow * out_stride + c0 + c];
      dv[c] = dy[crow * dy_stride + c0 + c];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      float v = 0.0f;
      if (grow < N) {
        const float o = drla_bf16_to_f32(ov[c]);
        if (o > 0.0f) v = drla_bf16_to_f32(dv[c]);
      }
      const bf16raw bv = drla_f32_to_bf16(v);
      dz2img[r][c0 + c] = bv;
      if (grow < N) dz2[(long long)grow * MH_HID + c0 + c] = bv;
      part[c] = v;
    }
    for (int c = 0; c < 16; ++c) atomicAdd(&colsum[c0 + c], part[c]);
  }
  __syncthreads();
  if (tid < MH_HID) {
    atomicAdd(&bias_ws[MH_HID + tid], colsum[tid]);
    colsum[tid] = 0.0f;
  }
  __syncthreads();
  // dgrad through W2 with the ReLU1 mask and db1 column sums fused
  f32x4 acc[4];
  mh_mma(acc, fw, dz2img, MH_HID);
  // the mask values are requested here, behind the prologue's own loads
  mh_load_mask(sm, a1stash, row0, N);
  mh_epilogue<false, MH_MASK>(acc, da1img, sm, da1, colsum, nullptr,
                              nullptr, row0, N, MH_HID);
  if (tid < MH_HID) atomicAdd(&bias_ws[tid], colsum[tid]);
  if (scat_idx) {
    // table scatter in the epilogue (was drla_embed_bwd_scatter re-reading
    // da1 from global one launch later): thread = column, walking the
    // block's rows of the bf16 da1 image mh_pass left in LDS. Runs of rows
    // with the same table row are summed first, so a block issues between
    // 1 and MH_BM atomics per column, coalesced across the lanes. The
    // addends are the bf16-rounded values the standalone scatter reads.
    const int oc = tid;  // blockDim.x == MH_HID
    float acc = 0.0f;
    int cur = -1;
#pragma unroll 1  // unrolled, the 16 row/value pairs cost VGPRs (occupancy)
    for (int r = 0; r < MH_BM; ++r) {
      const int row = srow[r];
      if (row < 0) break;  // rows past N (only at the block's end)
      if (row != cur) {
        if (cur >= 0) atomicAdd(&scat[(long long)cur * MH_HID + oc], acc);
        acc = 0.0f;
        cur = row;
      }
      acc += drla_bf16_to_f32(da1img[r][oc]);
    }
    if (cur >= 0) atomicAdd(&scat[(long long)cur * MH_HID + oc], acc);
  }
}

// finalize for the fused embed backward: cast the persistent f32 scratch
// ([A*256] table-grad partials ++ [512] bias partials) to three contiguous
// bf16 outputs, re-zeroing the scratch (zero-between-calls invariant).
extern "C" __global__ void drla_embed_finalize(
    float* __restrict__ src, bf16raw* __restrict__ dtable,
    bf16raw* __restrict__ db1, bf16raw* __restrict__ db2,
    long long n_table) {
  const long long total = n_table + 512;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += gridDim.x * (long long)blockDim.x) {
    const bf16raw v = drla_f32_to_bf16(src[i]);
    src[i] = 0.0f;
    if (i < n_table) dtable[i] = v;
    else if (i < n_table + 256) db1[i - n_table] = v;
    else db2[i - n_table - 256] = v;
  }
}
