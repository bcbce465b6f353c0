// Backward of the two IMPALA heads (policy 256->256->256->A, value
// 256->256->256->1; forward in mlp_heads.hip), two launches:
//
//   drla_mlp_heads_bwd  d3 -> dz2 -> dz1 -> dh for both chains, the six f32
//                       bias-gradient sums
//   drla_heads_wgrad    six dW = dz^T . act in one launch, and the bf16
//                       conversion of the bias sums
//
// drla_mlp_heads_bwd: one 512-thread workgroup owns 16 rows of BOTH chains.
// Wave w runs chain w / 4 (0 policy, 1 value) and output columns
// 64 (w % 4) .. + 63. Output is computed transposed (D[out][row]) so the
// pre-transposed weight is the first MFMA operand, read straight from global
// memory into registers, and the activation is a 16-byte LDS read; a lane
// then holds four consecutive outputs of one row. All of W2^T and the first
// half of W1^T are requested before anything is used, the second half of
// W1^T as soon as W2^T's MFMAs have freed its registers.
//   * dz2 / dz1 are rounded once, written to an LDS image (the next pass's
//     operand), and leave for global memory from that image as 16-byte row
//     stores behind the barrier that publishes it.
//   * Bias-gradient column sums add the unrounded f32 values over the 16
//     lanes that share a column with four DPP steps; a block then issues one
//     global atomic per column into the workspace tail (which must be zero).
//   * dh: the value waves leave their f32 tile in LDS; after one barrier the
//     policy waves add their own accumulators and store 16 bytes per lane.
//     Each element is written once with a plain store: no atomics on dh, and
//     nothing of its previous contents is read.
//
// drla_heads_wgrad: 64 x 64 tiles, both operands k-rows ([N][256], a memory
// row is one k). A 64-row chunk is staged as it lies in memory, with 16-byte
// stores into the swizzled 64 x 128-byte image of conv_wgrad_lds.h, and read
// back transposed with ds_read_b64_tr_b16. Global loads run one chunk ahead
// in registers, the images are double-buffered, one barrier per chunk. Rows
// at or past N are loaded from a clamped address and staged as zeros. The
// two narrow jobs (dW3p from dlogits [N][A], dW3v from dvalue [N]) stage
// their dz operand as the flat bytes of the chunk (one or two aligned
// 16-byte loads per thread, or one f32) and pick their fragments out of it
// with 2-byte LDS reads.
//
// Packed-f32 VALU ops stay out of this file: every function carries NOPK_FN,
// helpers are drla_nopk.h's (which says why), this file's own or builtins.

#include "drla_kernels.h"
#include "drla_nopk.h"

namespace {

constexpr int HB_H = MH_HID;
constexpr int HB_ACT_LD = HB_H + 8;   // bf16 activation image rows, elements
constexpr int HB_DH_LD = HB_H + 4;    // f32 dh tile rows, elements
constexpr int HB_D3_LD = MH_MAX_A + 8;
constexpr int HB_BLOCK = 512;         // drla_mlp_heads_bwd
constexpr int HB_WG_BLOCK = 256;      // drla_heads_wgrad
static_assert(HB_H == 4 * 64 && MH_BM == 16 && MH_MAX_A == 32,
              "two chains x four waves x 64 output columns, 16-row blocks, "
              "layer 3 one 32-deep k-step");
static_assert((HB_ACT_LD * 2 / 16) % 2 == 1,
              "odd pitch in 16-byte units: fragment reads spread over banks");
// the narrow jobs' flat chunk: 64 rows of at most 32 elements plus up to 7
// elements of misalignment, in whole 16-byte vectors
constexpr int HB_FLAT_VECS = DRLA_WG_ROWS * MH_MAX_A / 8 + 1;
static_assert(HB_FLAT_VECS * 16 <= NOPK_KR_SUB && HB_FLAT_VECS <= HB_WG_BLOCK + 1,
              "the flat chunk fits the dz image it replaces; a thread loads "
              "vector tid, thread 0 also vector 256");

NOPK_INL long long hb_minll(long long a, long long b) { return a < b ? a : b; }
NOPK_INL void hb_atomic_add(float* p, float v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// v summed over the 16 lanes of a DPP row (the lanes that share lane / 16);
// every lane of the row gets the sum. quad_perm [1,0,3,2], [2,3,0,1],
// row_half_mirror, row_mirror.
NOPK_INL float hb_row_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
           0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
           0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
           0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
           0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
  return v;
}

// ---- drla_mlp_heads_bwd: per-wave pieces ----------------------------------

// half of a wave's slice of a [256][256] first operand: rows out0 + 16 ni +
// l % 16, four 32-deep k-steps from k0 (64 VGPRs), requested together
struct HbW128 {
  bf16x8 a[4][4];
};
NOPK_INL void hb_load_w128(HbW128& f, const bf16raw* __restrict__ w, int out0,
                         int k0, int lane) {
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      f.a[kc][ni] = *reinterpret_cast<const bf16x8*>(
          w + (out0 + ni * 16 + (lane & 15)) * HB_H + k0 + kc * 32 +
          (lane >> 4) * 8);
    }
  }
}
// acc[ni] += D[out0 + 16 ni + 4 (l / 16) + e][row l % 16] over the 128 k
// from k0 of act [16][HB_ACT_LD], k ascending
NOPK_INL void hb_mma128(f32x4 (&acc)[4], const HbW128& f,
                      const bf16raw (*act)[HB_ACT_LD], int k0, int lane) {
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) {
    const bf16x8 bf = *reinterpret_cast<const bf16x8*>(
        &act[lane & 15][k0 + kc * 32 + (lane >> 4) * 8]);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[kc][ni], bf,
                                                        acc[ni], 0, 0, 0);
    }
  }
}
// the four values a lane's acc[ni] goes with, of a [rows][256] bf16 matrix
// row: one 8-byte load per ni
NOPK_INL void hb_load_side(ushort4v (&s)[4], const bf16raw* __restrict__ row,
                         int out0, int lane) {
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    s[ni] = *reinterpret_cast<const ushort4v*>(row + out0 + ni * 16 +
                                               (lane >> 4) * 4);
  }
}

// One masked pass's epilogue for a wave: v = live && mask > 0 ? acc : 0; the
// column sums of the unrounded v go to bias[256] with one atomic per column
// (lane 16 g + j owns column out0 + 16 (j / 4) + 4 g + j % 4); v rounded to
// bf16 goes to the LDS image img [16][HB_ACT_LD].
NOPK_INL void hb_masked_out(const f32x4 (&acc)[4], const ushort4v (&mask)[4],
                          bool live, bf16raw (*img)[HB_ACT_LD],
                          float* __restrict__ bias, int out0, int lane) {
  const int row = lane & 15, g = lane >> 4;
  float mine = 0.f;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = (live && nopk_f32(mask[ni][e]) > 0.f) ? acc[ni][e] : 0.f;
      const float s = hb_row_sum(v[e]);
      mine = (row == ni * 4 + e) ? s : mine;
    }
    *reinterpret_cast<nopk_u32x2*>(&img[row][out0 + ni * 16 + g * 4]) =
        nopk_round4(v);
  }
  hb_atomic_add(bias + out0 + 16 * (row >> 2) + 4 * g + (row & 3), mine);
}

// the block's two [16][256] bf16 images (policy, value) -> global rows, two
// 16-byte stores per thread; rows < N only
NOPK_INL void hb_store_images(const bf16raw (*imgp)[HB_ACT_LD],
                            const bf16raw (*imgv)[HB_ACT_LD],
                            bf16raw* __restrict__ outp,
                            bf16raw* __restrict__ outv, int row0, int N,
                            int tid) {
  const int c = tid >> 8, r = (tid >> 4) & 15, ch = tid & 15;
  const bf16raw(*img)[HB_ACT_LD] = c ? imgv : imgp;
  bf16raw* out = c ? outv : outp;
  if (row0 + r < N) {
    bf16raw* d = out + (long long)(row0 + r) * HB_H;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<nopk_u32x4*>(d + 8 * (ch + 16 * j)) =
          *reinterpret_cast<const nopk_u32x4*>(&img[r][8 * (ch + 16 * j)]);
    }
  }
}

}  // namespace

// grid ceil(N / 16). Takes PRE-TRANSPOSED weights: wT3p [256][32] =
// pad(W3p^T), wT2p / wT1p / wT2v / wT1v [256][256] = W^T, W3v [1][256] as it
// is (the value out layer's backward is an outer product). dh is written,
// every element once; the six bias sums are added to and must come in zero.
NOPK_PRE(HB_BLOCK) __global__ void drla_mlp_heads_bwd(
    const bf16raw* __restrict__ dlogits,   // [N,A]
    const float* __restrict__ dvalue,      // [N]
    const bf16raw* __restrict__ stash,     // [N,5*256]
    const bf16raw* __restrict__ wT1p, const bf16raw* __restrict__ wT2p,
    const bf16raw* __restrict__ wT3p,      // [256,32] padded
    const bf16raw* __restrict__ wT1v, const bf16raw* __restrict__ wT2v,
    const bf16raw* __restrict__ W3v,       // [1,256]
    bf16raw* __restrict__ dz1p, bf16raw* __restrict__ dz2p,  // [N,256]
    bf16raw* __restrict__ dz1v, bf16raw* __restrict__ dz2v,  // [N,256]
    float* __restrict__ dh,                // [N,256]
    float* __restrict__ db1p, float* __restrict__ db2p,
    float* __restrict__ db3p,              // [A]
    float* __restrict__ db1v, float* __restrict__ db2v,
    float* __restrict__ db3v,              // [1]
    int N, int A) {
  __shared__ __attribute__((aligned(16))) bf16raw d3[MH_BM][HB_D3_LD];
  // [chain][0: dz2, 1: dz1]
  __shared__ __attribute__((aligned(16)))
      bf16raw dzl[2][2][MH_BM][HB_ACT_LD];
  __shared__ __attribute__((aligned(16))) float dht[MH_BM][HB_DH_LD];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int c = __builtin_amdgcn_readfirstlane(wave >> 2);
  const int out0 = __builtin_amdgcn_readfirstlane((wave & 3) * 64);
  const int row0 = blockIdx.x * MH_BM;
  const int row = lane & 15;  // the row of this lane's accumulators
  const bool live = row0 + row < N;
  const long long grow = nopk_min(row0 + row, N - 1);
  const long long soff = (long long)N * HB_H;
  const bf16raw* a1 = stash + (c ? 2 * soff : 0);
  const bf16raw* a2 = a1 + soff;

  // everything the chain reads from global memory, requested before anything
  // is used
  HbW128 f2lo, f2hi, f1lo;
  bf16x8 f3[4];
  ushort4v w3r[4], mask2[4], mask1[4];
  const bf16raw* wT2 = c ? wT2v : wT2p;
  const bf16raw* wT1 = c ? wT1v : wT1p;
  hb_load_w128(f2lo, wT2, out0, 0, lane);
  hb_load_w128(f2hi, wT2, out0, 128, lane);
  hb_load_w128(f1lo, wT1, out0, 0, lane);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    f3[ni] = *reinterpret_cast<const bf16x8*>(
        wT3p + (out0 + ni * 16 + (lane & 15)) * MH_MAX_A + (lane >> 4) * 8);
  }
  hb_load_side(w3r, W3v, out0, lane);
  hb_load_side(mask2, a2 + grow * HB_H, out0, lane);
  const float dv_raw = dvalue[grow];
  const float dv = live ? dv_raw : 0.f;

  // d3p = dlogits, zero-padded to 16 x 32
  {
    const int r = tid >> 5, a = tid & 31;
    const bool in = a < A && row0 + r < N;
    const bf16raw v = dlogits[(long long)nopk_min(row0 + r, N - 1) * A +
                              nopk_min(a, A - 1)];
    d3[r][a] = in ? v : (bf16raw)0;
  }
  // db3v: the block's dvalue rows, summed in row order by one thread
  if (tid == HB_BLOCK - 1) {
    float x[MH_BM];
#pragma unroll
    for (int r = 0; r < MH_BM; ++r) x[r] = dvalue[nopk_min(row0 + r, N - 1)];
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < MH_BM; ++r) s += row0 + r < N ? x[r] : 0.f;
    hb_atomic_add(db3v, s);
  }
  nopk_barrier();
  // db3p: dlogits column sums in row order (dead rows are zeros)
  if (tid < A) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < MH_BM; ++r) s += nopk_f32(d3[r][tid]);
    hb_atomic_add(db3p + tid, s);
  }

  // dz2 = (d3 . W3) masked by a2 > 0
  {
    f32x4 acc[4];
    if (c == 0) {
      const bf16x8 bf =
          *reinterpret_cast<const bf16x8*>(&d3[row][(lane >> 4) * 8]);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        acc[ni] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(f3[ni], bf, z, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[ni][e] = dv * nopk_f32(w3r[ni][e]);
      }
    }
    hb_masked_out(acc, mask2, live, dzl[c][0], c ? db2v : db2p, out0, lane);
  }
  // the second mask takes the registers layer 3 has left; W2^T's MFMAs run
  // in front of its first use
  hb_load_side(mask1, a1 + grow * HB_H, out0, lane);
  nopk_barrier();
  hb_store_images(dzl[0][0], dzl[1][0], dz2p, dz2v, row0, N, tid);

  // dz1 = (dz2 . W2) masked by a1 > 0
  HbW128 f1hi;
  {
    f32x4 acc[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};
    hb_mma128(acc, f2lo, dzl[c][0], 0, lane);
    hb_mma128(acc, f2hi, dzl[c][0], 128, lane);
    // the second half of W1^T takes the registers W2^T has left
    hb_load_w128(f1hi, wT1, out0, 128, lane);
    hb_masked_out(acc, mask1, live, dzl[c][1], c ? db1v : db1p, out0, lane);
  }
  nopk_barrier();
  hb_store_images(dzl[0][1], dzl[1][1], dz1p, dz1v, row0, N, tid);

  // dh = dz1p . W1p + dz1v . W1v: the value chain's f32 tile goes through
  // LDS to the policy waves, which add their own and store
  {
    f32x4 acc[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};
    hb_mma128(acc, f1lo, dzl[c][1], 0, lane);
    hb_mma128(acc, f1hi, dzl[c][1], 128, lane);
    if (c == 1) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        *reinterpret_cast<f32x4*>(
            &dht[row][out0 + ni * 16 + (lane >> 4) * 4]) = acc[ni];
      }
    }
    nopk_barrier();
    if (c == 0 && live) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int col = out0 + ni * 16 + (lane >> 4) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(&dht[row][col]);
        f32x4 o;
        // (0 + p) + v: the bits two atomic adds onto a zeroed buffer gave
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (0.f + acc[ni][e]) + v[e];
        *reinterpret_cast<f32x4*>(dh + grow * HB_H + col) = o;
      }
    }
  }
}

// grid 73: jobs 0-3 are 4 x 4 tiles of 64 x 64 (blocks 0..63), job 4 is
// blocks 64..67 (one m-tile, A <= 32), job 5 blocks 68..71; block 72 converts
// the f32 bias-gradient sums to six contiguous bf16 tensors.
//   0: dW1p = dz1p^T . hb     3: dW2v = dz2v^T . a1v
//   1: dW2p = dz2p^T . a1p    4: dW3p = dlogits^T . a2p   M = A
//   2: dW1v = dz1v^T . hb     5: dW3v = dvalue^T . a2v    M = 1
NOPK_PRE(HB_WG_BLOCK) __global__ void drla_heads_wgrad(
    const bf16raw* __restrict__ dz1p, const bf16raw* __restrict__ dz2p,
    const bf16raw* __restrict__ dz1v, const bf16raw* __restrict__ dz2v,
    const bf16raw* __restrict__ dlogits,  // [N,A]
    const float* __restrict__ dvalue,     // [N]
    const bf16raw* __restrict__ stash,    // [N,5*256]
    bf16raw* __restrict__ dw1p, bf16raw* __restrict__ dw2p,
    bf16raw* __restrict__ dw3p,           // [A,256]
    bf16raw* __restrict__ dw1v, bf16raw* __restrict__ dw2v,
    bf16raw* __restrict__ dw3v,           // [1,256]
    const float* __restrict__ ws_tail,    // f32 bias sums from heads_bwd
    bf16raw* __restrict__ db1p, bf16raw* __restrict__ db2p,
    bf16raw* __restrict__ db3p, bf16raw* __restrict__ db1v,
    bf16raw* __restrict__ db2v, bf16raw* __restrict__ db3v,
    int N, int A) {
  // [dz: 2 buffers][act: 2 buffers]
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * NOPK_KR_SUB];
  const int tid = threadIdx.x;
  const int bid = blockIdx.x;
  if (bid == 72) {
    const int total = 4 * 256 + A + 1;
    for (int i = tid; i < total; i += HB_WG_BLOCK) {
      const bf16raw v = nopk_round1(ws_tail[i]);
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
  const long long soff = (long long)N * HB_H;
  const bf16raw* dz;
  const bf16raw* act;
  bf16raw* out;
  int M;
  switch (job) {
    case 0: dz = dz1p; act = stash + 4 * soff; out = dw1p; M = 256; break;
    case 1: dz = dz2p; act = stash;            out = dw2p; M = 256; break;
    case 2: dz = dz1v; act = stash + 4 * soff; out = dw1v; M = 256; break;
    case 3: dz = dz2v; act = stash + 2 * soff; out = dw2v; M = 256; break;
    case 4: dz = dz1p; act = stash + soff;     out = dw3p; M = A;   break;
    default: dz = dz1p; act = stash + 3 * soff; out = dw3v; M = 1;
  }
  const int m0 = mt * 64;
  const int n0 = nt * 64;
  const int wave = tid >> 6, lane = tid & 63;
  const int srow = nopk_slot_row(tid, 0), sch = nopk_slot_ch(tid);
  const bool wide = job < 4;  // block-uniform
  const int nchunks = (N + DRLA_WG_ROWS - 1) / DRLA_WG_ROWS;

  // The narrow jobs' dz operand. Job 4: dlogits seen as 16-byte vectors from
  // its pointer rounded down to 16 bytes, `mis` elements in front. A chunk of
  // 64 rows starts at element mis + 64 A t, that is in vector 8 A t, and ends
  // in vector 8 A (t + 1) at the latest. An aligned vector that holds one
  // element of the tensor lies in one page with it, so loading it whole is
  // safe; vectors past the last such one are clamped to it. Job 5: rounded
  // dvalue, one element per row.
  const unsigned long long dl_addr = (unsigned long long)dlogits;
  const int mis = job == 4 ? (int)((dl_addr & 15) >> 1) : 0;
  const nopk_u32x4* dl_vec =
      reinterpret_cast<const nopk_u32x4*>(dl_addr & ~15ull);
  const long long vlast = (mis + (long long)N * A - 1) >> 3;
  const int An = job == 4 ? A : 1;  // row pitch of the flat chunk

  unsigned char* As = lds;
  unsigned char* Bs = lds + 2 * NOPK_KR_SUB;
  bf16x8 r_a[2], r_b[2];
  nopk_u32x4 r_n0, r_n1;
  float r_dv;
  unsigned int klive = 0;

  auto load = [&](int t) NOPK_LAMBDA {
    klive = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = t * DRLA_WG_ROWS + srow + 32 * j;
      klive |= (unsigned int)(k < N) << j;
      const long long koff = (long long)nopk_min(k, N - 1) * HB_H + 8 * sch;
      r_b[j] = *reinterpret_cast<const bf16x8*>(act + koff + n0);
      if (wide) r_a[j] = *reinterpret_cast<const bf16x8*>(dz + koff + m0);
    }
    if (job == 4) {
      const long long v0 = 8ll * A * t;
      r_n0 = dl_vec[hb_minll(v0 + nopk_min(tid, 8 * A), vlast)];
      r_n1 = dl_vec[hb_minll(v0 + HB_WG_BLOCK, vlast)];
    } else if (job == 5) {
      r_dv = dvalue[nopk_min(t * DRLA_WG_ROWS + (tid & 63), N - 1)];
    }
  };
  auto store = [&](int buf) NOPK_LAMBDA {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool in = ((klive >> j) & 1u) != 0;
      const int o = nopk_chunk_off(srow + 32 * j, sch);
      *reinterpret_cast<bf16x8*>(Bs + buf * NOPK_KR_SUB + o) =
          in ? r_b[j] : nopk_zero8();
      if (wide) {
        *reinterpret_cast<bf16x8*>(As + buf * NOPK_KR_SUB + o) =
            in ? r_a[j] : nopk_zero8();
      }
    }
    if (job == 4) {
      *reinterpret_cast<nopk_u32x4*>(As + buf * NOPK_KR_SUB + 16 * tid) = r_n0;
      if (tid == 0) {
        *reinterpret_cast<nopk_u32x4*>(As + buf * NOPK_KR_SUB + 16 * HB_WG_BLOCK) =
            r_n1;
      }
    } else if (job == 5) {
      if (tid < 64) {
        *reinterpret_cast<bf16raw*>(As + buf * NOPK_KR_SUB + 2 * tid) =
            nopk_round1(r_dv);
      }
    }
  };
  auto frag = [&](const unsigned char* img, int t16, int ks)
                  NOPK_LAMBDA -> bf16x8 {
    return nopk_frag_kr(img, t16, ks, lane);
  };

  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};
  // a narrow job's waves past its M rows stage and wait, and compute nothing
  const bool computes = wide || wave * 16 < M;  // wave-uniform
  const int mloc = wave * 16 + (lane & 15);     // this lane's m in the tile

  load(0);
  store(0);
  load(1);
  nopk_barrier();
#pragma unroll 1
  for (int t = 0; t < nchunks; ++t) {
    const int cur = t & 1;
    if (t + 1 < nchunks) {
      store(1 - cur);
      load(t + 2);
    }
    if (computes) {
#pragma unroll
      for (int ks = 0; ks < DRLA_WG_ROWS / 32; ++ks) {
        bf16x8 af;
        if (wide) {
          af = frag(As + cur * NOPK_KR_SUB, wave, ks);
        } else {
          const bf16raw* flat =
              reinterpret_cast<const bf16raw*>(As + cur * NOPK_KR_SUB);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int k = 32 * ks + 8 * (lane >> 4) + e;
            const bf16raw v = flat[mis + k * An + nopk_min(mloc, M - 1)];
            af[e] = (mloc < M && t * DRLA_WG_ROWS + k < N) ? (short)v
                                                           : (short)0;
          }
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const bf16x8 bf = frag(Bs + cur * NOPK_KR_SUB, ni, ks);
          // B first: D[n][m], a lane holds n = 4 (l / 16) .. + 3 of m = l % 16
          acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, af, acc[ni],
                                                            0, 0, 0);
        }
      }
    }
    nopk_barrier();
  }
  const int m = m0 + mloc;
  if (m < M) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + ni * 16 + (lane >> 4) * 4;
      *reinterpret_cast<nopk_u32x2*>(out + (long long)m * HB_H + n) =
          nopk_round4(acc[ni]);
    }
  }
}
