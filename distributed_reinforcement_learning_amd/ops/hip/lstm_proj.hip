// The R2D2 LSTM's input projection and every weight gradient of the layer,
// bf16 in and out, f32 accumulation in mfma_f32_16x16x32_bf16, one rounding
// per stored bf16 value. The LSTM input is [conv | emb] along the features;
// the kernels take the two parts as they are and never see a concatenation.
// W is lstm.weight [F + H][4H] whole (F = F1 + F2), read in place.
//
//   drla_lstm_proj_fwd     ws[z][M][4H] = split z of conv . W[0:F1] +
//                                         emb . W[F1:F]
//   drla_lstm_proj_reduce  xg[M][4H]    = bf16(ws[0] + .. + ws[S-1] + b)
//   drla_lstm_proj_dgrad   dconv[M][F1], demb[M][F2] = dxg[M][4H] . W[0:F]^T
//   drla_lstm_proj_wgrad   dW[F + H][4H] = [conv | emb | h_prev]^T . dxg,
//                          db[4H]        = column sums of dxg
//
// Every block is 256 threads on one 64 x 64 output tile; wave w owns the
// 16-row tile w across the four 16-column tiles. The contraction runs in
// chunks of 64: global loads go to registers one chunk ahead, the LDS images
// are double-buffered, one barrier per chunk. An operand lies one of two ways:
//   k-contiguous  memory rows run along k (conv, emb in the forward; dxg and
//                 W's rows in the dgrad). Staged as a padded [64][64 + 8]
//                 tile, read back as 16-byte fragments.
//   k-rows        a memory row is one k (W in the forward; conv, emb, h_prev
//                 and dxg in the wgrad). Staged as it comes from memory in
//                 the swizzled 64-row x 128-byte image of conv_wgrad_lds.h
//                 (slot drla_wg_b_slot<64>) and read back transposed with
//                 ds_read_b64_tr_b16; that header proves the gather and both
//                 bank rules at compile time.
// A thread stages two 16-byte pieces of each operand per chunk: row srow and
// srow + 32, 16-byte column sch.
//
// Forward: F1 is a multiple of 64, so a 64-k chunk lies in conv or in emb and
// the W row of chunk c is 64 c in both. grid = (4H tiles, M tiles, S); a
// split walks its share of the chunks and stores its whole f32 tile (zeros
// for an empty share), so the workspace needs no clearing; the reduce adds
// the slices in index order and the bias in f32. Same bits every call.
//
// dgrad: the reduction is only 4H deep and both operands are k-contiguous. A
// 64-column tile starts at a multiple of 64, F1 is one, so a tile belongs to
// dconv or to demb, each a dense tensor of its own.
//
// wgrad: blockIdx.x is the job, (dW row tile, column tile). Rows of dW below
// F1 come from conv, below F from emb, the rest from the bf16 h_prev stash.
// F is a multiple of 8 only, so the tile that holds row F takes its rows per
// 8-row piece: a thread's piece lies in one source, and the threads of one
// block may read from two. h_prev rows are H elements with H even, not
// 16-byte pieces: a piece of it is four 4-byte loads. The tiles of the first
// row block also add the dxg image's columns in row order: db.
//
// Edges: M and H are arbitrary (H even), F2 and 4H multiples of 8. A piece
// outside its matrix is loaded from a clamped (valid) address and staged as
// zeros, EXEC is full around the transposed reads, stores are predicated.
//
// Packed-f32 VALU ops stay out of this file as in gate_gemm.hip: every
// function carries LP_FN, helpers are this file's own or builtins.

#include "drla_kernels.h"
#include "conv_wgrad_lds.h"

#define LP_FN __attribute__((target("no-packed-fp32-ops")))
#define LP_INL LP_FN __device__ __forceinline__
#define LP_LAMBDA \
  __attribute__((always_inline, target("no-packed-fp32-ops")))
#define LP_PRE extern "C" LP_FN __launch_bounds__(DRLA_LP_BLOCK)

namespace {

constexpr int LP_T = DRLA_LP_TILE;        // tile edge and chunk depth
constexpr int LP_PITCH = (LP_T + 8) * 2;  // bytes per k-contiguous LDS row
constexpr int LP_KC = LP_T * LP_PITCH;    // one k-contiguous tile
constexpr int LP_ROWB = 128;              // k-rows image: 64 columns
constexpr int LP_KR = DRLA_WG_ROWS * LP_ROWB;
static_assert(LP_T == 64 && LP_T == DRLA_WG_ROWS && DRLA_LP_BLOCK == 256,
              "the k-rows image of conv_wgrad_lds.h is 64 k x 64 columns, "
              "staged by 256 threads in two passes");
static_assert((LP_PITCH / 16) % 2 == 1,
              "odd pitch in 16-byte units: fragment reads spread over banks");

typedef __attribute__((ext_vector_type(2))) float lp_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 lp_bf16x2;
typedef __attribute__((ext_vector_type(4))) short lp_s16x4;
typedef __attribute__((ext_vector_type(2))) unsigned int lp_u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int lp_u32x4;

LP_INL void lp_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
LP_INL int lp_min(int a, int b) { return a < b ? a : b; }
LP_INL float lp_f32(bf16raw u) {
  return __builtin_bit_cast(float, (unsigned int)u << 16);
}
// two f32 -> packed bf16, round to nearest even: one v_cvt_pk_bf16_f32
LP_INL unsigned int lp_round2(float a, float b) {
  return __builtin_bit_cast(
      unsigned int, __builtin_convertvector(lp_f32x2{a, b}, lp_bf16x2));
}
LP_INL lp_u32x2 lp_round4(f32x4 v) {
  return lp_u32x2{lp_round2(v[0], v[1]), lp_round2(v[2], v[3])};
}

// drla_wg_chunk_off<128> / drla_wg_tr_off<128> / drla_wg_elem_off<128> at run
// time. The header's constexpr functions are not always_inline, so they are
// restated here under LP_FN and held equal to them at compile time.
LP_INL constexpr int lp_chunk_off(int row, int ch) {
  const int sw = (row & 1) | (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2);
  return LP_ROWB * row + 16 * (ch ^ sw);
}
LP_INL constexpr int lp_tr_off(int lane, int tile) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  return lp_chunk_off(8 * g + q, 2 * tile + (p >> 1)) + 8 * (p & 1);
}
LP_INL constexpr int lp_elem_off(int row, int col) {
  return lp_chunk_off(row, col >> 3) + 2 * (col & 7);
}
constexpr bool lp_maps_match_header() {
  for (int row = 0; row < DRLA_WG_ROWS; ++row) {
    for (int ch = 0; ch < 8; ++ch)
      if (lp_chunk_off(row, ch) != drla_wg_chunk_off<LP_ROWB>(row, ch))
        return false;
    for (int col = 0; col < 64; ++col)
      if (lp_elem_off(row, col) != drla_wg_elem_off<LP_ROWB>(row, col))
        return false;
  }
  for (int lane = 0; lane < 64; ++lane)
    for (int tile = 0; tile < 4; ++tile)
      if (lp_tr_off(lane, tile) != drla_wg_tr_off<LP_ROWB>(lane, tile))
        return false;
  // the staging slot of this file: row tid / 8 + 32 j, chunk tid % 8
  for (int tid = 0; tid < DRLA_LP_BLOCK; ++tid)
    for (int j = 0; j < 2; ++j) {
      const DrlaWgSlot s = drla_wg_b_slot<64>(tid, j);
      if (s.row != (tid >> 3) + 32 * j || s.ch != (tid & 7)) return false;
    }
  return true;
}
static_assert(lp_maps_match_header(),
              "the k-rows maps and slot are those conv_wgrad_lds.h proves");

// registers -> LDS, pass j of this thread's slot
LP_INL void lp_stage_kc(unsigned char* lds, int tid, int j, bf16x8 v) {
  *reinterpret_cast<bf16x8*>(lds + ((tid >> 3) + 32 * j) * LP_PITCH +
                             16 * (tid & 7)) = v;
}
LP_INL void lp_stage_kr(unsigned char* lds, int tid, int j, bf16x8 v) {
  *reinterpret_cast<bf16x8*>(lds + lp_chunk_off((tid >> 3) + 32 * j,
                                                tid & 7)) = v;
}
// 16x16x32 operand of 16-wide tile t16, k-step ks: lane l gets element
// (16 t16 + l % 16, 32 ks + 8 (l / 16) + e) in e = 0..7
LP_INL bf16x8 lp_frag_kc(const unsigned char* lds, int t16, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(
      lds + (t16 * 16 + (lane & 15)) * LP_PITCH + 64 * ks + 16 * (lane >> 4));
}
// EXEC is full at every call
LP_INL bf16x8 lp_frag_kr(const unsigned char* lds, int t16, int ks, int lane) {
  typedef __attribute__((address_space(3))) lp_s16x4* lds_ptr;
  const unsigned char* q = lds + lp_tr_off(lane, t16) + 32 * ks * LP_ROWB;
  const lp_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)q);
  const lp_s16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(q + 4 * LP_ROWB));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// A [rows][ld] bf16 matrix read in 16-byte pieces, for one 64 x 64 tile whose
// second index (the contiguous one) starts at c0. As a k-contiguous operand
// the first index is the tile's row and the second is k; as a k-rows operand
// the first is k and the second the tile's column: the same addresses, the
// caller says which index moves per chunk.
struct LpPiece {
  bf16x8 r[2];
  unsigned int live;  // bit j: piece j is inside the matrix

  // rows r0 + srow + 32 j, columns c0 + 8 sch .. + 7 of p [nrows][ld] with
  // ncols columns (a multiple of 8, at least 8; nrows at least 1)
  LP_INL void load(const bf16raw* __restrict__ p, long long ld, int r0,
                   int nrows, int c0, int ncols, int tid) {
    const int c = c0 + 8 * (tid & 7);
    const long long coff = lp_min(c, ncols - 8);
    live = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = r0 + (tid >> 3) + 32 * j;
      live |= (unsigned int)(row < nrows && c < ncols) << j;
      r[j] = *reinterpret_cast<const bf16x8*>(
          p + (long long)lp_min(row, nrows - 1) * ld + coff);
    }
  }
  LP_INL bf16x8 get(int j) const {
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    return ((live >> j) & 1u) ? r[j] : z;
  }
};

// the epilogue all three products share: wave's 16-row tile, lane's row
// l % 16 and four columns 4 (l / 16) .. + 3 of each 16-column tile
LP_INL void lp_store_bf16(const f32x4 (&acc)[4], bf16raw* __restrict__ c,
                          long long ldc, int m0, int mmax, int n0, int nmax,
                          int wave, int lane) {
  const int m = m0 + 16 * wave + (lane & 15);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = n0 + 16 * ni + 4 * (lane >> 4);
    if (m < mmax && n < nmax) {  // nmax % 8 == 0: four columns in or out
      *reinterpret_cast<lp_u32x2*>(c + (long long)m * ldc + n) =
          lp_round4(acc[ni]);
    }
  }
}

}  // namespace

// grid (ceil(N / 64), ceil(M / 64), S). conv [M][F1] (row stride ldc), emb
// [M][F2] (lde), w [F1 + F2 ..][N] (ldw) -> ws [S][M][N] f32
LP_PRE __global__ void drla_lstm_proj_fwd(
    const bf16raw* __restrict__ conv, long long ldc,
    const bf16raw* __restrict__ emb, long long lde,
    const bf16raw* __restrict__ w, long long ldw, float* __restrict__ ws,
    int M, int F1, int F2, int N) {
  __shared__ __attribute__((aligned(16))) unsigned char As[2][LP_KC];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2][LP_KR];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int n0 = blockIdx.x * LP_T, m0 = blockIdx.y * LP_T;
  const int F = F1 + F2;
  const int nc1 = F1 / LP_T;
  const int chunks = nc1 + (F2 + LP_T - 1) / LP_T;
  const int per = (chunks + (int)gridDim.z - 1) / (int)gridDim.z;
  const int c_begin = lp_min((int)blockIdx.z * per, chunks);
  const int nchunks = lp_min(c_begin + per, chunks) - c_begin;

  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};

  LpPiece pa, pb;
  // chunk c of the whole product; past the last one the addresses are the
  // last chunk's and the registers are never staged
  auto load = [&](int c) LP_LAMBDA {
    c = lp_min(c, chunks - 1);
    if (c < nc1) {  // block-uniform
      pa.load(conv, ldc, m0, M, LP_T * c, F1, tid);
    } else {
      pa.load(emb, lde, m0, M, LP_T * (c - nc1), F2, tid);
    }
    pb.load(w, ldw, LP_T * c, F, n0, N, tid);
  };
  auto stage = [&](int buf) LP_LAMBDA {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      lp_stage_kc(As[buf], tid, j, pa.get(j));
      lp_stage_kr(Bs[buf], tid, j, pb.get(j));
    }
  };

  if (nchunks > 0) {
    load(c_begin);
    stage(0);
    load(c_begin + 1);
    lp_barrier();
#pragma unroll 1
    for (int t = 0; t < nchunks; ++t) {
      const int cur = t & 1;
      if (t + 1 < nchunks) {
        stage(1 - cur);
        load(c_begin + t + 2);
      }
#pragma unroll
      for (int ks = 0; ks < LP_T / 32; ++ks) {
        const bf16x8 af = lp_frag_kc(As[cur], wave, ks, lane);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          // B first: D[n][m], a lane holds n = 4 (l / 16) .. + 3 of m = l % 16
          acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              lp_frag_kr(Bs[cur], ni, ks, lane), af, acc[ni], 0, 0, 0);
        }
      }
      lp_barrier();
    }
  }

  const int m = m0 + 16 * wave + (lane & 15);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = n0 + 16 * ni + 4 * (lane >> 4);
    if (m < M && n < N) {
      *reinterpret_cast<f32x4*>(ws + ((long long)blockIdx.z * M + m) * N + n) =
          acc[ni];
    }
  }
}

// xg[i] = bf16(ws[0][i] + .. + ws[S-1][i] + bias[i % N]), four outputs per
// thread and step; n4 = M * N / 4, N % 4 == 0
LP_PRE __global__ void drla_lstm_proj_reduce(const float* __restrict__ ws,
                                             const bf16raw* __restrict__ bias,
                                             bf16raw* __restrict__ xg,
                                             long long n4, int N, int S) {
  const long long stride = (long long)gridDim.x * DRLA_LP_BLOCK;
  for (long long i = (long long)blockIdx.x * DRLA_LP_BLOCK + threadIdx.x;
       i < n4; i += stride) {
    f32x4 sum = *reinterpret_cast<const f32x4*>(ws + 4 * i);
    for (int s = 1; s < S; ++s) {
      const f32x4 v =
          *reinterpret_cast<const f32x4*>(ws + 4 * ((long long)s * n4 + i));
#pragma unroll
      for (int e = 0; e < 4; ++e) sum[e] += v[e];
    }
    // M * N < 2^31 (launcher): 32-bit remainder
    const ushort4v b = *reinterpret_cast<const ushort4v*>(
        bias + (unsigned int)(4 * i) % (unsigned int)N);
#pragma unroll
    for (int e = 0; e < 4; ++e) sum[e] += lp_f32(b[e]);
    *reinterpret_cast<lp_u32x2*>(xg + 4 * i) = lp_round4(sum);
  }
}

// grid (F1 / 64 + ceil(F2 / 64), ceil(M / 64)). dxg [M][N] (lddg), w (ldw)
// -> dconv [M][F1], demb [M][F2], both dense
LP_PRE __global__ void drla_lstm_proj_dgrad(
    const bf16raw* __restrict__ dxg, long long lddg,
    const bf16raw* __restrict__ w, long long ldw, bf16raw* __restrict__ dconv,
    bf16raw* __restrict__ demb, int M, int F1, int F2, int N) {
  __shared__ __attribute__((aligned(16))) unsigned char As[2][LP_KC];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2][LP_KC];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int f0 = blockIdx.x * LP_T, m0 = blockIdx.y * LP_T;
  const int F = F1 + F2;
  const int nchunks = (N + LP_T - 1) / LP_T;

  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};

  LpPiece pa, pb;
  auto load = [&](int c) LP_LAMBDA {
    c = lp_min(c, nchunks - 1);
    pa.load(dxg, lddg, m0, M, LP_T * c, N, tid);
    pb.load(w, ldw, f0, F, LP_T * c, N, tid);
  };
  auto stage = [&](int buf) LP_LAMBDA {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      lp_stage_kc(As[buf], tid, j, pa.get(j));
      lp_stage_kc(Bs[buf], tid, j, pb.get(j));
    }
  };

  load(0);
  stage(0);
  load(1);
  lp_barrier();
#pragma unroll 1
  for (int t = 0; t < nchunks; ++t) {
    const int cur = t & 1;
    if (t + 1 < nchunks) {
      stage(1 - cur);
      load(t + 2);
    }
#pragma unroll
    for (int ks = 0; ks < LP_T / 32; ++ks) {
      const bf16x8 af = lp_frag_kc(As[cur], wave, ks, lane);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            lp_frag_kc(Bs[cur], ni, ks, lane), af, acc[ni], 0, 0, 0);
      }
    }
    lp_barrier();
  }

  if (f0 < F1) {  // block-uniform: the tile is dconv's or demb's
    lp_store_bf16(acc, dconv, F1, m0, M, f0, F1, wave, lane);
  } else {
    lp_store_bf16(acc, demb, F2, m0, M, f0 - F1, F2, wave, lane);
  }
}

// grid ceil((F + H) / 64) * ceil(N / 64). conv [M][F1] (ldc), emb [M][F2]
// (lde), hprev [M][H] dense, dxg [M][N] (lddg) -> dw [F + H][N], db [N]
LP_PRE __global__ void drla_lstm_proj_wgrad(
    const bf16raw* __restrict__ conv, long long ldc,
    const bf16raw* __restrict__ emb, long long lde,
    const bf16raw* __restrict__ hprev, const bf16raw* __restrict__ dxg,
    long long lddg, bf16raw* __restrict__ dw, bf16raw* __restrict__ db, int M,
    int F1, int F2, int H, int N) {
  __shared__ __attribute__((aligned(16))) unsigned char As[2][LP_KR];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2][LP_KR];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int nct = (N + LP_T - 1) / LP_T;
  const int by = blockIdx.x / nct, bx = blockIdx.x % nct;
  const int r0 = by * LP_T, n0 = bx * LP_T;
  const int F = F1 + F2, R = F + H;
  const int nchunks = (M + LP_T - 1) / LP_T;
  const bool with_db = by == 0;  // block-uniform

  // this thread's 8 rows of dW, rp .. rp + 7, lie in one source: F1 and F
  // are multiples of 8
  const int rp = r0 + 8 * (tid & 7);
  const bool from_h = rp >= F;
  const bf16raw* src = rp < F1 ? conv : emb;
  const long long lds_ = rp < F1 ? ldc : lde;
  const int scol = rp < F1 ? r0 : r0 - F1;  // the tile's first column there
  const int sncol = rp < F1 ? F1 : F2;
  // h_prev: four pairs of columns hc + 2 e, H is even
  const int hc = rp - F;
  unsigned int hlive = 0;
  int hoff[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    hlive |= (unsigned int)(from_h && hc + 2 * e < H) << e;
    const int c = lp_min(hc + 2 * e, H - 2);
    hoff[e] = c < 0 ? 0 : c;
  }

  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  LpPiece pa, pb;
  auto load = [&](int c) LP_LAMBDA {
    c = lp_min(c, nchunks - 1);
    if (from_h) {
      pa.live = 0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = LP_T * c + (tid >> 3) + 32 * j;
        pa.live |= (unsigned int)(row < M) << j;
        const bf16raw* q = hprev + (long long)lp_min(row, M - 1) * H;
        lp_u32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned int u =
              *reinterpret_cast<const unsigned int*>(q + hoff[e]);
          v[e] = ((hlive >> e) & 1u) ? u : 0u;
        }
        pa.r[j] = __builtin_bit_cast(bf16x8, v);
      }
    } else {
      pa.load(src, lds_, LP_T * c, M, scol, sncol, tid);
    }
    pb.load(dxg, lddg, LP_T * c, M, n0, N, tid);
  };
  auto stage = [&](int buf) LP_LAMBDA {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      lp_stage_kr(As[buf], tid, j, pa.get(j));
      lp_stage_kr(Bs[buf], tid, j, pb.get(j));
    }
  };

  load(0);
  stage(0);
  load(1);
  lp_barrier();
#pragma unroll 1
  for (int t = 0; t < nchunks; ++t) {
    const int cur = t & 1;
    if (t + 1 < nchunks) {
      stage(1 - cur);
      load(t + 2);
    }
#pragma unroll
    for (int ks = 0; ks < LP_T / 32; ++ks) {
      const bf16x8 af = lp_frag_kr(As[cur], wave, ks, lane);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            lp_frag_kr(Bs[cur], ni, ks, lane), af, acc[ni], 0, 0, 0);
      }
    }
    if (with_db && wave == 0) {  // uniform: lane = column, rows in order
#pragma unroll 16
      for (int r = 0; r < LP_T; ++r) {
        bsum += lp_f32(*reinterpret_cast<const bf16raw*>(
            Bs[cur] + lp_elem_off(r, lane)));
      }
    }
    lp_barrier();
  }

  lp_store_bf16(acc, dw, N, r0, R, n0, N, wave, lane);
  if (with_db && wave == 0 && n0 + lane < N) {
    db[n0 + lane] = (bf16raw)(lp_round2(bsum, 0.f) & 0xffffu);
  }
}
