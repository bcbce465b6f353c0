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
// Packed-f32 VALU ops stay out of this file: every function carries NOPK_FN,
// helpers are drla_nopk.h's (which says why), this file's own or builtins.

#include "drla_kernels.h"
#include "drla_nopk.h"

namespace {

constexpr int LP_T = DRLA_LP_TILE;        // tile edge and chunk depth
static_assert(LP_T == NOPK_BK && DRLA_LP_BLOCK == 256,
              "the tiles of drla_nopk.h: 64 k x 64 columns, staged by 256 "
              "threads in two passes");

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
  NOPK_INL void load(const bf16raw* __restrict__ p, long long ld, int r0,
                   int nrows, int c0, int ncols, int tid) {
    const int c = c0 + 8 * (tid & 7);
    const long long coff = nopk_min(c, ncols - 8);
    live = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = r0 + (tid >> 3) + 32 * j;
      live |= (unsigned int)(row < nrows && c < ncols) << j;
      r[j] = *reinterpret_cast<const bf16x8*>(
          p + (long long)nopk_min(row, nrows - 1) * ld + coff);
    }
  }
  NOPK_INL bf16x8 get(int j) const {
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    return ((live >> j) & 1u) ? r[j] : z;
  }
};

// the epilogue all three products share: wave's 16-row tile, lane's row
// l % 16 and four columns 4 (l / 16) .. + 3 of each 16-column tile
NOPK_INL void lp_store_bf16(const f32x4 (&acc)[4], bf16raw* __restrict__ c,
                          long long ldc, int m0, int mmax, int n0, int nmax,
                          int wave, int lane) {
  const int m = m0 + 16 * wave + (lane & 15);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = n0 + 16 * ni + 4 * (lane >> 4);
    if (m < mmax && n < nmax) {  // nmax % 8 == 0: four columns in or out
      *reinterpret_cast<nopk_u32x2*>(c + (long long)m * ldc + n) =
          nopk_round4(acc[ni]);
    }
  }
}

}  // namespace

// grid (ceil(N / 64), ceil(M / 64), S). conv [M][F1] (row stride ldc), emb
// [M][F2] (lde), w [F1 + F2 ..][N] (ldw) -> ws [S][M][N] f32
NOPK_PRE(DRLA_LP_BLOCK) __global__ void drla_lstm_proj_fwd(
    const bf16raw* __restrict__ conv, long long ldc,
    const bf16raw* __restrict__ emb, long long lde,
    const bf16raw* __restrict__ w, long long ldw, float* __restrict__ ws,
    int M, int F1, int F2, int N) {
  __shared__ __attribute__((aligned(16))) unsigned char As[2][NOPK_KC_SUB];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2][NOPK_KR_SUB];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int n0 = blockIdx.x * LP_T, m0 = blockIdx.y * LP_T;
  const int F = F1 + F2;
  const int nc1 = F1 / LP_T;
  const int chunks = nc1 + (F2 + LP_T - 1) / LP_T;
  const int per = (chunks + (int)gridDim.z - 1) / (int)gridDim.z;
  const int c_begin = nopk_min((int)blockIdx.z * per, chunks);
  const int nchunks = nopk_min(c_begin + per, chunks) - c_begin;

  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};

  LpPiece pa, pb;
  // chunk c of the whole product; past the last one the addresses are the
  // last chunk's and the registers are never staged
  auto load = [&](int c) NOPK_LAMBDA {
    c = nopk_min(c, chunks - 1);
    if (c < nc1) {  // block-uniform
      pa.load(conv, ldc, m0, M, LP_T * c, F1, tid);
    } else {
      pa.load(emb, lde, m0, M, LP_T * (c - nc1), F2, tid);
    }
    pb.load(w, ldw, LP_T * c, F, n0, N, tid);
  };
  auto stage = [&](int buf) NOPK_LAMBDA {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      nopk_stage_kc(As[buf], tid, j, pa.get(j));
      nopk_stage_kr(Bs[buf], tid, j, pb.get(j));
    }
  };

  if (nchunks > 0) {
    load(c_begin);
    stage(0);
    load(c_begin + 1);
    nopk_barrier();
#pragma unroll 1
    for (int t = 0; t < nchunks; ++t) {
      const int cur = t & 1;
      if (t + 1 < nchunks) {
        stage(1 - cur);
        load(c_begin + t + 2);
      }
#pragma unroll
      for (int ks = 0; ks < LP_T / 32; ++ks) {
        const bf16x8 af = nopk_frag_kc(As[cur], NOPK_PITCH, wave, ks, lane);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          // B first: D[n][m], a lane holds n = 4 (l / 16) .. + 3 of m = l % 16
          acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              nopk_frag_kr(Bs[cur], ni, ks, lane), af, acc[ni], 0, 0, 0);
        }
      }
      nopk_barrier();
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

// xg[i] = bf16(ws[0][i] + .. + ws[S-1][i] + bias[i % N]); n4 = M * N / 4
NOPK_PRE(DRLA_LP_BLOCK) __global__ void drla_lstm_proj_reduce(
    const float* __restrict__ ws, const bf16raw* __restrict__ bias,
    bf16raw* __restrict__ xg, long long n4, int N, int S) {
  nopk_split_reduce<DRLA_LP_BLOCK, true>(ws, bias, xg, n4, N, S);
}

// grid (F1 / 64 + ceil(F2 / 64), ceil(M / 64)). dxg [M][N] (lddg), w (ldw)
// -> dconv [M][F1], demb [M][F2], both dense
NOPK_PRE(DRLA_LP_BLOCK) __global__ void drla_lstm_proj_dgrad(
    const bf16raw* __restrict__ dxg, long long lddg,
    const bf16raw* __restrict__ w, long long ldw, bf16raw* __restrict__ dconv,
    bf16raw* __restrict__ demb, int M, int F1, int F2, int N) {
  __shared__ __attribute__((aligned(16))) unsigned char As[2][NOPK_KC_SUB];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2][NOPK_KC_SUB];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int f0 = blockIdx.x * LP_T, m0 = blockIdx.y * LP_T;
  const int F = F1 + F2;
  const int nchunks = (N + LP_T - 1) / LP_T;

  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};

  LpPiece pa, pb;
  auto load = [&](int c) NOPK_LAMBDA {
    c = nopk_min(c, nchunks - 1);
    pa.load(dxg, lddg, m0, M, LP_T * c, N, tid);
    pb.load(w, ldw, f0, F, LP_T * c, N, tid);
  };
  auto stage = [&](int buf) NOPK_LAMBDA {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      nopk_stage_kc(As[buf], tid, j, pa.get(j));
      nopk_stage_kc(Bs[buf], tid, j, pb.get(j));
    }
  };

  load(0);
  stage(0);
  load(1);
  nopk_barrier();
#pragma unroll 1
  for (int t = 0; t < nchunks; ++t) {
    const int cur = t & 1;
    if (t + 1 < nchunks) {
      stage(1 - cur);
      load(t + 2);
    }
#pragma unroll
    for (int ks = 0; ks < LP_T / 32; ++ks) {
      const bf16x8 af = nopk_frag_kc(As[cur], NOPK_PITCH, wave, ks, lane);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            nopk_frag_kc(Bs[cur], NOPK_PITCH, ni, ks, lane), af, acc[ni], 0, 0, 0);
      }
    }
    nopk_barrier();
  }

  if (f0 < F1) {  // block-uniform: the tile is dconv's or demb's
    lp_store_bf16(acc, dconv, F1, m0, M, f0, F1, wave, lane);
  } else {
    lp_store_bf16(acc, demb, F2, m0, M, f0 - F1, F2, wave, lane);
  }
}

// grid ceil((F + H) / 64) * ceil(N / 64). conv [M][F1] (ldc), emb [M][F2]
// (lde), hprev [M][H] dense, dxg [M][N] (lddg) -> dw [F + H][N], db [N]
NOPK_PRE(DRLA_LP_BLOCK) __global__ void drla_lstm_proj_wgrad(
    const bf16raw* __restrict__ conv, long long ldc,
    const bf16raw* __restrict__ emb, long long lde,
    const bf16raw* __restrict__ hprev, const bf16raw* __restrict__ dxg,
    long long lddg, bf16raw* __restrict__ dw, bf16raw* __restrict__ db, int M,
    int F1, int F2, int H, int N) {
  __shared__ __attribute__((aligned(16))) unsigned char As[2][NOPK_KR_SUB];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2][NOPK_KR_SUB];
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
    const int c = nopk_min(hc + 2 * e, H - 2);
    hoff[e] = c < 0 ? 0 : c;
  }

  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  LpPiece pa, pb;
  auto load = [&](int c) NOPK_LAMBDA {
    c = nopk_min(c, nchunks - 1);
    if (from_h) {
      pa.live = 0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = LP_T * c + (tid >> 3) + 32 * j;
        pa.live |= (unsigned int)(row < M) << j;
        const bf16raw* q = hprev + (long long)nopk_min(row, M - 1) * H;
        nopk_u32x4 v;
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
  auto stage = [&](int buf) NOPK_LAMBDA {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      nopk_stage_kr(As[buf], tid, j, pa.get(j));
      nopk_stage_kr(Bs[buf], tid, j, pb.get(j));
    }
  };

  load(0);
  stage(0);
  load(1);
  nopk_barrier();
#pragma unroll 1
  for (int t = 0; t < nchunks; ++t) {
    const int cur = t & 1;
    if (t + 1 < nchunks) {
      stage(1 - cur);
      load(t + 2);
    }
#pragma unroll
    for (int ks = 0; ks < LP_T / 32; ++ks) {
      const bf16x8 af = nopk_frag_kr(As[cur], wave, ks, lane);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            nopk_frag_kr(Bs[cur], ni, ks, lane), af, acc[ni], 0, 0, 0);
      }
    }
    if (with_db && wave == 0) {  // uniform: lane = column, rows in order
#pragma unroll 16
      for (int r = 0; r < LP_T; ++r) {
        bsum += nopk_f32(*reinterpret_cast<const bf16raw*>(
            Bs[cur] + nopk_elem_off(r, lane)));
      }
    }
    nopk_barrier();
  }

  lp_store_bf16(acc, dw, N, r0, R, n0, N, wave, lane);
  if (with_db && wave == 0 && n0 + lane < N) {
    db[n0 + lane] = (bf16raw)(nopk_round2(bsum, 0.f) & 0xffffu);
  }
}
