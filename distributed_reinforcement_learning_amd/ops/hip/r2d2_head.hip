// The R2D2 dueling head: Q = y[:A] - y[A] with y = out(relu(trunk(bf16(h)))),
// trunk H -> 128, out 128 -> A + 1, h f32 from the LSTM sequence kernels,
// bf16 weights read where the two nn.Linear keep them ([out][in]), f32
// accumulation in mfma_f32_16x16x32_bf16, every stored bf16 rounded once.
//
//   drla_r2h_fwd    h -> Q (and the z stash when a gradient is wanted)
//   drla_r2h_bwd    dQ -> dy, dz (bf16, for the weight gradients) and dh (f32)
//   drla_r2h_wgrad  dWt, dbt, dWo, dbo in one launch
//
// The head is 128 .. 640 rows against at most 128 KB of weights: latency
// decides, so each pass is one launch of 16-row blocks that ask for
// everything they can before they use anything.
//
// Forward: the block's 16 x H f32 rows (row n is (n / W, burn + n % W) of
// h_all [B][L][H], so the window form and the contiguous form are one kernel)
// are converted once into a padded bf16 LDS tile. Outputs are computed
// transposed, D[out][row]: the weight is the first MFMA operand and goes from
// global memory straight into registers, wave w holding trunk rows 32 w ..
// 32 w + 31 over the whole k range (up to 128 VGPRs) and wave t out rows
// 16 t .. 16 t + 15; the activation is the 16-byte LDS read. z crosses to
// layer 2 through LDS, the mean row to the value rows through LDS.
//
// Backward: both products reduce over the weight's memory rows (dz = dy . Wo
// over out rows, dh = dz . Wt over trunk rows), so the weights are staged
// row-major in the swizzled 64 x 128-byte image of conv_wgrad_lds.h and read
// back transposed with ds_read_b64_tr_b16: Wo whole (two images), Wt in
// 64-column blocks (two images each), double-buffered, the next block's
// loads in registers while this one is multiplied, one barrier per block.
//
// Weight gradients: 64 x 64 tiles over blockIdx.x, 2 ceil(H / 64) of dWt =
// dz^T . hb and 2 of dWo = dy^T . z (dy is kept 64 wide, zero past A). Both
// operands are k-rows images (the reduction runs over the N rows); hb is
// converted again from the f32 h while staging, with the forward's rounding.
// The tiles of the first column block also add up their dz / dy image column
// by column in row order: those are dbt and dbo. Chunks of 64 rows in order,
// no atomics, no scratch buffer: run-to-run deterministic.
//
// Pieces outside a matrix are loaded from a clamped address and staged as
// zeros; stores are predicated. Packed-f32 VALU ops stay out of this file:
// every function carries NOPK_FN, helpers are drla_nopk.h's (which says why),
// this file's own or builtins.

#include "drla_kernels.h"
#include "drla_nopk.h"

namespace {

constexpr int R2H_MID = DRLA_R2H_MID;
constexpr int R2H_BM = DRLA_R2H_BM;
constexpr int R2H_MAX_KS = DRLA_R2H_MAX_H / 32;  // layer-1 k-steps
constexpr int R2H_H_LD = DRLA_R2H_MAX_H + 8;     // hb rows, elements
constexpr int R2H_Z_LD = R2H_MID + 8;            // z / dz rows, elements
constexpr int R2H_DY_LD = DRLA_R2H_DY_LD + 8;    // dy rows in LDS, elements
static_assert(DRLA_R2H_BLOCK == 256 && R2H_BM == 16 && R2H_MID == 128 &&
                  DRLA_R2H_DY_LD == 64 && DRLA_R2H_MAX_AO == 64,
              "four waves: 32 trunk columns each, one 16-row out tile each; "
              "images are staged by 256 threads in two passes");
static_assert((R2H_H_LD * 2 / 16) % 2 == 1 && (R2H_Z_LD * 2 / 16) % 2 == 1 &&
                  (R2H_DY_LD * 2 / 16) % 2 == 1,
              "odd pitch in 16-byte units: fragment reads spread over banks");

// A thread's share of one 64 k-row x 64 column image of a bf16 matrix:
// rows srow and srow + 32, chunk sch (drla_wg_b_slot<64>)
struct R2hPiece {
  bf16x8 r[2];
  unsigned int live;
};
// k-rows k0 + .. of a [kmax][ld] matrix, columns c0 + 8 sch .. + 7 of cmax
// (a multiple of 8)
NOPK_INL void r2h_load_bf16(R2hPiece& p, const bf16raw* __restrict__ m,
                           long long ld, int k0, int kmax, int c0, int cmax,
                           int tid) {
  const int srow = tid >> 3, c = c0 + 8 * (tid & 7);
  p.live = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = k0 + srow + 32 * j;
    p.live |= (unsigned int)(k < kmax && c < cmax) << j;
    p.r[j] = *reinterpret_cast<const bf16x8*>(
        m + (long long)nopk_min(k, kmax - 1) * ld + nopk_min(c, cmax - 8));
  }
}
// the same out of an f32 matrix, rounded as the forward rounds h
NOPK_INL void r2h_load_f32(R2hPiece& p, const float* __restrict__ m,
                          long long ld, int k0, int kmax, int c0, int cmax,
                          int tid) {
  const int srow = tid >> 3, c = c0 + 8 * (tid & 7);
  f32x4 lo[2], hi[2];
  p.live = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = k0 + srow + 32 * j;
    p.live |= (unsigned int)(k < kmax && c < cmax) << j;
    const float* s = m + (long long)nopk_min(k, kmax - 1) * ld +
                     nopk_min(c, cmax - 8);
    lo[j] = *reinterpret_cast<const f32x4*>(s);
    hi[j] = *reinterpret_cast<const f32x4*>(s + 4);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) p.r[j] = nopk_round8(lo[j], hi[j]);
}
NOPK_INL void r2h_store_piece(const R2hPiece& p, unsigned char* img, int tid) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    nopk_stage_kr(img, tid, j, (p.live >> j) & 1u ? p.r[j] : nopk_zero8());
  }
}

}  // namespace

// ---- forward --------------------------------------------------------------

// grid ceil(N / 16), N = B W rows. h_all [B][L][H] f32, row n at (n / W,
// burn + n % W); wt [128][H], bt [128], wo [A + 1][128], bo [A + 1] ->
// q [N][A]; zs != null: also zs [N][128].
NOPK_PRE(DRLA_R2H_BLOCK) __global__ void drla_r2h_fwd(
    const float* __restrict__ h_all, const bf16raw* __restrict__ wt,
    const bf16raw* __restrict__ bt, const bf16raw* __restrict__ wo,
    const bf16raw* __restrict__ bo, bf16raw* __restrict__ q,
    bf16raw* __restrict__ zs, int N, int W, int L, int burn, int H, int A) {
  __shared__ __attribute__((aligned(16))) bf16raw hb[R2H_BM][R2H_H_LD];
  __shared__ __attribute__((aligned(16))) bf16raw zl[R2H_BM][R2H_Z_LD];
  __shared__ float ym[R2H_BM];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * R2H_BM;
  const int AO = A + 1;
  const int nks = (H + 31) / 32;
  const int kq = 8 * (lane >> 4);  // this lane's k offset within a k-step

  // everything that does not depend on the activations, requested first:
  // the wave's 32 x H slice of Wt, its 16 x 128 tile of Wo, both biases
  bf16x8 f1[R2H_MAX_KS][2];
#pragma unroll
  for (int ks = 0; ks < R2H_MAX_KS; ++ks) {
    if (ks < nks) {  // uniform
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        f1[ks][ni] = *reinterpret_cast<const bf16x8*>(
            wt + (long long)(32 * wave + 16 * ni + (lane & 15)) * H +
            nopk_min(32 * ks + kq, H - 8));
      }
    }
  }
  const bool l2 = 16 * wave < AO;  // wave-uniform: this wave has an out tile
  const int a_row = 16 * wave + (lane & 15);
  bf16x8 f2[R2H_MID / 32];
  bf16raw bias2[4];
  ushort4v bias1[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    bias1[ni] = *reinterpret_cast<const ushort4v*>(bt + 32 * wave + 16 * ni +
                                                   4 * (lane >> 4));
  }
  if (l2) {
#pragma unroll
    for (int kc = 0; kc < R2H_MID / 32; ++kc) {
      f2[kc] = *reinterpret_cast<const bf16x8*>(
          wo + nopk_min(a_row, AO - 1) * R2H_MID + 32 * kc + kq);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bias2[e] = bo[nopk_min(16 * wave + 4 * (lane >> 4) + e, AO - 1)];
    }
  }

  // hb = bf16(h): thread (row tid / 16, chunks tid % 16 + 16 j); k from H to
  // the end of the last k-step is zeros
  {
    const int r = tid >> 4;
    const int n = nopk_min(row0 + r, N - 1);
    const float* src =
        h_all + ((long long)(n / W) * L + burn + n % W) * (long long)H;
    f32x4 lo[4], hi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = nopk_min((tid & 15) + 16 * j, H / 8 - 1);
      lo[j] = *reinterpret_cast<const f32x4*>(src + 8 * c);
      hi[j] = *reinterpret_cast<const f32x4*>(src + 8 * c + 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = (tid & 15) + 16 * j;
      if (c < 4 * nks) {
        *reinterpret_cast<bf16x8*>(&hb[r][8 * c]) =
            (8 * c < H && row0 + r < N) ? nopk_round8(lo[j], hi[j])
                                        : nopk_zero8();
      }
    }
  }
  nopk_barrier();

  // layer 1: D[trunk column][row]
  const int row = lane & 15;
  const bool row_in = row0 + row < N;
  {
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < R2H_MAX_KS; ++ks) {
      if (ks < nks) {
        const bf16x8 bf = nopk_frag_kc(&hb[0][0], R2H_H_LD, 0, ks, lane);
        const bool k_in = 32 * ks + kq < H;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              k_in ? f1[ks][ni] : nopk_zero8(), bf, acc[ni], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int o = 32 * wave + 16 * ni + 4 * (lane >> 4);
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = nopk_relu(acc[ni][e] + nopk_f32(bias1[ni][e]));
      }
      const nopk_u32x2 z = nopk_round4(v);
      *reinterpret_cast<nopk_u32x2*>(&zl[row][o]) = z;
      if (zs && row_in) {
        *reinterpret_cast<nopk_u32x2*>(
            zs + (long long)(row0 + row) * R2H_MID + o) = z;
      }
    }
  }
  nopk_barrier();

  // layer 2: D[out row][row]; the mean row A goes to the other lanes by LDS
  f32x4 y = {0.f, 0.f, 0.f, 0.f};
  if (l2) {
#pragma unroll
    for (int kc = 0; kc < R2H_MID / 32; ++kc) {
      const bf16x8 bf = nopk_frag_kc(&zl[0][0], R2H_Z_LD, 0, kc, lane);
      y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_row < AO ? f2[kc] : nopk_zero8(), bf, y, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] += nopk_f32(bias2[e]);
    if (wave == (A >> 4) && (lane >> 4) == ((A & 15) >> 2)) {
      const int e = A & 3;
      ym[row] = e == 0 ? y[0] : e == 1 ? y[1] : e == 2 ? y[2] : y[3];
    }
  }
  nopk_barrier();
  if (l2 && row_in) {
    const float m = ym[row];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int a = 16 * wave + 4 * (lane >> 4) + e;
      if (a < A) q[(long long)(row0 + row) * A + a] = nopk_round1(y[e] - m);
    }
  }
}

// ---- backward -------------------------------------------------------------

// grid ceil(N / 16). dq [N][A], zs [N][128], wt [128][H], wo [A + 1][128] ->
// dh [N][H] f32, dyg [N][64] (columns past A zero), dzg [N][128]
NOPK_PRE(DRLA_R2H_BLOCK) __global__ void drla_r2h_bwd(
    const bf16raw* __restrict__ dq, const bf16raw* __restrict__ zs,
    const bf16raw* __restrict__ wt, const bf16raw* __restrict__ wo,
    float* __restrict__ dh, bf16raw* __restrict__ dyg,
    bf16raw* __restrict__ dzg, int N, int H, int A) {
  // Wt: [buffer][trunk rows 0..63 | 64..127] images of one 64-column block
  __shared__ __attribute__((aligned(16))) unsigned char wti[2][2 * NOPK_KR_SUB];
  // Wo: [columns 0..63 | 64..127] images, k-rows = out rows (zero past A)
  __shared__ __attribute__((aligned(16))) unsigned char woi[2 * NOPK_KR_SUB];
  __shared__ __attribute__((aligned(16))) bf16raw dyl[R2H_BM][R2H_DY_LD];
  __shared__ __attribute__((aligned(16))) bf16raw dzl[R2H_BM][R2H_Z_LD];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * R2H_BM;
  const int AO = A + 1;
  const int row = lane & 15;  // the row of this lane's accumulators
  const bool row_in = row0 + row < N;
  const long long grow = nopk_min(row0 + row, N - 1);
  const int nkb = (H + 63) / 64;

  // every load that needs no result of this kernel, requested first
  R2hPiece wtp[2], wop[2];
  ushort4v mask[2];
  bf16raw dqv[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    r2h_load_bf16(wtp[i], wt, H, 64 * i, R2H_MID, 0, H, tid);
    r2h_load_bf16(wop[i], wo, R2H_MID, 0, AO, 64 * i, R2H_MID, tid);
    mask[i] = *reinterpret_cast<const ushort4v*>(
        zs + grow * R2H_MID + 32 * wave + 16 * i + 4 * (lane >> 4));
  }
  const int sr = tid >> 4, sc = 4 * (tid & 15);  // dy slot: row, 4 columns
  const bool sr_in = row0 + sr < N;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    dqv[e] = dq[(long long)nopk_min(row0 + sr, N - 1) * A +
                nopk_min(sc + e, A - 1)];
  }

  // dy[:A] = dq, the rest of the 64 columns zero
  {
    ushort4v v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = (sr_in && sc + e < A) ? dqv[e] : (bf16raw)0;
    }
    *reinterpret_cast<ushort4v*>(&dyl[sr][sc]) = v;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    r2h_store_piece(wop[i], woi + i * NOPK_KR_SUB, tid);
    r2h_store_piece(wtp[i], wti[0] + i * NOPK_KR_SUB, tid);
  }
  // the second column block of Wt travels during the dy and dz phases
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    r2h_load_bf16(wtp[i], wt, H, 64 * i, R2H_MID, 64, H, tid);
  }
  nopk_barrier();
  // dy[A] = -sum_a dq[a], f32 in index order, rounded to bf16
  if (tid < R2H_BM) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < DRLA_R2H_DY_LD / 8; ++j) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(&dyl[tid][8 * j]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += nopk_f32((bf16raw)v[e]);
    }
    dyl[tid][A] = nopk_round1(-s);
  }
  nopk_barrier();
  if (sr_in) {
    *reinterpret_cast<ushort4v*>(
        dyg + (long long)(row0 + sr) * DRLA_R2H_DY_LD + sc) =
        *reinterpret_cast<const ushort4v*>(&dyl[sr][sc]);
  }

  // dz = (dy . Wo) masked by z > 0: D[trunk column][row], wave w owns
  // columns 32 w .. 32 w + 31 = tiles 2 (w % 2), + 1 of image w / 2
  {
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const unsigned char* img = woi + (wave >> 1) * NOPK_KR_SUB;
    const int nks = (AO + 31) / 32;
#pragma unroll
    for (int ks = 0; ks < DRLA_R2H_DY_LD / 32; ++ks) {
      if (ks < nks) {  // uniform
        const bf16x8 bf = nopk_frag_kc(&dyl[0][0], R2H_DY_LD, 0, ks, lane);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              nopk_frag_kr(img, 2 * (wave & 1) + ni, ks, lane), bf, acc[ni], 0,
              0, 0);
        }
      }
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int o = 32 * wave + 16 * ni + 4 * (lane >> 4);
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = nopk_pos(mask[ni][e]) ? acc[ni][e] : 0.f;
      }
      const nopk_u32x2 r = nopk_round4(v);
      *reinterpret_cast<nopk_u32x2*>(&dzl[row][o]) = r;
      if (row_in) {
        *reinterpret_cast<nopk_u32x2*>(dzg + grow * R2H_MID + o) = r;
      }
    }
  }
  nopk_barrier();

  // dh = dz . Wt: D[h column][row], one 64-column block of Wt per round,
  // wave w its columns 16 w .. 16 w + 15
  bf16x8 dzf[R2H_MID / 32];
#pragma unroll
  for (int kc = 0; kc < R2H_MID / 32; ++kc) {
    dzf[kc] = nopk_frag_kc(&dzl[0][0], R2H_Z_LD, 0, kc, lane);
  }
#pragma unroll 1
  for (int t = 0; t < nkb; ++t) {
    const int cur = t & 1;
    if (t + 1 < nkb) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        r2h_store_piece(wtp[i], wti[1 - cur] + i * NOPK_KR_SUB, tid);
        r2h_load_bf16(wtp[i], wt, H, 64 * i, R2H_MID, 64 * (t + 2), H, tid);
      }
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < R2H_MID / 32; ++kc) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          nopk_frag_kr(wti[cur] + (kc >> 1) * NOPK_KR_SUB, wave, kc & 1, lane),
          dzf[kc], acc, 0, 0, 0);
    }
    const int k = 64 * t + 16 * wave + 4 * (lane >> 4);
    if (row_in && k < H) {
      *reinterpret_cast<f32x4*>(dh + grow * H + k) = acc;
    }
    nopk_barrier();
  }
}

namespace {

// the b operand of a weight-gradient tile: bf16 or f32 [N][ld]
template <bool B_F32>
NOPK_INL void r2h_load_b(R2hPiece& p, const void* __restrict__ b, int ld,
                        int k0, int N, int n0, int nmax, int tid) {
  if constexpr (B_F32) {
    r2h_load_f32(p, static_cast<const float*>(b), ld, k0, N, n0, nmax, tid);
  } else {
    r2h_load_bf16(p, static_cast<const bf16raw*>(b), ld, k0, N, n0, nmax, tid);
  }
}

// One 64 x 64 tile c[m0 + i][n0 + j] = sum_n a[n][m0 + i] * b[n][n0 + j] over
// the N rows, 64 at a time in order; a is bf16 [N][lda], b is bf16 or f32
// [N][ldb] and c is [mmax][ldb], both nmax columns wide. Rows < mmax and
// columns < nmax are stored. bias != null: also bias[m0 + i] = sum_n
// a[n][m0 + i]. lds: [2 operands][2 buffers] images.
template <bool B_F32>
NOPK_INL void r2h_wgrad_tile(unsigned char* lds, const bf16raw* __restrict__ a,
                            int lda, const void* __restrict__ b, int ldb,
                            int n0, int nmax, bf16raw* __restrict__ c, int m0,
                            int mmax, bf16raw* __restrict__ bias, int N) {
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  unsigned char* As = lds;
  unsigned char* Bs = lds + 2 * NOPK_KR_SUB;
  R2hPiece pa, pb;
  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const int nchunks = (N + DRLA_WG_ROWS - 1) / DRLA_WG_ROWS;

  r2h_load_bf16(pa, a, lda, 0, N, m0, lda, tid);
  r2h_load_b<B_F32>(pb, b, ldb, 0, N, n0, nmax, tid);
  r2h_store_piece(pa, As, tid);
  r2h_store_piece(pb, Bs, tid);
  r2h_load_bf16(pa, a, lda, DRLA_WG_ROWS, N, m0, lda, tid);
  r2h_load_b<B_F32>(pb, b, ldb, DRLA_WG_ROWS, N, n0, nmax, tid);
  nopk_barrier();
#pragma unroll 1
  for (int t = 0; t < nchunks; ++t) {
    const int cur = t & 1;
    if (t + 1 < nchunks) {
      const int k0 = (t + 2) * DRLA_WG_ROWS;
      r2h_store_piece(pa, As + (1 - cur) * NOPK_KR_SUB, tid);
      r2h_store_piece(pb, Bs + (1 - cur) * NOPK_KR_SUB, tid);
      r2h_load_bf16(pa, a, lda, k0, N, m0, lda, tid);
      r2h_load_b<B_F32>(pb, b, ldb, k0, N, n0, nmax, tid);
    }
#pragma unroll
    for (int ks = 0; ks < DRLA_WG_ROWS / 32; ++ks) {
      const bf16x8 af = nopk_frag_kr(As + cur * NOPK_KR_SUB, wave, ks, lane);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        // B first: D[n][m], a lane holds n = 4 (l / 16) .. + 3 of m = l % 16
        acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            nopk_frag_kr(Bs + cur * NOPK_KR_SUB, ni, ks, lane), af, acc[ni], 0, 0,
            0);
      }
    }
    if (bias && wave == 0) {  // uniform: lane = column, rows in order
#pragma unroll 16
      for (int r = 0; r < DRLA_WG_ROWS; ++r) {
        bsum += nopk_f32(*reinterpret_cast<const bf16raw*>(
            As + cur * NOPK_KR_SUB + nopk_elem_off(r, lane)));
      }
    }
    nopk_barrier();
  }

  const int m = m0 + 16 * wave + (lane & 15);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = n0 + 16 * ni + 4 * (lane >> 4);
    if (m < mmax && n < nmax) {
      *reinterpret_cast<nopk_u32x2*>(c + (long long)m * ldb + n) =
          nopk_round4(acc[ni]);
    }
  }
  if (bias && wave == 0 && m0 + lane < mmax) {
    bias[m0 + lane] = nopk_round1(bsum);
  }
}

}  // namespace

// grid 2 ceil(H / 64) + 2. h [N][H] f32, zs [N][128], dyg [N][64], dzg
// [N][128] -> dwt [128][H], dbt [128], dwo [A + 1][128], dbo [A + 1]
NOPK_PRE(DRLA_R2H_BLOCK) __global__ void drla_r2h_wgrad(
    const float* __restrict__ h, const bf16raw* __restrict__ zs,
    const bf16raw* __restrict__ dyg, const bf16raw* __restrict__ dzg,
    bf16raw* __restrict__ dwt, bf16raw* __restrict__ dbt,
    bf16raw* __restrict__ dwo, bf16raw* __restrict__ dbo, int N, int H,
    int A) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * NOPK_KR_SUB];
  const int nk = (H + 63) / 64;
  const int job = blockIdx.x;
  if (job < 2 * nk) {  // block-uniform
    const int by = job / nk, bx = job % nk;
    r2h_wgrad_tile<true>(lds, dzg, R2H_MID, h, H, 64 * bx, H, dwt, 64 * by,
                         R2H_MID, bx == 0 ? dbt : nullptr, N);
  } else {
    const int bx = job - 2 * nk;
    r2h_wgrad_tile<false>(lds, dyg, DRLA_R2H_DY_LD, zs, R2H_MID, 64 * bx,
                          R2H_MID, dwo, 0, A + 1, bx == 0 ? dbo : nullptr, N);
  }
}
