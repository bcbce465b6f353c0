// The Ape-X dueling Q head: Q = value_branch(feat) - mean_branch(feat), both
// branches K -> 256 -> 256 -> {A, 1} with ReLU, bf16 in and out, f32
// accumulation in mfma_f32_16x16x32_bf16, every stored value rounded once.
// Weights are read where nn.Linear keeps them ([out][in], in-contiguous).
//
//   drla_dq_l1_fwd    P[s][N][512] = feat[N, K_s] . [W1v ; W1m][:, K_s]^T
//   drla_dq_tail_fwd  z1 = relu(sum_s P + b1), z2 = relu(z1 W2^T + b2),
//                     Q = (z2v W3v^T + b3v) - (z2m W3m^T + b3m)
//   drla_dq_tail_bwd  d3 -> dz2 -> dz1 for both branches
//   drla_dq_wgrad     six dW and six db in one launch
//   drla_dq_l1_dgrad  dfeat = dz1v . W1v + dz1m . W1m
//
// Two designs share the file.
//
// The three products with a long dimension (l1_fwd streams 2 x 256 x K
// weights, wgrad writes as many, l1_dgrad reads them again) are 64 x 64 block
// tiles of 256 threads, wave w owning rows 16 w .. 16 w + 15 (dq_product).
// An operand is k-contiguous (staged as padded [64][64 + 8] rows, read as
// 16-byte fragments) or k-rows (a memory row is one k: staged row-major in
// the swizzled 64 x 128-byte image of conv_wgrad_lds.h and read back
// transposed with ds_read_b64_tr_b16). Global loads run one 64-k chunk ahead
// in registers, the LDS images are double-buffered, one barrier per chunk.
// An operand may be two matrices end to end along k (kseg): that is how
// l1_dgrad runs both branches through one accumulator. Pieces outside a
// matrix are loaded from a clamped address and staged as zeros, so no load
// sits behind a branch and EXEC is full at the transposed reads.
//
// l1_fwd is weight streaming (N <= 64 rows against 3.5 MB), so its grid
// splits the 512 columns and K: grid.z = S splits, each block stores its
// whole f32 tile to ws[z][N][512]. No zero-fill, no atomics; the tail's
// prologue adds the S slices in index order. With a gradient wanted its
// blocks also write the transposed W2 / W3v the backward tail reads.
//
// The two tails keep a 16-row block's activations in LDS and walk both
// branches: 8 waves, wave w = branch w / 4, output columns 64 (w % 4) .. + 63.
// Output is computed transposed (D[out][row]) so the weight is the first MFMA
// operand, read straight from global memory into registers, a whole 256 x 64
// slice requested before first use; the activation is the 16-byte LDS read.
// A lane then holds four consecutive outputs of one row: one 8-byte store.
//
// Packed-f32 VALU ops stay out of this file: every function carries NOPK_FN,
// helpers are drla_nopk.h's (which says why), this file's own or builtins.

#include "drla_kernels.h"
#include "drla_nopk.h"

namespace {

constexpr int DQ_H = DRLA_DQ_HID;
constexpr int DQ_ACT_LD = DQ_H + 8;        // tail activation rows, elements
static_assert(DRLA_DQ_BLOCK == 256,
              "the tiles of drla_nopk.h are staged by 256 threads in two "
              "passes");
static_assert((DQ_ACT_LD * 2 / 16) % 2 == 1,
              "odd pitch in 16-byte units: fragment reads spread over banks");
static_assert(DRLA_DQ_TAIL_BLOCK == 2 * 4 * 64 && DQ_H == 4 * 64,
              "tail: two branches x four waves x 64 output columns");
static_assert(DRLA_DQ_MAX_A == 32 && DRLA_DQ_BM == 16,
              "layer 3 is one 32-deep k-step backward, two 16-row tiles "
              "forward");

// ---- the tiled product ----------------------------------------------------

// An operand: k in [0, kseg) comes from p0, k in [kseg, 2 kseg) from p1 (p1 =
// p0 for a single matrix: the prefetch past the end then stays on it).
struct DqOperand {
  const bf16raw* p0;
  const bf16raw* p1;
  long long ld;
  int kseg;
};

// One operand's 64 (rows or columns) x 64 k tile. Thread slot: LDS row
// srow + 32 j (pass j = 0, 1), 16-byte chunk sch: drla_wg_b_slot<64>.
template <bool KROWS>
struct DqTile {
  DqOperand g;
  int srow, sch;
  long long off[2];    // clamped element offset of the non-k index
  unsigned int live;   // bit j: that piece's non-k index is inside
  unsigned int klive;  // bit j: the loaded chunk's k is inside
  bf16x8 r[2];         // the chunk in flight

  // tile0: first row (k-contiguous) / column (k-rows) of the tile; nmax: how
  // many the matrix has (k-rows: a multiple of 8)
  NOPK_INL void init(const DqOperand& g_, int tile0, int nmax, int tid) {
    g = g_;
    srow = tid >> 3;
    sch = tid & 7;
    live = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if constexpr (KROWS) {
        const int c = tile0 + 8 * sch;
        live |= (unsigned int)(c < nmax) << j;
        off[j] = nopk_min(c, nmax - 8);
      } else {
        const int row = tile0 + srow + 32 * j;
        live |= (unsigned int)(row < nmax) << j;
        off[j] = (long long)nopk_min(row, nmax - 1) * g.ld;
      }
    }
  }

  // global -> registers for the chunk at k0 of a range that ends at k_end
  NOPK_INL void load(int k0, int k_end) {
    const bool second = k0 >= g.kseg;
    const bf16raw* p = second ? g.p1 : g.p0;
    const int kb = k0 - (second ? g.kseg : 0);
    const int ke = nopk_min(k_end - (second ? g.kseg : 0), g.kseg);
    klive = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      long long koff;
      if constexpr (KROWS) {
        const int k = kb + srow + 32 * j;
        klive |= (unsigned int)(k < ke) << j;
        koff = (long long)nopk_min(k, g.kseg - 1) * g.ld;
      } else {
        const int k = kb + 8 * sch;
        klive |= (unsigned int)(k < ke) << j;
        koff = nopk_min(k, g.kseg - 8);
      }
      r[j] = *reinterpret_cast<const bf16x8*>(p + off[j] + koff);
    }
  }

  // registers -> LDS image; pieces outside the matrix or the range are zeros
  NOPK_INL void store(unsigned char* lds) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool in = ((live >> j) & (klive >> j) & 1u) != 0;
      const int o = KROWS ? nopk_chunk_off(srow + 32 * j, sch)
                          : (srow + 32 * j) * NOPK_PITCH + 16 * sch;
      *reinterpret_cast<bf16x8*>(lds + o) = in ? r[j] : nopk_zero8();
    }
  }

  // 16x16x32 operand of 16-wide tile t16, k-step ks: lane l gets element
  // (t16 * 16 + l % 16, 32 ks + 8 (l / 16) + e) in e = 0..7. EXEC is full.
  static NOPK_INL bf16x8 frag(const unsigned char* lds, int t16, int ks,
                            int lane) {
    if constexpr (KROWS) {
      return nopk_frag_kr(lds, t16, ks, lane);
    } else {
      return nopk_frag_kc(lds, NOPK_PITCH, t16, ks, lane);
    }
  }
};

// acc = A[m0 .. m0+63][k] . B[k][n0 .. n0+63] over k in [k_begin, k_end),
// k_begin a multiple of 64. The calling wave's 16 rows are m0 + 16 wave +
// l % 16; acc[ni][e] is column n0 + 16 ni + 4 (l / 16) + e. Rows at or past
// mmax and columns at or past nmax contribute zeros. Every thread of the
// block calls it with the same arguments. lds: [2][2][NOPK_SUB].
template <bool A_KROWS, bool B_KROWS>
NOPK_INL void dq_product(f32x4 (&acc)[4], unsigned char* lds,
                       const DqOperand& a, int m0, int mmax,
                       const DqOperand& b, int n0, int nmax, int k_begin,
                       int k_end) {
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  unsigned char* As = lds;
  unsigned char* Bs = lds + 2 * NOPK_SUB;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};
  const int nchunks = k_end > k_begin ? (k_end - k_begin + NOPK_BK - 1) / NOPK_BK
                                      : 0;
  if (nchunks == 0) return;

  DqTile<A_KROWS> ta;
  DqTile<B_KROWS> tb;
  ta.init(a, m0, mmax, tid);
  tb.init(b, n0, nmax, tid);
  ta.load(k_begin, k_end);
  tb.load(k_begin, k_end);
  ta.store(As);
  tb.store(Bs);
  ta.load(k_begin + NOPK_BK, k_end);
  tb.load(k_begin + NOPK_BK, k_end);
  nopk_barrier();
#pragma unroll 1
  for (int t = 0; t < nchunks; ++t) {
    const int cur = t & 1;
    if (t + 1 < nchunks) {
      ta.store(As + (1 - cur) * NOPK_SUB);
      tb.store(Bs + (1 - cur) * NOPK_SUB);
      ta.load(k_begin + (t + 2) * NOPK_BK, k_end);
      tb.load(k_begin + (t + 2) * NOPK_BK, k_end);
    }
#pragma unroll
    for (int ks = 0; ks < NOPK_BK / 32; ++ks) {
      const bf16x8 af =
          DqTile<A_KROWS>::frag(As + cur * NOPK_SUB, wave, ks, lane);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const bf16x8 bf =
            DqTile<B_KROWS>::frag(Bs + cur * NOPK_SUB, ni, ks, lane);
        // B first: D[n][m], a lane holds n = 4 (l / 16) .. + 3 of m = l % 16
        acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, af, acc[ni], 0,
                                                          0, 0);
      }
    }
    nopk_barrier();
  }
}

// bf16 store of a wave's 16 x 64 slice of a tile to c (row stride ldc); rows
// < mmax and columns < nmax (a multiple of 8) only
NOPK_INL void dq_store_tile(const f32x4 (&acc)[4], bf16raw* __restrict__ c,
                          long long ldc, int m0, int mmax, int n0, int nmax) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = m0 + wave * 16 + (lane & 15);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = n0 + ni * 16 + (lane >> 4) * 4;
    if (m < mmax && n < nmax) {
      *reinterpret_cast<nopk_u32x2*>(c + (long long)m * ldc + n) =
          nopk_round4(acc[ni]);
    }
  }
}

// ---- the tails' per-wave pieces -------------------------------------------

// A wave's slice of a [256][256] first operand: rows out0 + 16 ni + l % 16,
// all eight 32-deep k-steps (128 VGPRs), requested together
struct DqW256 {
  bf16x8 a[DQ_H / 32][4];
};
NOPK_INL void dq_load_w256(DqW256& f, const bf16raw* __restrict__ w, int out0,
                         int lane) {
#pragma unroll
  for (int kc = 0; kc < DQ_H / 32; ++kc) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      f.a[kc][ni] = *reinterpret_cast<const bf16x8*>(
          w + (out0 + ni * 16 + (lane & 15)) * DQ_H + kc * 32 +
          (lane >> 4) * 8);
    }
  }
}
// acc[ni] = D[out0 + 16 ni + 4 (l / 16) + e][row l % 16] over the 256 k of
// act [16][DQ_ACT_LD]
NOPK_INL void dq_mma256(f32x4 (&acc)[4], const DqW256& f,
                      const bf16raw (*act)[DQ_ACT_LD], int lane) {
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kc = 0; kc < DQ_H / 32; ++kc) {
    const bf16x8 bf = *reinterpret_cast<const bf16x8*>(
        &act[lane & 15][kc * 32 + (lane >> 4) * 8]);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[kc][ni], bf,
                                                        acc[ni], 0, 0, 0);
    }
  }
}
// the four values a lane's acc[ni] goes with, of a [rows][256] bf16 matrix
// row (bias: row 0) - one 8-byte load per ni
NOPK_INL void dq_load_side(ushort4v (&s)[4], const bf16raw* __restrict__ row,
                         int out0, int lane) {
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    s[ni] = *reinterpret_cast<const ushort4v*>(row + out0 + ni * 16 +
                                               (lane >> 4) * 4);
  }
}

}  // namespace

// ---- forward --------------------------------------------------------------

// grid (8, ceil(N / 64), S). feat [N][K] (row stride ldf), w1v / w1m [256][K]
// -> ws [S][N][512] f32. w2t != null: also w2t [2][256][256] = W2{v,m}^T and
// w3t [256][32] = W3v^T, columns >= A zero, every block its share.
NOPK_PRE(DRLA_DQ_BLOCK) __global__ void drla_dq_l1_fwd(
    const bf16raw* __restrict__ feat, long long ldf,
    const bf16raw* __restrict__ w1v, const bf16raw* __restrict__ w1m,
    float* __restrict__ ws, int N, int K, const bf16raw* __restrict__ w2v,
    const bf16raw* __restrict__ w2m, const bf16raw* __restrict__ w3v, int A,
    bf16raw* __restrict__ w2t, bf16raw* __restrict__ w3t) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * NOPK_SUB];
  const int tid = threadIdx.x;

  if (w2t) {
    const int nt = (int)(gridDim.x * gridDim.y * gridDim.z) * DRLA_DQ_BLOCK;
    const int gt = (int)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x +
                         blockIdx.x) * DRLA_DQ_BLOCK + tid;
    // a unit is 8 consecutive k of one W2 row: a 16-byte load, 8 stores that
    // run along the lanes (consecutive lanes = consecutive rows)
    for (int u = gt; u < 2 * 8192; u += nt) {
      const int c = u >> 13, row = u & 255, k0 = ((u >> 8) & 31) * 8;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(
          (c ? w2m : w2v) + row * DQ_H + k0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        w2t[c * DQ_H * DQ_H + (k0 + j) * DQ_H + row] = (bf16raw)v[j];
      }
    }
    for (int e = gt; e < DQ_H * DRLA_DQ_MAX_A; e += nt) {
      const int a = e & (DRLA_DQ_MAX_A - 1), i = e >> 5;
      w3t[e] = a < A ? w3v[a * DQ_H + i] : (bf16raw)0;
    }
  }

  // the split's k range, in whole chunks; an empty one stores zeros
  const int chunks = (K + NOPK_BK - 1) / NOPK_BK;
  const int per = (chunks + (int)gridDim.z - 1) / (int)gridDim.z;
  const int k_begin = nopk_min((int)blockIdx.z * per, chunks) * NOPK_BK;
  const int k_end = nopk_min(k_begin + per * NOPK_BK, K);
  const int m0 = blockIdx.y * 64;
  const int n0 = blockIdx.x * 64;  // column of [W1v ; W1m]
  const bf16raw* w1 = n0 < DQ_H ? w1v : w1m;

  f32x4 acc[4];
  dq_product<false, false>(acc, lds, DqOperand{feat, feat, ldf, K}, m0, N,
                           DqOperand{w1, w1, K, K}, n0 & (DQ_H - 1), DQ_H,
                           k_begin, k_end);

  const int m = m0 + (tid >> 6) * 16 + (tid & 15);
  if (m < N) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + ni * 16 + ((tid & 63) >> 4) * 4;
      *reinterpret_cast<f32x4*>(
          ws + ((long long)blockIdx.z * N + m) * (2 * DQ_H) + n) = acc[ni];
    }
  }
}

// grid ceil(N / 16). ws [S][N][512] -> q [N][A]; z1s != null: also z1s, z2s
// [2][G][256], rows < G.
NOPK_PRE(DRLA_DQ_TAIL_BLOCK) __global__ void drla_dq_tail_fwd(
    const float* __restrict__ ws, int S, const bf16raw* __restrict__ b1v,
    const bf16raw* __restrict__ b1m, const bf16raw* __restrict__ w2v,
    const bf16raw* __restrict__ b2v, const bf16raw* __restrict__ w2m,
    const bf16raw* __restrict__ b2m, const bf16raw* __restrict__ w3v,
    const bf16raw* __restrict__ b3v, const bf16raw* __restrict__ w3m,
    const bf16raw* __restrict__ b3m, bf16raw* __restrict__ q,
    bf16raw* __restrict__ z1s, bf16raw* __restrict__ z2s, int N, int A,
    int G) {
  __shared__ __attribute__((aligned(16))) bf16raw z1[2][DRLA_DQ_BM][DQ_ACT_LD];
  __shared__ __attribute__((aligned(16))) bf16raw z2[2][DRLA_DQ_BM][DQ_ACT_LD];
  __shared__ float ym[DRLA_DQ_BM];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int c = wave >> 2, wq = wave & 3;  // branch, quarter of its columns
  const int out0 = wq * 64;
  const int row0 = blockIdx.x * DRLA_DQ_BM;

  // everything that does not depend on the activations, requested first
  DqW256 f2;
  ushort4v bias2[4];
  dq_load_w256(f2, c ? w2m : w2v, out0, lane);
  dq_load_side(bias2, c ? b2m : b2v, out0, lane);
  // layer 3: branch v's quarters 0 and 1 own outputs 0..15 and 16..31, branch
  // m's quarter 0 owns its one output; rows of W3 past the end are zeros
  const int n3 = c ? 1 : A;
  const bool l3 = wq * 16 < n3;  // wave-uniform
  bf16x8 f3[DQ_H / 32];
  bf16raw bias3[4];
  if (l3) {
    const int a = wq * 16 + (lane & 15);
    const bf16raw* w3 = (c ? w3m : w3v) + nopk_min(a, n3 - 1) * DQ_H;
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int kc = 0; kc < DQ_H / 32; ++kc) {
      const bf16x8 v =
          *reinterpret_cast<const bf16x8*>(w3 + kc * 32 + (lane >> 4) * 8);
      f3[kc] = a < n3 ? v : z;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bias3[e] =
          (c ? b3m : b3v)[nopk_min(wq * 16 + (lane >> 4) * 4 + e, n3 - 1)];
    }
  }

  // prologue: z1 = relu(sum_s ws[s] + b1) for 16 rows x 512 columns; a thread
  // has 16 consecutive columns of one row
  {
    const int row = tid >> 5, col0 = (tid & 31) * 16;
    const int cc = col0 >> 8, cl = col0 & (DQ_H - 1);
    const int grow = nopk_min(row0 + row, N - 1);
    const bf16raw* b1 = (cc ? b1m : b1v) + cl;
    const bf16x8 blo = *reinterpret_cast<const bf16x8*>(b1);
    const bf16x8 bhi = *reinterpret_cast<const bf16x8*>(b1 + 8);
    const float* p = ws + (long long)grow * (2 * DQ_H) + col0;
    f32x4 sum[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] = *reinterpret_cast<const f32x4*>(p + 4 * j);
    // two slices' loads in flight per round (the second from a clamped
    // slice, dropped when it is past the end), added in index order
    const long long slice = (long long)N * (2 * DQ_H);
    for (int s = 1; s < S; s += 2) {
      const bool two = s + 1 < S;
      const float* pa = p + s * slice;
      const float* pb = p + (two ? s + 1 : s) * slice;
      f32x4 va[4], vb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        va[j] = *reinterpret_cast<const f32x4*>(pa + 4 * j);
        vb[j] = *reinterpret_cast<const f32x4*>(pb + 4 * j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sum[j][e] += va[j][e];
          sum[j][e] += two ? vb[j][e] : 0.f;
        }
      }
    }
    nopk_u32x2 o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * j + e;
        const bf16raw b = (bf16raw)(i < 8 ? blo[i & 7] : bhi[i & 7]);
        v[e] = nopk_relu(sum[j][e] + nopk_f32(b));
      }
      o[j] = nopk_round4(v);
    }
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    const u32x4 lo = {o[0][0], o[0][1], o[1][0], o[1][1]};
    const u32x4 hi = {o[2][0], o[2][1], o[3][0], o[3][1]};
    *reinterpret_cast<u32x4*>(&z1[cc][row][cl]) = lo;
    *reinterpret_cast<u32x4*>(&z1[cc][row][cl + 8]) = hi;
    if (z1s && row0 + row < G) {
      bf16raw* d = z1s + ((long long)cc * G + row0 + row) * DQ_H + cl;
      *reinterpret_cast<u32x4*>(d) = lo;
      *reinterpret_cast<u32x4*>(d + 8) = hi;
    }
  }
  nopk_barrier();

  // layer 2
  {
    f32x4 acc[4];
    dq_mma256(acc, f2, z1[c], lane);
    const int row = lane & 15;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int o = out0 + ni * 16 + (lane >> 4) * 4;
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = nopk_relu(acc[ni][e] + nopk_f32(bias2[ni][e]));
      }
      const nopk_u32x2 r = nopk_round4(v);
      *reinterpret_cast<nopk_u32x2*>(&z2[c][row][o]) = r;
      if (z2s && row0 + row < G) {
        *reinterpret_cast<nopk_u32x2*>(
            z2s + ((long long)c * G + row0 + row) * DQ_H + o) = r;
      }
    }
  }
  nopk_barrier();

  // layer 3: D[a][row]
  f32x4 y = {0.f, 0.f, 0.f, 0.f};
  if (l3) {
#pragma unroll
    for (int kc = 0; kc < DQ_H / 32; ++kc) {
      const bf16x8 bf = *reinterpret_cast<const bf16x8*>(
          &z2[c][lane & 15][kc * 32 + (lane >> 4) * 8]);
      y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f3[kc], bf, y, 0, 0, 0);
    }
    if (c && lane < 16) ym[lane] = y[0] + nopk_f32(bias3[0]);
  }
  nopk_barrier();
  if (l3 && !c) {
    const int row = lane & 15;
    if (row0 + row < N) {
      const float m = ym[row];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int a = wq * 16 + (lane >> 4) * 4 + e;
        if (a < A) {
          q[(long long)(row0 + row) * A + a] =
              nopk_round1((y[e] + nopk_f32(bias3[e])) - m);
        }
      }
    }
  }
}

// ---- backward -------------------------------------------------------------

// grid ceil(G / 16). dq [>= G][A] dense, z1s / z2s [2][G][256], w2t
// [2][256][256], w3t [256][32], w3m [256] -> dz1, dz2 [2][G][256], d3m [G]
NOPK_PRE(DRLA_DQ_TAIL_BLOCK) __global__ void drla_dq_tail_bwd(
    const bf16raw* __restrict__ dq, const bf16raw* __restrict__ z1s,
    const bf16raw* __restrict__ z2s, const bf16raw* __restrict__ w2t,
    const bf16raw* __restrict__ w3t, const bf16raw* __restrict__ w3m,
    bf16raw* __restrict__ dz1, bf16raw* __restrict__ dz2,
    bf16raw* __restrict__ d3m, int A, int G) {
  constexpr int D3_LD = DRLA_DQ_MAX_A + 8;
  __shared__ __attribute__((aligned(16))) bf16raw d3[DRLA_DQ_BM][D3_LD];
  __shared__ __attribute__((aligned(16))) bf16raw dzl[2][DRLA_DQ_BM][DQ_ACT_LD];
  __shared__ float d3mf[DRLA_DQ_BM];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int c = wave >> 2;
  const int out0 = (wave & 3) * 64;
  const int row0 = blockIdx.x * DRLA_DQ_BM;
  const int row = lane & 15;  // the row of this lane's accumulators
  const long long grow = (long long)c * G + nopk_min(row0 + row, G - 1);

  // weights and both masks, requested before anything is used
  DqW256 f2;
  bf16x8 f3[4];
  ushort4v w3r[4], mask2[4], mask1[4];
  dq_load_w256(f2, w2t + c * DQ_H * DQ_H, out0, lane);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    f3[ni] = *reinterpret_cast<const bf16x8*>(
        w3t + (out0 + ni * 16 + (lane & 15)) * DRLA_DQ_MAX_A +
        (lane >> 4) * 8);
  }
  dq_load_side(w3r, w3m, out0, lane);
  dq_load_side(mask2, z2s + grow * DQ_H, out0, lane);
  dq_load_side(mask1, z1s + grow * DQ_H, out0, lane);

  // d3v = dQ, zero-padded to 16 x 32
  {
    const int r = tid >> 5, a = tid & 31;
    const bool in = a < A && row0 + r < G;
    const bf16raw v = dq[(long long)nopk_min(row0 + r, G - 1) * A +
                         nopk_min(a, A - 1)];
    d3[r][a] = in ? v : (bf16raw)0;
  }
  nopk_barrier();
  // d3m = -sum_a dQ, f32 in index order, rounded to bf16
  if (tid < DRLA_DQ_BM) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < DRLA_DQ_MAX_A / 8; ++j) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(&d3[tid][8 * j]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += nopk_f32((bf16raw)v[e]);
    }
    const bf16raw m = nopk_round1(-s);
    d3mf[tid] = nopk_f32(m);
    if (row0 + tid < G) d3m[row0 + tid] = m;
  }
  nopk_barrier();

  // dz2 = (d3 . W3) masked by z2 > 0
  {
    f32x4 acc[4];
    if (c == 0) {
      const bf16x8 bf = *reinterpret_cast<const bf16x8*>(
          &d3[row][(lane >> 4) * 8]);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f3[ni], bf, z, 0, 0,
                                                          0);
      }
    } else {
      const float m = d3mf[row];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[ni][e] = m * nopk_f32(w3r[ni][e]);
      }
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int o = out0 + ni * 16 + (lane >> 4) * 4;
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = nopk_pos(mask2[ni][e]) ? acc[ni][e] : 0.f;
      }
      const nopk_u32x2 r = nopk_round4(v);
      *reinterpret_cast<nopk_u32x2*>(&dzl[c][row][o]) = r;
      if (row0 + row < G) {
        *reinterpret_cast<nopk_u32x2*>(dz2 + grow * DQ_H + o) = r;
      }
    }
  }
  nopk_barrier();

  // dz1 = (dz2 . W2) masked by z1 > 0
  {
    f32x4 acc[4];
    dq_mma256(acc, f2, dzl[c], lane);
    if (row0 + row < G) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int o = out0 + ni * 16 + (lane >> 4) * 4;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = nopk_pos(mask1[ni][e]) ? acc[ni][e] : 0.f;
        }
        *reinterpret_cast<nopk_u32x2*>(dz1 + grow * DQ_H + o) = nopk_round4(v);
      }
    }
  }
}

namespace {

// sum over g < G of d[g][dcol] * x[g][col] (d == null: of x[g][col]): f32 in
// row order, eight rows' loads in flight at a time
NOPK_INL float dq_col_sum(const bf16raw* __restrict__ x, int ldx, int col,
                        const bf16raw* __restrict__ d, int ldd, int dcol,
                        int G) {
  float s = 0.f;
  for (int g0 = 0; g0 < G; g0 += 8) {
    float xv[8], dv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int g = nopk_min(g0 + j, G - 1);
      xv[j] = nopk_f32(x[(long long)g * ldx + col]);
      dv[j] = d ? nopk_f32(d[(long long)g * ldd + dcol]) : 1.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s += g0 + j < G ? dv[j] * xv[j] : 0.f;
  }
  return s;
}

}  // namespace

// All twelve parameter gradients of the head, jobs on blockIdx.x:
//   [0, 8 nk)       dW1{v,m} [256][K] = dz1^T . feat, 64 x 64 tiles,
//                   nk = ceil(K / 64)
//   + [0, 32)       dW2{v,m} [256][256] = dz2^T . z1
//   + [0, A + 1)    dW3v row a = sum_g dQ[g][a] z2v[g], then dW3m from d3m
//   + [0, 5)        db1v, db1m, db2v, db2m column sums; db3v and db3m
// The tiled jobs reduce over the G live rows only: both operands are k-rows.
NOPK_PRE(DRLA_DQ_BLOCK) __global__ void drla_dq_wgrad(
    const bf16raw* __restrict__ feat, long long ldf,
    const bf16raw* __restrict__ dz1, const bf16raw* __restrict__ dz2,
    const bf16raw* __restrict__ z1s, const bf16raw* __restrict__ z2s,
    const bf16raw* __restrict__ dq, const bf16raw* __restrict__ d3m,
    DrlaDqGrads out, int K, int A, int G) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * NOPK_SUB];
  const int tid = threadIdx.x;
  const int nk = (K + 63) / 64;
  const long long br = (long long)G * DQ_H;  // one branch of a [2][G][256]
  int job = blockIdx.x;

  if (job < 8 * nk + 32) {  // block-uniform
    const bool first = job < 8 * nk;
    if (!first) job -= 8 * nk;
    const int per = first ? 4 * nk : 16, nx = first ? nk : 4;
    const int c = job / per, by = (job % per) / nx, bx = job % nx;
    const bf16raw* a = (first ? dz1 : dz2) + c * br;
    const bf16raw* b = first ? feat : z1s + c * br;
    const long long ldb = first ? ldf : DQ_H;
    const int ncol = first ? K : DQ_H;
    f32x4 acc[4];
    dq_product<true, true>(acc, lds, DqOperand{a, a, DQ_H, G}, by * 64, DQ_H,
                           DqOperand{b, b, ldb, G}, bx * 64, ncol, 0, G);
    dq_store_tile(acc, first ? out.dw1[c] : out.dw2[c], ncol, by * 64, DQ_H,
                  bx * 64, ncol);
    return;
  }
  job -= 8 * nk + 32;
  if (job <= A) {
    const bool m = job == A;
    const float s = m ? dq_col_sum(z2s + br, DQ_H, tid, d3m, 1, 0, G)
                      : dq_col_sum(z2s, DQ_H, tid, dq, A, job, G);
    (m ? out.dw3[1] : out.dw3[0] + job * DQ_H)[tid] = nopk_round1(s);
    return;
  }
  job -= A + 1;
  if (job < 4) {
    const bf16raw* x = (job < 2 ? dz1 : dz2) + (job & 1) * br;
    (job < 2 ? out.db1 : out.db2)[job & 1][tid] =
        nopk_round1(dq_col_sum(x, DQ_H, tid, nullptr, 0, 0, G));
  } else if (tid < A) {
    out.db3[0][tid] = nopk_round1(dq_col_sum(dq, A, tid, nullptr, 0, 0, G));
  } else if (tid == DRLA_DQ_BLOCK - 1) {
    out.db3[1][0] = nopk_round1(dq_col_sum(d3m, 1, 0, nullptr, 0, 0, G));
  }
}

// grid (ceil(K / 64), ceil(N / 64)). dz1 [2][G][256], w1v / w1m [256][K] ->
// dfeat [N][K] dense: rows < G = dz1v . W1v + dz1m . W1m in one accumulator,
// the rest zeros; a row tile wholly past G computes nothing.
NOPK_PRE(DRLA_DQ_BLOCK) __global__ void drla_dq_l1_dgrad(
    const bf16raw* __restrict__ dz1, const bf16raw* __restrict__ w1v,
    const bf16raw* __restrict__ w1m, bf16raw* __restrict__ dfeat, int N,
    int K, int G) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * NOPK_SUB];
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  f32x4 acc[4];
  dq_product<false, true>(
      acc, lds, DqOperand{dz1, dz1 + (long long)G * DQ_H, DQ_H, DQ_H}, m0, G,
      DqOperand{w1v, w1m, K, DQ_H}, n0, K, 0, m0 < G ? 2 * DQ_H : 0);
  dq_store_tile(acc, dfeat, K, m0, N, n0, K);
}
