// The LSTM cell's gate GEMM (K3) and its two backward products, bf16 in and
// out, f32 accumulation in mfma_f32_16x16x32_bf16, one rounding per output.
//
//   drla_gate_gemm_fwd    G[M,N]    = XH[M,K] . W[K,N]
//   drla_gate_gemm_dgrad  dXH[M,K'] = dG[M,N] . W[K',N]^T
//   drla_gate_gemm_wgrad  dW[K,N]   = XH[M,K]^T . dG[M,N]
//
// ONE body (gate_gemm_impl) computes C[Mo][No] = sum_k A(m,k) B(k,n) for all
// three. What differs is how an operand lies in memory, a template flag per
// operand:
//   k-contiguous  memory rows run along k (XH and dG as A, W^T as dgrad's B).
//                 Staged as padded [64][DRLA_GG_BK + 8] sub-tiles and read as
//                 16-byte fragments (the layout of drla_mfma_step_kmajor).
//   k-rows        a memory row is one k (W as the forward's B, XH and dG in
//                 the wgrad). Staged row-major as it comes from memory in the
//                 swizzled 64-row x 128-byte image of conv_wgrad_lds.h and
//                 read back transposed (ds_read_b64_tr_b16); that header
//                 proves the gather and both bank rules at compile time, and
//                 the staging slot here is its drla_wg_b_slot<64>.
// A block of 256 threads owns 64 * MT rows x 64 columns; wave w owns the MT
// 16-row tiles w*MT .. w*MT + MT-1 across all 64 columns. Per 64-k chunk a
// thread moves two 16-byte pieces of every 64 x 64 sub-tile: global loads go
// to registers one chunk ahead, the LDS images are double-buffered, one
// barrier per chunk (the structure of conv_wgrad_impl).
//
// Edges: M is arbitrary, the two other dimensions are multiples of 8, so a
// 16-byte piece is wholly inside or wholly outside. An outside piece is
// loaded from a clamped (valid) address and staged as zeros: no load sits
// behind a branch and EXEC is full around the transposed reads. Stores are
// predicated.
//
// Epilogue: the MFMA takes B's fragment first, so a lane's four accumulators
// are four consecutive columns of one row: one 8-byte bf16 store (16 bytes
// of f32 in a split) per row and column tile.
//
// Forward split-K: grid.z = S splits of the chunk range. For S > 1 a block
// stores its f32 partial tile into ws[z][M][N] and drla_gate_gemm_reduce adds
// the S slices in index order and rounds once: no atomics, the same bits
// every call. Every block of a split stores its whole tile, so the workspace
// needs no zero-fill and carries nothing between calls.
//
// dgrad: columns at or past n_live (grad_cols) are stored as zeros; a column
// tile wholly past it computes nothing.
//
// Packed-f32 VALU ops stay out of this file: every function carries NOPK_FN,
// helpers are drla_nopk.h's (which says why), this file's own or builtins.

#include "drla_kernels.h"
#include "drla_nopk.h"

namespace {

static_assert(DRLA_GG_BK == NOPK_BK && DRLA_GG_BN == 64 && DRLA_GG_BLOCK == 256,
              "the tiles of drla_nopk.h: 64 k x 64 columns, staged by 256 "
              "threads in two passes");

// One operand's block tile: SUBS sub-tiles of 64 rows (k-contiguous) or 64
// columns (k-rows) x 64 k. Thread slot: LDS row srow + 32 j (pass j = 0, 1),
// 16-byte chunk sch: drla_wg_b_slot<64>, whose stores conv_wgrad_lds.h
// proves conflict-free for the k-rows image; in the padded k-contiguous tile
// eight lanes fill 128 contiguous bytes of one row.
template <bool KROWS, int SUBS>
struct GgTile {
  const bf16raw* p;
  long long ld;
  int kmax;               // contraction length of the whole product
  int srow, sch;
  long long off[SUBS][2];  // clamped element offset of the non-k index
  unsigned int live;       // bit 2s + j: that piece's non-k index is inside
  unsigned int klive;      // bit j: the loaded chunk's k is inside
  bf16x8 r[SUBS][2];       // the chunk in flight

  // tile0: first row (k-contiguous) / column (k-rows) of the block's tile;
  // nmax: how many the matrix has
  NOPK_INL void init(const bf16raw* p_, long long ld_, int tile0, int nmax,
                   int kmax_, int tid) {
    p = p_; ld = ld_; kmax = kmax_;
    srow = tid >> 3; sch = tid & 7;
    live = 0;
#pragma unroll
    for (int s = 0; s < SUBS; ++s) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr (KROWS) {
          const int c = tile0 + 64 * s + 8 * sch;
          live |= (unsigned int)(c < nmax) << (2 * s + j);
          off[s][j] = nopk_min(c, nmax - 8);
        } else {
          const int row = tile0 + 64 * s + srow + 32 * j;
          live |= (unsigned int)(row < nmax) << (2 * s + j);
          off[s][j] = (long long)nopk_min(row, nmax - 1) * ld;
        }
      }
    }
  }

  // global -> registers for chunk k0 of a split that ends at k_end
  NOPK_INL void load(int k0, int k_end) {
    klive = 0;
    long long koff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if constexpr (KROWS) {
        const int k = k0 + srow + 32 * j;
        klive |= (unsigned int)(k < k_end) << j;
        koff[j] = (long long)nopk_min(k, kmax - 1) * ld;
      } else {
        const int k = k0 + 8 * sch;
        klive |= (unsigned int)(k < k_end) << j;
        koff[j] = nopk_min(k, kmax - 8);
      }
    }
#pragma unroll
    for (int s = 0; s < SUBS; ++s) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        r[s][j] = *reinterpret_cast<const bf16x8*>(p + off[s][j] + koff[j]);
      }
    }
  }

  // registers -> LDS image; pieces outside the matrix or the split are zeros
  NOPK_INL void store(unsigned char* lds) const {
#pragma unroll
    for (int s = 0; s < SUBS; ++s) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool in = ((live >> (2 * s + j)) & (klive >> j) & 1u) != 0;
        const int o = KROWS ? s * NOPK_KR_SUB + nopk_chunk_off(srow + 32 * j, sch)
                            : s * NOPK_KC_SUB + (srow + 32 * j) * NOPK_PITCH +
                                  16 * sch;
        *reinterpret_cast<bf16x8*>(lds + o) = in ? r[s][j] : nopk_zero8();
      }
    }
  }

  // 16x16x32 operand of 16-wide tile t16, k-step ks: lane l gets element
  // (t16 * 16 + l % 16, 32 ks + 8 (l / 16) + e) in e = 0..7. EXEC is full.
  static NOPK_INL bf16x8 frag(const unsigned char* lds, int t16, int ks,
                            int lane) {
    if constexpr (KROWS) {
      return nopk_frag_kr(lds + (t16 >> 2) * NOPK_KR_SUB, t16 & 3, ks, lane);
    } else {
      return nopk_frag_kc(lds, NOPK_PITCH, t16, ks, lane);
    }
  }
};

// C[Mo][No] = A . B over k in [0, Kc). ws == null: bf16 to c (row stride
// ldc), columns >= n_live as zeros. ws != null: this block's split of k as
// f32 to ws[blockIdx.z][Mo][No].
template <bool A_KROWS, bool B_KROWS, int MT>
NOPK_INL void gate_gemm_impl(const bf16raw* __restrict__ a, long long lda,
                           const bf16raw* __restrict__ b, long long ldb,
                           bf16raw* __restrict__ c, long long ldc,
                           float* __restrict__ ws, int Mo, int No, int Kc,
                           int n_live) {
  constexpr int A_SUB = A_KROWS ? NOPK_KR_SUB : NOPK_KC_SUB;
  constexpr int B_SUB = B_KROWS ? NOPK_KR_SUB : NOPK_KC_SUB;
  constexpr int NFRAG = DRLA_GG_BN / 16;
  __shared__ __attribute__((aligned(16))) unsigned char As[2][MT * A_SUB];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2][B_SUB];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int n0 = blockIdx.x * DRLA_GG_BN;
  const int m0 = blockIdx.y * (64 * MT);

  f32x4 acc[MT][NFRAG];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
#pragma unroll
    for (int ni = 0; ni < NFRAG; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};
  }

  // the split's k range, in whole chunks; an empty one stores zeros
  const int chunks = (Kc + NOPK_BK - 1) / NOPK_BK;
  const int per = (chunks + (int)gridDim.z - 1) / (int)gridDim.z;
  const int k_begin = nopk_min((int)blockIdx.z * per, chunks) * NOPK_BK;
  const int k_end = nopk_min(k_begin + per * NOPK_BK, Kc);
  // block-uniform: a dead column tile computes nothing
  const int nchunks =
      n0 >= n_live ? 0 : (k_end - k_begin + NOPK_BK - 1) / NOPK_BK;

  if (nchunks > 0) {
    GgTile<A_KROWS, MT> ta;
    GgTile<B_KROWS, 1> tb;
    ta.init(a, lda, m0, Mo, Kc, tid);
    tb.init(b, ldb, n0, No, Kc, tid);
    ta.load(k_begin, k_end);
    tb.load(k_begin, k_end);
    ta.store(As[0]);
    tb.store(Bs[0]);
    ta.load(k_begin + NOPK_BK, k_end);
    tb.load(k_begin + NOPK_BK, k_end);
    nopk_barrier();
#pragma unroll 1
    for (int t = 0; t < nchunks; ++t) {
      const int cur = t & 1;
      if (t + 1 < nchunks) {
        ta.store(As[1 - cur]);
        tb.store(Bs[1 - cur]);
        ta.load(k_begin + (t + 2) * NOPK_BK, k_end);
        tb.load(k_begin + (t + 2) * NOPK_BK, k_end);
      }
#pragma unroll
      for (int ks = 0; ks < NOPK_BK / 32; ++ks) {
        bf16x8 bf[NFRAG];
#pragma unroll
        for (int ni = 0; ni < NFRAG; ++ni) {
          bf[ni] = GgTile<B_KROWS, 1>::frag(Bs[cur], ni, ks, lane);
        }
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
          const bf16x8 af =
              GgTile<A_KROWS, MT>::frag(As[cur], wave * MT + mi, ks, lane);
#pragma unroll
          for (int ni = 0; ni < NFRAG; ++ni) {
            // B first: D[n][m], a lane holds n = 4 (l / 16) .. + 3 of m = l % 16
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                bf[ni], af, acc[mi][ni], 0, 0, 0);
          }
        }
      }
      nopk_barrier();
    }
  }

#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    const int m = m0 + (wave * MT + mi) * 16 + (lane & 15);
#pragma unroll
    for (int ni = 0; ni < NFRAG; ++ni) {
      const int n = n0 + ni * 16 + (lane >> 4) * 4;
      if (m < Mo && n < No) {  // No % 8 == 0: four columns in or out together
        if (ws) {
          *reinterpret_cast<f32x4*>(
              ws + ((long long)blockIdx.z * Mo + m) * No + n) = acc[mi][ni];
        } else {
          f32x4 v = acc[mi][ni];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (n + e < n_live) ? v[e] : 0.f;
          *reinterpret_cast<nopk_u32x2*>(c + (long long)m * ldc + n) =
              nopk_round4(v);
        }
      }
    }
  }
}

}  // namespace

// xh [M][K] (row stride ldx), w [K][N] (ldw) -> g [M][N] dense, or ws
NOPK_PRE(DRLA_GG_BLOCK) __global__ void drla_gate_gemm_fwd(const bf16raw* xh, long long ldx,
                             const bf16raw* w, long long ldw, bf16raw* g,
                             float* ws, int M, int K, int N) {
  gate_gemm_impl<false, true, DRLA_GG_FWD_MT>(xh, ldx, w, ldw, g, N, ws, M, N,
                                              K, N);
}

// dg [M][N] (lddg), w [K][N] (ldw) -> dxh [M][K] dense; columns >= grad_cols
// are zeros
NOPK_PRE(DRLA_GG_BLOCK) __global__ void drla_gate_gemm_dgrad(const bf16raw* dg, long long lddg,
                               const bf16raw* w, long long ldw, bf16raw* dxh,
                               int M, int K, int N, int grad_cols) {
  gate_gemm_impl<false, false, DRLA_GG_DGRAD_MT>(dg, lddg, w, ldw, dxh, K,
                                                 nullptr, M, K, N, grad_cols);
}

// xh [M][K] (ldx), dg [M][N] (lddg) -> dw [K][N] dense
NOPK_PRE(DRLA_GG_BLOCK) __global__ void drla_gate_gemm_wgrad(const bf16raw* xh, long long ldx,
                               const bf16raw* dg, long long lddg, bf16raw* dw,
                               int M, int K, int N) {
  gate_gemm_impl<true, true, DRLA_GG_WGRAD_MT>(xh, ldx, dg, lddg, dw, N,
                                               nullptr, K, N, M, N);
}

// g[i] = bf16(ws[0][i] + ws[1][i] + ... + ws[S-1][i]); n4 = M * N / 4
NOPK_PRE(DRLA_GG_BLOCK) __global__ void drla_gate_gemm_reduce(
    const float* __restrict__ ws, bf16raw* __restrict__ g, long long n4,
    int S) {
  nopk_split_reduce<DRLA_GG_BLOCK, false>(ws, nullptr, g, n4, 0, S);
}
