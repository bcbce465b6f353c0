// 3x3 / stride 2 / padding 1 max-pool of the IMPALA ResNet torso on gfx950,
// forward and backward: NHWC bf16, C = 16 or 32 channels (template), N, H, W
// at run time, HO = (H - 1)/2 + 1 and WO likewise. Pure data movement: no
// matrix instruction fits a max or a compare-and-add, so the design is about
// touching every global byte once, 16 bytes (8 channels) per lane.
//
// Forward (maxpool3s2_fwd_impl). A block owns `rows` consecutive output rows
// of the flattened [N*HO] row space and stages their 2*rows + 1 input rows in
// LDS once: output row j reads slots 2j, 2j+1, 2j+2 (kh = 0, 1, 2), so the row
// between two output rows is fetched once, not twice. Slot s >= 1 is input row
// 2*ho - 1 + kh of output row (s-1)/2, decoded per row; where the next output
// row starts a new image its kh = 0 row is padding and is never read, so a
// tile may span images. A padding slot is loaded from the clamped row (bytes
// the block fetches anyway) to keep the staging loop free of branches. Then
// one lane per (output pixel, 8 channels) scans kh, kw over LDS with the
// library's rule: a value replaces the running maximum if it is greater or
// NaN, so the first maximum wins a tie, NaN propagates and padding never
// wins. It writes the winning bf16 bits and, if asked, tap = kh*3 + kw as ONE
// byte per element (the library keeps an int64 index).
//
// Backward (maxpool3s2_bwd_impl) is a gather: no atomics, no zero-fill, every
// dx element written once. Input row hi lies in window row ho = hi/2 (as
// kh = 1 for even hi, 2 for odd hi) and, for odd hi, also in ho + 1 (kh = 0)
// when that row exists; columns likewise. So output row ho "owns" input rows
// 2ho and 2ho+1, and a block that owns `pairs` consecutive output rows of
// [N*HO] writes their input rows from pairs + 1 CONSECUTIVE rows of dY and
// tap, which are one contiguous copy into LDS. One lane per (input pixel, 8
// channels), in memory order, reads its <= 2x2 windows from LDS and adds, in
// f32 and in the library's order (ho, then wo), the dY whose tap names this
// pixel; windows that do not exist get the tap 0xFF that no byte equals.
// + addend in f32, one rounding to bf16 (the conv_dgrad convention).
//
// Rows are ints, element offsets 64-bit; the launcher checks both ranges.
//
// Every function of this file is compiled without the packed-f32 VALU ops
// (the compiler pairs the backward's eight sums into them otherwise):
// drla_nopk.h says why, and why every helper here is under NOPK_FN.

#include "drla_kernels.h"
#include "drla_nopk.h"

namespace {

NOPK_INL int pool_max(int a, int b) { return a > b ? a : b; }

// the two bf16 of a 32-bit word as f32 (exact), and back for two f32 that
// hold bf16 values (low = a)
NOPK_INL float pool_lo(unsigned int v) {
  return __builtin_bit_cast(float, v << 16);
}
NOPK_INL float pool_hi(unsigned int v) {
  return __builtin_bit_cast(float, v & 0xFFFF0000u);
}
NOPK_INL unsigned int pool_bits(float a, float b) {
  return (__builtin_bit_cast(unsigned int, a) >> 16) |
         (__builtin_bit_cast(unsigned int, b) & 0xFFFF0000u);
}

// n / d by one multiply-high. m = floor((2^32 - 1) / d) + 1 is 2^32 / d
// rounded up (exact for a power of two); the quotient is exact while
// n * d < 2^32. Here d >= 2 is a row length in 16-byte units (<= 2^11, from
// DRLA_POOL_MAX_ROW_ELEMS) and n an index into one block's tile (< 2^16).
struct PoolDiv { unsigned int d, m; };
NOPK_INL PoolDiv pool_div_by(int d) {
  return {(unsigned int)d, 0xFFFFFFFFu / (unsigned int)d + 1u};
}
NOPK_INL int pool_div(int n, PoolDiv dv) {
  return (int)(((unsigned long long)(unsigned int)n * dv.m) >> 32);
}

// replace the running maximum if v is greater or NaN
NOPK_INL void pool_take(float v, int id, float& m, int& t) {
  if (v > m || v != v) {
    m = v;
    t = id;
  }
}

template <int C>
NOPK_FN __device__ void maxpool3s2_fwd_impl(
    const bf16raw* __restrict__ x, bf16raw* __restrict__ y,
    unsigned char* __restrict__ tap,  // null: not wanted
    int N, int H, int W, int HO, int WO, int rows) {
  constexpr int G = C / 8;  // 16-byte units per pixel
  static_assert(C == 16 || C == 32, "8 channels per lane, 2 or 4 lanes");
  extern __shared__ uint4 pool_lds[];  // [2*rows + 1][W*G]
  __shared__ long long slot_src[2 * DRLA_POOL_MAX_ROWS + 1];
  __shared__ int row_ho[DRLA_POOL_MAX_ROWS];

  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * rows;
  const int nrows = nopk_min(rows, N * HO - r0);
  const int upr = W * G;  // units per input row

  // slot 0: kh = 0 of output row 0; slot s >= 1: kh = 1, 2 of row (s-1)/2
  if (tid <= 2 * nrows) {
    const int j = tid == 0 ? 0 : (tid - 1) >> 1;
    const int r = r0 + j;
    const int n = r / HO;
    const int ho = r - n * HO;
    const int hi =
        nopk_min(pool_max(2 * ho - 1 + (tid - 2 * j), 0), H - 1);
    slot_src[tid] = ((long long)n * H + hi) * upr;
    if (tid & 1) row_ho[j] = ho;
  }
  nopk_barrier();

  const uint4* xu = reinterpret_cast<const uint4*>(x);
  const int staged = (2 * nrows + 1) * upr;
  const PoolDiv by_upr = pool_div_by(upr);
#pragma unroll 4
  for (int u = tid; u < staged; u += DRLA_BLOCK) {
    const int s = pool_div(u, by_upr);
    pool_lds[u] = xu[slot_src[s] + (u - s * upr)];
  }
  nopk_barrier();

  const int opr = WO * G;  // units per output row
  const int nout = nrows * opr;
  const PoolDiv by_opr = pool_div_by(opr);
  for (int o = tid; o < nout; o += DRLA_BLOCK) {
    const int j = pool_div(o, by_opr);
    const int rem = o - j * opr;
    const int wo = rem / G;
    const int g = rem - wo * G;
    const int ho = row_ho[j];

    // the library starts from -inf at the first in-bounds tap
    float m[8];
    int t[8];
    const int tap0 = (ho == 0 ? 3 : 0) + (wo == 0 ? 1 : 0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      m[e] = -INFINITY;
      t[e] = tap0;
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int hi = 2 * ho - 1 + kh;
      if (hi < 0 || hi >= H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int wi = 2 * wo - 1 + kw;
        if (wi < 0 || wi >= W) continue;
        const uint4 v = pool_lds[(2 * j + kh) * upr + wi * G + g];
        const int id = kh * 3 + kw;
        pool_take(pool_lo(v.x), id, m[0], t[0]);
        pool_take(pool_hi(v.x), id, m[1], t[1]);
        pool_take(pool_lo(v.y), id, m[2], t[2]);
        pool_take(pool_hi(v.y), id, m[3], t[3]);
        pool_take(pool_lo(v.z), id, m[4], t[4]);
        pool_take(pool_hi(v.z), id, m[5], t[5]);
        pool_take(pool_lo(v.w), id, m[6], t[6]);
        pool_take(pool_hi(v.w), id, m[7], t[7]);
      }
    }

    // m holds bf16 values: the high halves ARE the winning input bits
    const long long off = (long long)(r0 + j) * opr + rem;
    uint4 out;
    out.x = pool_bits(m[0], m[1]);
    out.y = pool_bits(m[2], m[3]);
    out.z = pool_bits(m[4], m[5]);
    out.w = pool_bits(m[6], m[7]);
    reinterpret_cast<uint4*>(y)[off] = out;
    if (tap) {
      uint2 tp;
      tp.x = t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24);
      tp.y = t[4] | (t[5] << 8) | (t[6] << 16) | (t[7] << 24);
      reinterpret_cast<uint2*>(tap)[off] = tp;
    }
  }
}

// acc[0..7] += the 8 dY of one window whose tap byte equals `expect`
NOPK_INL void pool_add_matching(
    uint4 d, uint2 t, unsigned int expect, float (&acc)[8]) {
  const float v[8] = {pool_lo(d.x), pool_hi(d.x),
                      pool_lo(d.y), pool_hi(d.y),
                      pool_lo(d.z), pool_hi(d.z),
                      pool_lo(d.w), pool_hi(d.w)};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const unsigned int word = e < 4 ? t.x : t.y;
    const unsigned int byte = (word >> (8 * (e & 3))) & 0xFFu;
    acc[e] += byte == expect ? v[e] : 0.0f;
  }
}

template <int C>
NOPK_FN __device__ void maxpool3s2_bwd_impl(
    const bf16raw* __restrict__ dy, const unsigned char* __restrict__ tap,
    const bf16raw* __restrict__ addend,  // null: none
    bf16raw* __restrict__ dx, int N, int H, int W, int HO, int WO,
    int pairs) {
  constexpr int G = C / 8;
  static_assert(C == 16 || C == 32, "8 channels per lane, 2 or 4 lanes");
  constexpr unsigned int NO_WINDOW = 0xFFu;  // taps are 0..8
  extern __shared__ uint4 pool_lds[];  // dY [pairs+1][WO*G], then the taps
  __shared__ long long pair_row[DRLA_POOL_MAX_ROWS];  // n*H + 2*ho
  __shared__ int pair_ho[DRLA_POOL_MAX_ROWS];

  const int tid = threadIdx.x;
  const int total_pairs = N * HO;
  const int p0 = blockIdx.x * pairs;
  const int np = nopk_min(pairs, total_pairs - p0);
  const int nslots = nopk_min(np + 1, total_pairs - p0);
  const int opr = WO * G;  // 16-byte dY units = 8-byte tap units per row
  uint2* tap_lds = reinterpret_cast<uint2*>(pool_lds + (pairs + 1) * opr);

  if (tid < np) {
    const int p = p0 + tid;
    const int n = p / HO;
    const int ho = p - n * HO;
    pair_ho[tid] = ho;
    pair_row[tid] = (long long)n * H + 2 * ho;
  }
  const uint4* dyu = reinterpret_cast<const uint4*>(dy) + (long long)p0 * opr;
  const uint2* tapu = reinterpret_cast<const uint2*>(tap) + (long long)p0 * opr;
  const int staged = nslots * opr;
#pragma unroll 4
  for (int u = tid; u < staged; u += DRLA_BLOCK) {
    pool_lds[u] = dyu[u];
    tap_lds[u] = tapu[u];
  }
  nopk_barrier();

  const int ipr = W * G;  // units per input row
  const int nin = np * 2 * ipr;
  const PoolDiv by_pair = pool_div_by(2 * ipr);
  for (int i = tid; i < nin; i += DRLA_BLOCK) {
    const int j = pool_div(i, by_pair);
    int rem = i - j * 2 * ipr;
    const int hp = rem >= ipr ? 1 : 0;  // 0: row 2*ho, 1: row 2*ho + 1
    rem -= hp * ipr;
    const int ho = pair_ho[j];
    if (2 * ho + hp >= H) continue;  // odd H: the last pair has one row
    const int wi = rem / G;
    const int g = rem - wi * G;
    const int wo = wi >> 1;
    const int wp = wi & 1;

    // window (ho, wo) always holds this pixel, as tap (1+hp, 1+wp); the
    // next window down / right holds it as kh = 0 / kw = 0 for an odd
    // coordinate, if that window exists
    const bool down = hp && ho + 1 < HO;
    const bool right = wp && wo + 1 < WO;
    const unsigned int kh3 = 3 * (1 + hp);
    const unsigned int kw = 1 + wp;
    const int a0 = j * opr + wo * G + g;
    const int a1 = a0 + (right ? G : 0);
    const int b0 = a0 + (down ? opr : 0);
    const int b1 = b0 + (right ? G : 0);

    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    pool_add_matching(pool_lds[a0], tap_lds[a0], kh3 + kw, acc);
    pool_add_matching(pool_lds[a1], tap_lds[a1], right ? kh3 : NO_WINDOW, acc);
    pool_add_matching(pool_lds[b0], tap_lds[b0], down ? kw : NO_WINDOW, acc);
    pool_add_matching(pool_lds[b1], tap_lds[b1],
                      down && right ? 0u : NO_WINDOW, acc);

    const long long off = (pair_row[j] + hp) * ipr + rem;
    if (addend) {
      const uint4 a = reinterpret_cast<const uint4*>(addend)[off];
      acc[0] += pool_lo(a.x); acc[1] += pool_hi(a.x);
      acc[2] += pool_lo(a.y); acc[3] += pool_hi(a.y);
      acc[4] += pool_lo(a.z); acc[5] += pool_hi(a.z);
      acc[6] += pool_lo(a.w); acc[7] += pool_hi(a.w);
    }
    uint4 out;
    out.x = nopk_round2(acc[0], acc[1]);
    out.y = nopk_round2(acc[2], acc[3]);
    out.z = nopk_round2(acc[4], acc[5]);
    out.w = nopk_round2(acc[6], acc[7]);
    reinterpret_cast<uint4*>(dx)[off] = out;
  }
}

}  // namespace

// one kernel per direction and channel count; blockDim.x = DRLA_BLOCK

extern "C" __global__ NOPK_FN void drla_maxpool3s2_fwd_c16(
    const bf16raw* x, bf16raw* y, unsigned char* tap, int N, int H, int W,
    int HO, int WO, int rows) {
  maxpool3s2_fwd_impl<16>(x, y, tap, N, H, W, HO, WO, rows);
}

extern "C" __global__ NOPK_FN void drla_maxpool3s2_fwd_c32(
    const bf16raw* x, bf16raw* y, unsigned char* tap, int N, int H, int W,
    int HO, int WO, int rows) {
  maxpool3s2_fwd_impl<32>(x, y, tap, N, H, W, HO, WO, rows);
}

extern "C" __global__ NOPK_FN void drla_maxpool3s2_bwd_c16(
    const bf16raw* dy, const unsigned char* tap, const bf16raw* addend,
    bf16raw* dx, int N, int H, int W, int HO, int WO, int pairs) {
  maxpool3s2_bwd_impl<16>(dy, tap, addend, dx, N, H, W, HO, WO, pairs);
}

extern "C" __global__ NOPK_FN void drla_maxpool3s2_bwd_c32(
    const bf16raw* dy, const unsigned char* tap, const bf16raw* addend,
    bf16raw* dx, int N, int H, int W, int HO, int WO, int pairs) {
  maxpool3s2_bwd_impl<32>(dy, tap, addend, dx, N, H, W, HO, WO, pairs);
}
