// LDS image maps of the conv wgrad kernels (conv.hip, conv_wgrad_impl).
//
// Both operand tiles of dW^T[k][co] = sum_m A[m][k] * dY[m][co] sit in LDS
// ROW-MAJOR, as they come from memory: 64 m-rows of ROWB bytes (128 B for
// the A tile and the CO=64 dY tile, 64 B for the CO=32 dY tile), written
// with 16-byte stores. ds_read_b64_tr_b16 hands them back column-major as
// 16x16x32 MFMA operands: per 16-lane group it reads a block of 4 rows x 16
// columns, lane 4q+p supplying the address of row q, columns 4p..4p+3, and
// lane i receiving column i with row q in element q.
//
// Bank rule: the transposed read uses 64 banks and conflicts within a
// 32-lane half, whose two groups take rows r..r+3 and r+8..r+11 of the same
// 16 columns (32 B per row) - eight 32-byte pieces that must tile 256 B.
// The 16-byte store uses 32 banks and conflicts within 8 consecutive lanes.
// Padding alone cannot satisfy the read (8 * pitch is always 0 mod 256), so
// the 16-byte chunk index is XORed with row bits:
//   128 B rows: bit0 ^= row bit 0 (separates the two rows one store group
//               spans in the A map), bit1 ^= row bit 1, bit2 ^= row bit 3
//               (row parity picks the 128 B half of the 256 B bank line;
//               bits 1 and 3 spread the four same-parity rows of a half).
//   64 B rows:  bit1 ^= row bit 3 (rows r..r+3 fill the four 64 B
//               quarters; r+8.. lands on the other chunk pair).
// Row bits 2 and 5 stay out of the XOR, so the second half-fragment (+4
// rows) and the second k-step (+32 rows) are constant offsets from one base.
// The static_asserts below emulate the gather and both bank rules for all
// 64 lanes / 256 threads; a wrong map would give wrong operands, no fault.
#pragma once

#define DRLA_WG_ROWS 64  // m-rows per chunk (two 32-row MFMA k-steps)

template <int ROWB>
constexpr int drla_wg_swizzle(int row) {
  static_assert(ROWB == 64 || ROWB == 128, "tile rows are 64 or 128 bytes");
  return ROWB == 128
             ? ((row & 1) | (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2))
             : (((row >> 3) & 1) << 1);
}

// byte offset of 16-byte chunk ch of row `row` (the store address map)
template <int ROWB>
constexpr int drla_wg_chunk_off(int row, int ch) {
  return ROWB * row + 16 * (ch ^ drla_wg_swizzle<ROWB>(row));
}

// byte offset of 16-bit element (row, col)
template <int ROWB>
constexpr int drla_wg_elem_off(int row, int col) {
  return drla_wg_chunk_off<ROWB>(row, col >> 3) + 2 * (col & 7);
}

// transposed-read address of `lane` for 16-column tile `tile`, rows
// 8g..8g+3 of the first k-step (g = lane / 16). The block 4 rows down
// (fragment elements 4..7) is + 4 * ROWB, the second k-step + 32 * ROWB.
template <int ROWB>
constexpr int drla_wg_tr_off(int lane, int tile) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  return drla_wg_chunk_off<ROWB>(8 * g + q, 2 * tile + (p >> 1)) + 8 * (p & 1);
}

// which (row, chunk) thread tid stores in pass j
struct DrlaWgSlot { int row, ch; };
// A tile: 4 threads per row, 16 consecutive k (two chunks) each
constexpr DrlaWgSlot drla_wg_a_slot(int tid, int j) {
  return {tid >> 2, 2 * (tid & 3) + j};
}
// dY tile: one chunk (8 co) per thread and pass; CO/8 threads per row
template <int CO>
constexpr DrlaWgSlot drla_wg_b_slot(int tid, int j) {
  return {tid / (CO / 8) + j * (256 / (CO / 8)), tid % (CO / 8)};
}

// ---- compile-time checks ---------------------------------------------------

// every lane receives, in fragment element e of k-step ks, element
// (m = 32 ks + 8g + e, col = 16 tile + lane % 16): the 16x16x32 operand map
template <int ROWB>
constexpr bool drla_wg_gather_ok() {
  for (int tile = 0; tile < ROWB / 32; ++tile)
    for (int ks = 0; ks < 2; ++ks)
      for (int h = 0; h < 2; ++h)
        for (int lane = 0; lane < 64; ++lane) {
          const int g = lane >> 4, i = lane & 15;
          if (drla_wg_tr_off<ROWB>(lane, tile) % 8) return false;
          for (int q = 0; q < 4; ++q) {
            // row q, columns 4p..4p+3 with p = i / 4 come from lane 4q+p
            const int src = 16 * g + 4 * q + (i >> 2);
            const int got = drla_wg_tr_off<ROWB>(src, tile) +
                            (32 * ks + 4 * h) * ROWB + 2 * (i & 3);
            const int want = drla_wg_elem_off<ROWB>(
                32 * ks + 8 * g + 4 * h + q, 16 * tile + i);
            if (got != want) return false;
          }
        }
  return true;
}

// transposed reads: within a 32-lane half no two lanes on one of 64 banks
template <int ROWB>
constexpr bool drla_wg_reads_conflict_free() {
  for (int tile = 0; tile < ROWB / 32; ++tile)
    for (int step = 0; step < 4; ++step)  // (ks, h)
      for (int half = 0; half < 2; ++half) {
        bool used[64] = {};
        for (int l = 0; l < 32; ++l) {
          const int a = drla_wg_tr_off<ROWB>(32 * half + l, tile) +
                        (32 * (step >> 1) + 4 * (step & 1)) * ROWB;
          for (int d = 0; d < 2; ++d) {
            const int bank = (a / 4 + d) % 64;
            if (used[bank]) return false;
            used[bank] = true;
          }
        }
      }
  return true;
}

// 16-byte stores: within 8 consecutive lanes no two lanes on one of 32
// banks; and the 256 threads' passes fill every chunk exactly once
template <int ROWB, typename SlotFn>
constexpr bool drla_wg_stores_ok(SlotFn slot, int passes) {
  bool filled[DRLA_WG_ROWS * ROWB / 16] = {};
  for (int j = 0; j < passes; ++j)
    for (int grp = 0; grp < 32; ++grp) {
      bool used[32] = {};
      for (int l = 0; l < 8; ++l) {
        const DrlaWgSlot s = slot(8 * grp + l, j);
        if (s.row < 0 || s.row >= DRLA_WG_ROWS || s.ch < 0 ||
            s.ch >= ROWB / 16)
          return false;
        const int a = drla_wg_chunk_off<ROWB>(s.row, s.ch);
        if (a % 16 || a < 0 || a >= DRLA_WG_ROWS * ROWB) return false;
        if (filled[a / 16]) return false;
        filled[a / 16] = true;
        for (int d = 0; d < 4; ++d) {
          const int bank = (a / 4 + d) % 32;
          if (used[bank]) return false;
          used[bank] = true;
        }
      }
    }
  for (int c = 0; c < DRLA_WG_ROWS * ROWB / 16; ++c)
    if (!filled[c]) return false;
  return true;
}

static_assert(drla_wg_gather_ok<128>() && drla_wg_gather_ok<64>(),
              "transposed reads must deliver the 16x16x32 operand map");
static_assert(drla_wg_reads_conflict_free<128>() &&
                  drla_wg_reads_conflict_free<64>(),
              "transposed reads must be bank-conflict-free");
static_assert(drla_wg_stores_ok<128>(drla_wg_a_slot, 2),
              "A tile stores: conflict-free, every chunk once");
static_assert(drla_wg_stores_ok<128>(drla_wg_b_slot<64>, 2),
              "dY tile stores (CO=64): conflict-free, every chunk once");
static_assert(drla_wg_stores_ok<64>(drla_wg_b_slot<32>, 1),
              "dY tile stores (CO=32): conflict-free, every chunk once");
