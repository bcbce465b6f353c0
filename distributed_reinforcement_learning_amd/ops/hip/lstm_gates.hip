// K3: fused LSTM-cell elementwise tail, forward + backward.
//
// The cell GEMM ([x,h] @ W) runs on MFMA via hipBLASLt; this kernel fuses the
// remaining 7 elementwise ops (2x sigmoid, 2x tanh, blend, output) into ONE
// HBM pass each way, instead of ~10 eager launches. Gate order [i, g, f, o]
// with TF forget_bias added to f (models/blocks.LSTMCellTF; reference
// impala_actor_critic.py:18-25 uses tf LSTMCell semantics).
//
// Layout: gates [N, 4H] row-major, states [N, H]. One lane per (n, h) cell;
// fully coalesced; stash holds the post-activation gates for backward.
//
// The cell math is written once, in lstm_cell_fwd / lstm_cell_bwd; the per
// step work of the sequence kernels around it (stashes, done mask) once, in
// lstm_seq_step_fwd / lstm_seq_step_bwd. Every kernel below calls these.
// The expressions contract into FMAs at the compiler's choice: keep their
// operand order and where their operands are loaded (KERNELS.md, K3).

#include "drla_kernels.h"

__device__ __forceinline__ float lstm_ld(const float* p) { return *p; }
__device__ __forceinline__ float lstm_ld(const bf16raw* p) {
  return drla_bf16_to_f32(*p);
}
__device__ __forceinline__ void lstm_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void lstm_st(bf16raw* p, float v) {
  *p = drla_f32_to_bf16(v);
}

struct LstmCell { float i_s, g_t, f_s, o_s, c_prev, c_new, h_new; };

// gates[k * H], k = 0..3: the pre-activations in gate order [i, g, f, o]
// -> activated gates, c', h'. Every value is loaded where it is first used:
// with both products of c' open to contraction, the compiler's pick follows
// the order of definitions.
template <typename GT>
__device__ __forceinline__ LstmCell lstm_cell_fwd(
    const GT* gates, int H, float forget_bias, const float* c_prev) {
  LstmCell r;
  r.i_s = drla_sigmoid(lstm_ld(gates));
  r.g_t = tanhf(lstm_ld(gates + H));
  r.f_s = drla_sigmoid(lstm_ld(gates + 2 * H) + forget_bias);
  r.o_s = drla_sigmoid(lstm_ld(gates + 3 * H));
  r.c_prev = *c_prev;
  r.c_new = r.f_s * r.c_prev + r.i_s * r.g_t;
  r.h_new = r.o_s * tanhf(r.c_new);
  return r;
}

struct LstmCellGrad { float di, dg, df, do_, dc_prev; };  // pre-act grads

// tc = tanh(c'), from wherever the caller has c' (the tail kernels read
// new_c, the sequence kernels recompute it from their stash)
__device__ __forceinline__ LstmCellGrad lstm_cell_bwd(
    float i_s, float g_t, float f_s, float o_s, float c_prev, float tc,
    float dh, float dc) {
  const float d_tc = dh * o_s * (1.0f - tc * tc) + dc;
  const float di = d_tc * g_t;
  const float dg = d_tc * i_s;
  const float df = d_tc * c_prev;
  const float do_ = dh * tc;
  LstmCellGrad r;
  r.di = di * i_s * (1.0f - i_s);
  r.dg = dg * (1.0f - g_t * g_t);
  r.df = df * f_s * (1.0f - f_s);
  r.do_ = do_ * o_s * (1.0f - o_s);
  r.dc_prev = d_tc * f_s;
  return r;
}

// GT = float, or bf16raw: the gate GEMM (addmm) emits bf16; reading it
// directly (and emitting bf16 grad_gates) removes the [N,4H] f32 cast
// kernel on each side of the tail (~2 x 4.7 us/step).
template <typename GT>
__device__ __forceinline__ void lstm_tail_fwd_impl(
    const GT* __restrict__ gates, const float* __restrict__ c_prev,
    float* __restrict__ new_h, float* __restrict__ new_c,
    float* __restrict__ stash,  // [N,4H] activated gates (i,g,f,o)
    float forget_bias, long long N, int H,
    float* __restrict__ c_stash,    // [N,H] copy of c_prev (nullable)
    const int* __restrict__ slot, long long c_dist) {  // drla_slot_base
  c_prev = drla_slot_base(c_prev, slot, c_dist);
  long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long total = N * H;
  const long long stride = gridDim.x * (long long)blockDim.x;
  for (; idx < total; idx += stride) {
    const long long n = idx / H;
    const int h = idx - n * H;
    const long long g0 = n * 4LL * H + h;
    const LstmCell r = lstm_cell_fwd(gates + g0, H, forget_bias,
                                     c_prev + idx);
    if (c_stash) c_stash[idx] = r.c_prev;
    new_c[idx] = r.c_new;
    new_h[idx] = r.h_new;
    stash[g0] = r.i_s;
    stash[g0 + H] = r.g_t;
    stash[g0 + 2 * H] = r.f_s;
    stash[g0 + 3 * H] = r.o_s;
  }
}

// grad_c may be null (the cell's new_c is unused downstream — IMPALA's
// batched unroll consumes only new_h — so autograd has no c-grad; the
// null saves a [N,H] zero-fill per step)
template <typename GT>
__device__ __forceinline__ void lstm_tail_bwd_impl(
    const float* __restrict__ grad_h, const float* __restrict__ grad_c,
    const float* __restrict__ stash, const float* __restrict__ c_prev,
    const float* __restrict__ new_c, GT* __restrict__ grad_gates,
    float* __restrict__ grad_c_prev, long long N, int H,
    long long gh_stride) {
  long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long total = N * H;
  const long long stride = gridDim.x * (long long)blockDim.x;
  for (; idx < total; idx += stride) {
    const long long n = idx / H;
    const int h = idx - n * H;
    const long long g0 = n * 4LL * H + h;
    const LstmCellGrad r = lstm_cell_bwd(
        stash[g0], stash[g0 + H], stash[g0 + 2 * H], stash[g0 + 3 * H],
        c_prev[idx], tanhf(new_c[idx]), grad_h[n * gh_stride + h],
        grad_c ? grad_c[idx] : 0.0f);
    grad_c_prev[idx] = r.dc_prev;
    lstm_st(grad_gates + g0, r.di);
    lstm_st(grad_gates + g0 + H, r.dg);
    lstm_st(grad_gates + g0 + 2 * H, r.df);
    lstm_st(grad_gates + g0 + 3 * H, r.do_);
  }
}

extern "C" __global__ void drla_lstm_tail_fwd(
    const float* __restrict__ gates, const float* __restrict__ c_prev,
    float* __restrict__ new_h, float* __restrict__ new_c,
    float* __restrict__ stash, float forget_bias, long long N, int H,
    float* __restrict__ c_stash, const int* __restrict__ slot,
    long long c_dist) {
  lstm_tail_fwd_impl(gates, c_prev, new_h, new_c, stash, forget_bias, N, H,
                     c_stash, slot, c_dist);
}

extern "C" __global__ void drla_lstm_tail_fwd_bf16(
    const bf16raw* __restrict__ gates, const float* __restrict__ c_prev,
    float* __restrict__ new_h, float* __restrict__ new_c,
    float* __restrict__ stash, float forget_bias, long long N, int H,
    float* __restrict__ c_stash, const int* __restrict__ slot,
    long long c_dist) {
  lstm_tail_fwd_impl(gates, c_prev, new_h, new_c, stash, forget_bias, N, H,
                     c_stash, slot, c_dist);
}

extern "C" __global__ void drla_lstm_tail_bwd(
    const float* __restrict__ grad_h, const float* __restrict__ grad_c,
    const float* __restrict__ stash, const float* __restrict__ c_prev,
    const float* __restrict__ new_c, float* __restrict__ grad_gates,
    float* __restrict__ grad_c_prev, long long N, int H,
    long long gh_stride) {
  lstm_tail_bwd_impl(grad_h, grad_c, stash, c_prev, new_c, grad_gates,
                     grad_c_prev, N, H, gh_stride);
}

extern "C" __global__ void drla_lstm_tail_bwd_bf16(
    const float* __restrict__ grad_h, const float* __restrict__ grad_c,
    const float* __restrict__ stash, const float* __restrict__ c_prev,
    const float* __restrict__ new_c, bf16raw* __restrict__ grad_gates,
    float* __restrict__ grad_c_prev, long long N, int H,
    long long gh_stride) {
  lstm_tail_bwd_impl(grad_h, grad_c, stash, c_prev, new_c, grad_gates,
                     grad_c_prev, N, H, gh_stride);
}

// ---------------------------------------------------------------------------
// Sequence kernels: the per-step work of one hidden unit j of batch row
// `row / L`, shared by the narrow and the wide family. gates / dg4 are the
// [4H] LDS gate buffers, hbuf / cbuf / dhc / dcc the [H] LDS carries.
// ---------------------------------------------------------------------------

// STASH (train forward): activated gates [B,L,4H] f32, c_prev [B,L,H] f32
// and h_prev [B,L,H] bf16 (consumed by the dWh GEMM).
template <bool STASH>
__device__ __forceinline__ void lstm_seq_step_fwd(
    const float* gates, float* hbuf, float* cbuf, float* __restrict__ h_out,
    float* __restrict__ acts, float* __restrict__ c_prev_st,
    bf16raw* __restrict__ h_prev_st, float forget_bias, float keep,
    long long row, int j, int H) {
  const long long sb = row * H + j;
  const LstmCell r = lstm_cell_fwd(gates + j, H, forget_bias, cbuf + j);
  if (STASH) {
    const long long ab = row * 4 * H;
    h_prev_st[sb] = drla_f32_to_bf16(hbuf[j]);
    c_prev_st[sb] = r.c_prev;
    acts[ab + j] = r.i_s;
    acts[ab + H + j] = r.g_t;
    acts[ab + 2 * H + j] = r.f_s;
    acts[ab + 3 * H + j] = r.o_s;
  }
  h_out[sb] = r.h_new;
  // done-mask reset applies to the CARRY, not the emitted h
  hbuf[j] = r.h_new * keep;
  cbuf[j] = r.c_new * keep;
}

// Writes the four gate pre-activation grads to dg4 and the c carry to dcc;
// the caller reduces dg4 against Wh into dhc.
__device__ __forceinline__ void lstm_seq_step_bwd(
    const float* __restrict__ dh_out, const float* __restrict__ acts,
    const float* __restrict__ c_prev_st, float* dg4, const float* dhc,
    float* dcc, float keep, long long row, int j, int H) {
  const long long ab = row * 4 * H;
  const long long sb = row * H + j;
  const float i_s = acts[ab + j];
  const float g_t = acts[ab + H + j];
  const float f_s = acts[ab + 2 * H + j];
  const float o_s = acts[ab + 3 * H + j];
  const float cp = c_prev_st[sb];
  const float c_new = f_s * cp + i_s * g_t;
  // carry grads were stored PRE-mask; the forward applied keep_t to
  // this step's outputs before carrying them into t+1
  const float dh_new = dh_out[sb] + dhc[j] * keep;
  const LstmCellGrad r = lstm_cell_bwd(i_s, g_t, f_s, o_s, cp, tanhf(c_new),
                                       dh_new, dcc[j] * keep);
  dg4[j] = r.di;
  dg4[H + j] = r.dg;
  dg4[2 * H + j] = r.df;
  dg4[3 * H + j] = r.do_;
  dcc[j] = r.dc_prev;  // pre-mask carry for t-1
}

// K3 sequence form (SURVEY §5.7a + BASELINE "burn_in hidden-state
// recompute"): the WHOLE LSTM unroll in ONE kernel.
//
// The x-projection (feat @ Wx + b) has no recurrence and runs as one
// batched MFMA GEMM outside; only the tiny h @ Wh chain is sequential.
// One block per batch row: Wh [H][4H] staged in LDS once, then L steps of
// {gates_h = h @ Wh + xgates[t]; cell tail; done-mask reset} with h/c in
// LDS. blockDim = 4H (H=64 -> 256 threads); consecutive lanes read
// consecutive Wh bytes (conflict-free). A hidden size whose Wh is larger
// than LDS (H > 140, up to the 4H <= 1024 block cap) runs the same body
// with Wh read from global memory, where its <= 512 KB stay L2-resident.
// STASH is the forward WITH GRADIENTS of the R2D2 trained window; its
// backward is drla_lstm_seq_train_bwd, and the x-projection GEMM, dWh GEMM
// and bias reduce stay outside (MFMA-shaped, autograd/hipBLASLt).
//
// Replaces the reference's per-timestep replica chain
// (r2d2_lstm.py:67-114): ~5 launches/step -> 1 launch per sequence.

template <bool WH_IN_LDS, bool STASH>
__device__ __forceinline__ void lstm_seq_fwd_impl(
    const bf16raw* __restrict__ xg16,  // [B,L,4H] (nullable)
    const float* __restrict__ xg32,      // [B,L,4H] (nullable)
    const bf16raw* __restrict__ Wh,    // [H][4H] bf16
    const float* __restrict__ h0,        // [B,H]
    const float* __restrict__ c0,        // [B,H]
    const unsigned char* __restrict__ done,  // [B,L]
    float* __restrict__ h_out,           // [B,L,H]
    float* __restrict__ h_fin,           // [B,H]
    float* __restrict__ c_fin,           // [B,H]
    float* __restrict__ acts,            // [B,L,4H]  (STASH only)
    float* __restrict__ c_prev_st,       // [B,L,H]   (STASH only)
    bf16raw* __restrict__ h_prev_st,   // [B,L,H]   (STASH only)
    float forget_bias, int L, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16raw* wh_lds = reinterpret_cast<bf16raw*>(smem);    // [H*4H] or empty
  float* hbuf = reinterpret_cast<float*>(
      wh_lds + (WH_IN_LDS ? drla_lstm_seq_wh_elems(H) : 0));
  float* cbuf = hbuf + H;                                    // [H]

  const int b = blockIdx.x;
  const int j = threadIdx.x;          // gate index in [0, 4H)
  const int G = 4 * H;

  if (WH_IN_LDS) {
    for (int i = j; i < H * G; i += blockDim.x) wh_lds[i] = Wh[i];
  }
  const bf16raw* wh = WH_IN_LDS ? wh_lds : Wh;
  if (j < H) {
    hbuf[j] = h0[(long long)b * H + j];
    cbuf[j] = c0[(long long)b * H + j];
  }
  __syncthreads();

  for (int t = 0; t < L; ++t) {
    const long long row = (long long)b * L + t;
    // gates_h[j] = sum_k h[k] * Wh[k][j]
    float g = 0.0f;
    for (int k = 0; k < H; ++k) {
      g = fmaf(hbuf[k], drla_bf16_to_f32(wh[k * G + j]), g);
    }
    const long long xbase = row * G + j;
    g += xg16 ? drla_bf16_to_f32(xg16[xbase]) : xg32[xbase];
    __shared__ float gates[LSTM_SEQ_MAX_GATES];
    static_assert(sizeof(gates) == LSTM_SEQ_STATIC_LDS_BYTES, "LDS budget");
    gates[j] = g;
    __syncthreads();
    if (j < H) {
      lstm_seq_step_fwd<STASH>(gates, hbuf, cbuf, h_out, acts, c_prev_st,
                               h_prev_st, forget_bias,
                               done[row] ? 0.0f : 1.0f, row, j, H);
    }
    __syncthreads();
  }
  if (j < H) {
    h_fin[(long long)b * H + j] = hbuf[j];
    c_fin[(long long)b * H + j] = cbuf[j];
  }
}

extern "C" __global__ void drla_lstm_seq_fwd(
    const bf16raw* __restrict__ xg16, const float* __restrict__ xg32,
    const bf16raw* __restrict__ Wh, const float* __restrict__ h0,
    const float* __restrict__ c0, const unsigned char* __restrict__ done,
    float* __restrict__ h_out, float* __restrict__ h_fin,
    float* __restrict__ c_fin, float forget_bias, int B, int L, int H) {
  lstm_seq_fwd_impl<true, false>(xg16, xg32, Wh, h0, c0, done, h_out, h_fin,
                                 c_fin, nullptr, nullptr, nullptr,
                                 forget_bias, L, H);
}

extern "C" __global__ void drla_lstm_seq_fwd_gmem(
    const bf16raw* __restrict__ xg16, const float* __restrict__ xg32,
    const bf16raw* __restrict__ Wh, const float* __restrict__ h0,
    const float* __restrict__ c0, const unsigned char* __restrict__ done,
    float* __restrict__ h_out, float* __restrict__ h_fin,
    float* __restrict__ c_fin, float forget_bias, int B, int L, int H) {
  lstm_seq_fwd_impl<false, false>(xg16, xg32, Wh, h0, c0, done, h_out, h_fin,
                                  c_fin, nullptr, nullptr, nullptr,
                                  forget_bias, L, H);
}

extern "C" __global__ void drla_lstm_seq_train_fwd(
    const bf16raw* __restrict__ xg16, const bf16raw* __restrict__ Wh,
    const float* __restrict__ h0, const float* __restrict__ c0,
    const unsigned char* __restrict__ done, float* __restrict__ h_out,
    float* __restrict__ h_fin, float* __restrict__ c_fin,
    float* __restrict__ acts, float* __restrict__ c_prev_st,
    bf16raw* __restrict__ h_prev_st, float forget_bias, int B, int L,
    int H) {
  lstm_seq_fwd_impl<true, true>(xg16, nullptr, Wh, h0, c0, done, h_out,
                                h_fin, c_fin, acts, c_prev_st, h_prev_st,
                                forget_bias, L, H);
}

// One kernel over the whole backward recurrence: thread per gate, Wh in LDS.
extern "C" __global__ void drla_lstm_seq_train_bwd(
    const float* __restrict__ dh_out,    // [B,L,H]
    const float* __restrict__ dh_fin,    // [B,H] or null
    const float* __restrict__ dc_fin,    // [B,H] or null
    const float* __restrict__ acts,      // [B,L,4H]
    const float* __restrict__ c_prev_st, // [B,L,H]
    const bf16raw* __restrict__ Wh,    // [H][4H]
    const unsigned char* __restrict__ done,  // [B,L]
    bf16raw* __restrict__ dxg,         // [B,L,4H] gate-preact grads
    float* __restrict__ dh0, float* __restrict__ dc0,  // [B,H]
    int B, int L, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16raw* wh = reinterpret_cast<bf16raw*>(smem);
  float* dhc = reinterpret_cast<float*>(wh + drla_lstm_seq_wh_elems(H));
  float* dcc = dhc + H;                                   // [H]

  const int b = blockIdx.x;
  const int j = threadIdx.x;
  const int G = 4 * H;

  for (int i = j; i < H * G; i += blockDim.x) wh[i] = Wh[i];
  if (j < H) {
    dhc[j] = dh_fin ? dh_fin[(long long)b * H + j] : 0.0f;
    dcc[j] = dc_fin ? dc_fin[(long long)b * H + j] : 0.0f;
  }
  __syncthreads();

  __shared__ float dg4[LSTM_SEQ_MAX_GATES];
  static_assert(sizeof(dg4) == LSTM_SEQ_STATIC_LDS_BYTES, "LDS budget");
  for (int t = L - 1; t >= 0; --t) {
    const long long row = (long long)b * L + t;
    const float keep = done[row] ? 0.0f : 1.0f;
    if (j < H) {
      lstm_seq_step_bwd(dh_out, acts, c_prev_st, dg4, dhc, dcc, keep, row, j,
                        H);
    }
    __syncthreads();
    dxg[row * G + j] = drla_f32_to_bf16(dg4[j]);
    if (j < H) {
      float s = 0.0f;
      for (int l = 0; l < G; ++l) {
        s = fmaf(dg4[l], drla_bf16_to_f32(wh[j * G + l]), s);
      }
      dhc[j] = s;  // pre-mask carry for t-1 (h0 enters unmasked)
    }
    __syncthreads();
  }
  if (j < H) {
    dh0[(long long)b * H + j] = dhc[j];
    dc0[(long long)b * H + j] = dcc[j];
  }
}

// ---------------------------------------------------------------------------
// Wide family: hidden sizes the kernels above cannot take (train H > 123,
// no-grad H > 256), up to LSTM_SEQ_MAX_HIDDEN. The block size is fixed
// (LSTM_SEQ_WIDE_BLOCK) and every thread strides over the 4H gate columns,
// two adjacent columns at a time: one 32-bit load brings both bf16 weights
// (4H is even and the launcher checks Wh's alignment), which measured 1.82
// -> 1.40 ms per R2D2 step at H = 512 against one column per load. Wh stays
// in global memory and is streamed every step — all B workgroups read the
// same <= 2 MiB, so it is L2 traffic. LDS holds only the gate buffer and the
// two carries (drla_lstm_seq_wide_lds_bytes). Same math as above: per column
// f32 accumulation over k = 0..H-1 in order, x-projection added last, done
// mask on the carry only.
// ---------------------------------------------------------------------------

template <bool STASH>  // parameters as lstm_seq_fwd_impl
__device__ __forceinline__ void lstm_seq_wide_fwd_impl(
    const bf16raw* __restrict__ xg16, const float* __restrict__ xg32,
    const bf16raw* __restrict__ Wh, const float* __restrict__ h0,
    const float* __restrict__ c0, const unsigned char* __restrict__ done,
    float* __restrict__ h_out, float* __restrict__ h_fin,
    float* __restrict__ c_fin, float* __restrict__ acts,
    float* __restrict__ c_prev_st, bf16raw* __restrict__ h_prev_st,
    float forget_bias, int L, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* gates = reinterpret_cast<float*>(smem);  // [4H]
  float* hbuf = gates + 4 * H;                    // [H]
  float* cbuf = hbuf + H;                         // [H]

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int G = 4 * H;

  for (int j = tid; j < H; j += LSTM_SEQ_WIDE_BLOCK) {
    hbuf[j] = h0[(long long)b * H + j];
    cbuf[j] = c0[(long long)b * H + j];
  }
  __syncthreads();

  for (int t = 0; t < L; ++t) {
    const long long row = (long long)b * L + t;
    // gates_h[j] = sum_k h[k] * Wh[k][j] for the column pair (2p, 2p+1);
    // lanes on consecutive pairs
    for (int p = tid; p < 2 * H; p += LSTM_SEQ_WIDE_BLOCK) {
      const unsigned int* w = reinterpret_cast<const unsigned int*>(Wh) + p;
      float ga = 0.0f, gb = 0.0f;
#pragma unroll 8
      for (int k = 0; k < H; ++k) {
        const unsigned int u = w[k * 2 * H];
        const float hk = hbuf[k];
        ga = fmaf(hk, __uint_as_float(u << 16), ga);
        gb = fmaf(hk, __uint_as_float(u & 0xffff0000u), gb);
      }
      const long long xi = row * G + 2 * p;
      gates[2 * p] = ga + (xg16 ? drla_bf16_to_f32(xg16[xi]) : xg32[xi]);
      gates[2 * p + 1] =
          gb + (xg16 ? drla_bf16_to_f32(xg16[xi + 1]) : xg32[xi + 1]);
    }
    __syncthreads();
    const float keep = done[row] ? 0.0f : 1.0f;
    for (int j = tid; j < H; j += LSTM_SEQ_WIDE_BLOCK) {
      lstm_seq_step_fwd<STASH>(gates, hbuf, cbuf, h_out, acts, c_prev_st,
                               h_prev_st, forget_bias, keep, row, j, H);
    }
    __syncthreads();
  }
  for (int j = tid; j < H; j += LSTM_SEQ_WIDE_BLOCK) {
    h_fin[(long long)b * H + j] = hbuf[j];
    c_fin[(long long)b * H + j] = cbuf[j];
  }
}

extern "C" __global__ __launch_bounds__(LSTM_SEQ_WIDE_BLOCK) void
drla_lstm_seq_wide_fwd(
    const bf16raw* __restrict__ xg16, const float* __restrict__ xg32,
    const bf16raw* __restrict__ Wh, const float* __restrict__ h0,
    const float* __restrict__ c0, const unsigned char* __restrict__ done,
    float* __restrict__ h_out, float* __restrict__ h_fin,
    float* __restrict__ c_fin, float forget_bias, int B, int L, int H) {
  lstm_seq_wide_fwd_impl<false>(xg16, xg32, Wh, h0, c0, done, h_out, h_fin,
                                c_fin, nullptr, nullptr, nullptr,
                                forget_bias, L, H);
}

extern "C" __global__ __launch_bounds__(LSTM_SEQ_WIDE_BLOCK) void
drla_lstm_seq_wide_train_fwd(
    const bf16raw* __restrict__ xg16, const bf16raw* __restrict__ Wh,
    const float* __restrict__ h0, const float* __restrict__ c0,
    const unsigned char* __restrict__ done, float* __restrict__ h_out,
    float* __restrict__ h_fin, float* __restrict__ c_fin,
    float* __restrict__ acts, float* __restrict__ c_prev_st,
    bf16raw* __restrict__ h_prev_st, float forget_bias, int B, int L,
    int H) {
  lstm_seq_wide_fwd_impl<true>(xg16, nullptr, Wh, h0, c0, done, h_out,
                               h_fin, c_fin, acts, c_prev_st, h_prev_st,
                               forget_bias, L, H);
}

// Backward of the wide train forward; the contract of
// drla_lstm_seq_train_bwd. dh[j] = sum_l dg4[l] * Wh[j][l] walks ROW j of
// Wh, so a wave owns a row: its lanes stride over l in bf16 pairs
// (consecutive lanes on consecutive addresses), then a shuffle reduction.
extern "C" __global__ __launch_bounds__(LSTM_SEQ_WIDE_BLOCK) void
drla_lstm_seq_wide_train_bwd(
    const float* __restrict__ dh_out, const float* __restrict__ dh_fin,
    const float* __restrict__ dc_fin, const float* __restrict__ acts,
    const float* __restrict__ c_prev_st, const bf16raw* __restrict__ Wh,
    const unsigned char* __restrict__ done, bf16raw* __restrict__ dxg,
    float* __restrict__ dh0, float* __restrict__ dc0, int B, int L, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dg4 = reinterpret_cast<float*>(smem);  // [4H]
  float* dhc = dg4 + 4 * H;                     // [H]
  float* dcc = dhc + H;                         // [H]

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid % DRLA_WAVE;
  const int wave = tid / DRLA_WAVE;
  const int G = 4 * H;

  for (int j = tid; j < H; j += LSTM_SEQ_WIDE_BLOCK) {
    dhc[j] = dh_fin ? dh_fin[(long long)b * H + j] : 0.0f;
    dcc[j] = dc_fin ? dc_fin[(long long)b * H + j] : 0.0f;
  }
  __syncthreads();

  for (int t = L - 1; t >= 0; --t) {
    const long long row = (long long)b * L + t;
    const float keep = done[row] ? 0.0f : 1.0f;
    for (int j = tid; j < H; j += LSTM_SEQ_WIDE_BLOCK) {
      lstm_seq_step_bwd(dh_out, acts, c_prev_st, dg4, dhc, dcc, keep, row, j,
                        H);
    }
    __syncthreads();
    for (int j = tid; j < G; j += LSTM_SEQ_WIDE_BLOCK) {
      dxg[row * G + j] = drla_f32_to_bf16(dg4[j]);
    }
    // j is wave-uniform, so every lane of a wave reaches the shuffles
    for (int j = wave; j < H; j += LSTM_SEQ_WIDE_BLOCK / DRLA_WAVE) {
      const unsigned int* w =
          reinterpret_cast<const unsigned int*>(Wh) + (long long)j * 2 * H;
      float s = 0.0f;
#pragma unroll 4
      for (int q = lane; q < 2 * H; q += DRLA_WAVE) {
        const unsigned int u = w[q];
        s = fmaf(dg4[2 * q], __uint_as_float(u << 16), s);
        s = fmaf(dg4[2 * q + 1], __uint_as_float(u & 0xffff0000u), s);
      }
      for (int off = DRLA_WAVE / 2; off > 0; off >>= 1) {
        s += __shfl_down(s, off, DRLA_WAVE);
      }
      if (lane == 0) dhc[j] = s;  // pre-mask carry for t-1 (h0 unmasked)
    }
    __syncthreads();
  }
  for (int j = tid; j < H; j += LSTM_SEQ_WIDE_BLOCK) {
    dh0[(long long)b * H + j] = dhc[j];
    dc0[(long long)b * H + j] = dcc[j];
  }
}
