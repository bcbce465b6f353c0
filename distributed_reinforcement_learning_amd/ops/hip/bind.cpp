// PyTorch bindings for the drla gfx950 kernels (native HIP — no CUDA
// masquerade: ATen/hip API, hipLaunchKernelGGL on the current HIP stream).
// Compiled by hipcc together with the .hip translation units (see
// ops/build.py); loaded as
// distributed_reinforcement_learning_amd.ops._drla_hip.
// Kernel signatures and every shape constant shared with the kernels come
// from drla_kernels.h / drla_common.h — none is restated here.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <tuple>

#include "drla_kernels.h"

namespace {

hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// ---- argument checks and typed pointers -----------------------------------
void check_gpu_contig(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

template <typename... Ts>
void check_all_gpu_contig(const char* what, const Ts&... ts) {
  (check_gpu_contig(ts, what), ...);
}

// bf16 bits of a tensor that must BE bf16 (data_ptr<float>() checks its
// dtype; a bare reinterpret would not). BF16P / BF16PM name the argument.
bf16raw* bf16_ptr(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  return static_cast<bf16raw*>(t.data_ptr());
}
#define BF16P(t) static_cast<const bf16raw*>(bf16_ptr(t, #t))
#define BF16PM(t) bf16_ptr(t, #t)

// kernels that take bf16 OR float32 have a pointer pair, one of them null
struct DualPtr { bf16raw* bf16; float* f32; };

// The device slot word of double-buffered static inputs (drla_slot_base):
// absent -> null, and the kernel reads its inputs where they are given.
// dist holds one element distance per slotted input of the launcher.
const int* slot_ptr(const c10::optional<torch::Tensor>& slot,
                    const std::vector<int64_t>& dist, size_t n_dist) {
  if (!slot.has_value()) return nullptr;
  TORCH_CHECK(slot->is_cuda() && slot->scalar_type() == torch::kInt &&
                  slot->numel() == 1,
              "slot must be one int32 on the GPU");
  TORCH_CHECK(dist.size() == n_dist, "slot_dist needs ", n_dist, " entries");
  for (auto d : dist) TORCH_CHECK(d >= 0, "negative slot distance");
  return slot->data_ptr<int>();
}
DualPtr dual_ptr(const torch::Tensor& t) {
  if (t.scalar_type() == torch::kBFloat16)
    return {static_cast<bf16raw*>(t.data_ptr()), nullptr};
  return {nullptr, t.data_ptr<float>()};
}

const unsigned char* boolp(const torch::Tensor& t) {
  return reinterpret_cast<const unsigned char*>(t.data_ptr<bool>());
}
// int64 tables: indices (i64p) or raw device addresses (u64p)
long long* i64p(const torch::Tensor& t) {
  return reinterpret_cast<long long*>(t.data_ptr<int64_t>());
}
const unsigned long long* u64p(const torch::Tensor& t) {
  return reinterpret_cast<const unsigned long long*>(t.data_ptr<int64_t>());
}

// ---- frame normalize, V-trace scan ----------------------------------------

torch::Tensor normalize_frames_f32(torch::Tensor frames) {
  check_gpu_contig(frames, "frames");
  TORCH_CHECK(frames.scalar_type() == torch::kUInt8, "frames must be uint8");
  auto out = torch::empty_like(frames, frames.options().dtype(torch::kFloat));
  const long long n = frames.numel();
  const long long n4 = n / 4;
  if (n4 > 0) {
    hipLaunchKernelGGL(drla_u8_normalize_f32, dim3(drla_grid(n4)),
                       dim3(DRLA_BLOCK), 0, cur_stream(),
                       reinterpret_cast<const uchar4*>(frames.data_ptr<uint8_t>()),
                       reinterpret_cast<float4*>(out.data_ptr<float>()), n4);
  }
  if (n % 4) {
    hipLaunchKernelGGL(drla_u8_normalize_f32_tail, dim3(1), dim3(DRLA_BLOCK),
                       0, cur_stream(), frames.data_ptr<uint8_t>(),
                       out.data_ptr<float>(), n4 * 4, n);
  }
  return out;
}

torch::Tensor normalize_frames_bf16(torch::Tensor frames) {
  check_gpu_contig(frames, "frames");
  TORCH_CHECK(frames.scalar_type() == torch::kUInt8, "frames must be uint8");
  auto out = torch::empty_like(frames,
                               frames.options().dtype(torch::kBFloat16));
  const long long n = frames.numel();
  const long long n4 = n / 4;
  if (n4 > 0) {
    hipLaunchKernelGGL(drla_u8_normalize_bf16, dim3(drla_grid(n4)),
                       dim3(DRLA_BLOCK), 0, cur_stream(),
                       reinterpret_cast<const uchar4*>(frames.data_ptr<uint8_t>()),
                       reinterpret_cast<ushort4v*>(out.data_ptr()), n4);
  }
  if (n % 4) {
    hipLaunchKernelGGL(drla_u8_normalize_bf16_tail, dim3(1), dim3(DRLA_BLOCK),
                       0, cur_stream(), frames.data_ptr<uint8_t>(),
                       BF16PM(out), n4 * 4, n);
  }
  return out;
}

torch::Tensor vtrace_scan(torch::Tensor deltas, torch::Tensor discounts,
                          torch::Tensor cs) {
  for (auto* t : {&deltas, &discounts, &cs}) {
    check_gpu_contig(*t, "vtrace input");
    TORCH_CHECK(t->scalar_type() == torch::kFloat, "vtrace wants float32");
  }
  const int B = deltas.size(0);
  const int T = deltas.size(1);
  auto out = torch::empty_like(deltas);
  hipLaunchKernelGGL(drla_vtrace_scan, dim3(drla_grid(B)), dim3(DRLA_BLOCK),
                     0, cur_stream(), deltas.data_ptr<float>(),
                     discounts.data_ptr<float>(), cs.data_ptr<float>(),
                     out.data_ptr<float>(), B, T);
  return out;
}

// ---- conv stack ----------------------------------------------------------
// kernel per layer, indexed like DRLA_CONV_LAYERS; the two u8 layers share
// one signature, the two bf16 layers the other
constexpr auto kConvFwdU8 = std::array{&drla_conv_fwd_l1, &drla_conv_fwd_l1_c1};
constexpr auto kConvFwdBf16 = std::array{&drla_conv_fwd_l2, &drla_conv_fwd_l3};
constexpr auto kConvWgradU8 =
    std::array{&drla_conv_wgrad_l1, &drla_conv_wgrad_l1_c1};
constexpr auto kConvWgradBf16 =
    std::array{&drla_conv_wgrad_l2, &drla_conv_wgrad_l3};
constexpr auto kConvDgrad =
    std::array{&drla_conv_dgrad_l2, &drla_conv_dgrad_l3};

const DrlaConvLayer& conv_layer(int layer) {
  TORCH_CHECK(layer >= 0 && layer < 4, "bad layer");
  return DRLA_CONV_LAYERS[layer];
}
int conv_m_tiles(int rows) { return (rows + DRLA_CONV_BM - 1) / DRLA_CONV_BM; }

torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B) {
  check_gpu_contig(A, "A");
  check_gpu_contig(B, "B");
  auto D = torch::empty({16, 16}, A.options().dtype(torch::kFloat));
  // unchecked on purpose: the probe takes raw 16-bit patterns, and its test
  // passes them as uint16 views
  hipLaunchKernelGGL(drla_mfma_probe, dim3(1), dim3(64), 0, cur_stream(),
                     static_cast<const bf16raw*>(A.data_ptr()),
                     static_cast<const bf16raw*>(B.data_ptr()),
                     D.data_ptr<float>());
  return D;
}

// ---- 3x3 same-padding family (conv3x3.hip), layer ids 4..8 ---------------
// kernels indexed like DRLA_CONV3_LAYERS; the first layer has no dgrad
constexpr auto kConv3Fwd = std::array{
    &drla_c3_fwd_4_16_84, &drla_c3_fwd_16_16_42, &drla_c3_fwd_16_32_42,
    &drla_c3_fwd_32_32_21, &drla_c3_fwd_32_32_11};
constexpr auto kConv3Dgrad = std::array{
    &drla_c3_dgrad_16_16_42, &drla_c3_dgrad_16_32_42,
    &drla_c3_dgrad_32_32_21, &drla_c3_dgrad_32_32_11};
constexpr auto kConv3Wgrad = std::array{
    &drla_c3_wgrad_4_16_84, &drla_c3_wgrad_16_16_42, &drla_c3_wgrad_16_32_42,
    &drla_c3_wgrad_32_32_21, &drla_c3_wgrad_32_32_11};

bool is_conv3(int layer) {
  return layer >= DRLA_CONV3_FIRST &&
         layer < DRLA_CONV3_FIRST + DRLA_CONV3_COUNT;
}
const DrlaConv3Layer& conv3_layer(int layer) {
  TORCH_CHECK(is_conv3(layer), "bad 3x3 layer");
  return DRLA_CONV3_LAYERS[layer - DRLA_CONV3_FIRST];
}
// [batch, hw, hw, c] bf16, dense; the kernels keep row counts in int and
// element offsets in 64 bits, so the row count (plus a tile) must fit an int
void check_conv3_tensor(const torch::Tensor& t, const DrlaConv3Layer& g,
                        int c, const char* name) {
  check_gpu_contig(t, name);
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 4 && t.size(1) == g.hw && t.size(2) == g.hw &&
                  t.size(3) == c,
              name, " must be [N, ", g.hw, ", ", g.hw, ", ", c, "]");
  TORCH_CHECK(t.size(0) >= 1 &&
                  t.size(0) * (int64_t)g.hw * g.hw < (int64_t(1) << 30),
              name, ": batch out of range for the 3x3 conv kernels");
}
const bf16raw* conv3_opt(const c10::optional<torch::Tensor>& t,
                         const torch::Tensor& like, const char* name) {
  if (!t.has_value()) return nullptr;
  check_gpu_contig(*t, name);
  TORCH_CHECK(t->scalar_type() == torch::kBFloat16 &&
                  t->sizes() == like.sizes(),
              name, " must be bf16 and shaped like the output");
  return static_cast<const bf16raw*>(t->data_ptr());
}
// fwd/dgrad grid: one block per 128-row tile up to the cap, then blocks walk
// tiles grid-stride (the weight image is staged once per block)
dim3 conv3_grid(int rows) {
  return dim3(std::min(conv_m_tiles(rows), 4 * DRLA_MAX_BLOCKS));
}

torch::Tensor conv3_fwd(int layer, const torch::Tensor& in,
                        const torch::Tensor& w, const torch::Tensor& bias,
                        bool relu_in,
                        const c10::optional<torch::Tensor>& residual) {
  const auto& g = conv3_layer(layer);
  check_conv3_tensor(in, g, g.ci, "in");
  check_gpu_contig(w, "w");
  check_gpu_contig(bias, "bias");
  TORCH_CHECK(w.numel() == (int64_t)g.co * 9 * g.ci && bias.numel() == g.co,
              "weight/bias do not match the layer");
  const int batch = in.size(0);
  auto out = torch::empty({batch, g.hw, g.hw, g.co}, in.options());
  const bf16raw* resp = conv3_opt(residual, out, "residual");
  hipLaunchKernelGGL(kConv3Fwd[layer - DRLA_CONV3_FIRST],
                     conv3_grid(batch * g.hw * g.hw), dim3(DRLA_CONV_BLOCK),
                     0, cur_stream(), BF16P(in), BF16P(w), BF16P(bias),
                     static_cast<const bf16raw*>(nullptr), resp, BF16PM(out),
                     batch, (int)relu_in);
  return out;
}

torch::Tensor conv3_dgrad(int layer, const torch::Tensor& dy,
                          const torch::Tensor& w,
                          const c10::optional<torch::Tensor>& mask_src,
                          const c10::optional<torch::Tensor>& addend) {
  const auto& g = conv3_layer(layer);
  TORCH_CHECK(layer > DRLA_CONV3_FIRST, "the first 3x3 layer has no dgrad");
  check_conv3_tensor(dy, g, g.co, "dy");
  check_gpu_contig(w, "w");
  TORCH_CHECK(w.numel() == (int64_t)g.co * 9 * g.ci,
              "weight does not match the layer");
  const int batch = dy.size(0);
  auto dx = torch::empty({batch, g.hw, g.hw, g.ci}, dy.options());
  const bf16raw* maskp = conv3_opt(mask_src, dx, "mask_src");
  const bf16raw* addp = conv3_opt(addend, dx, "addend");
  hipLaunchKernelGGL(kConv3Dgrad[layer - DRLA_CONV3_FIRST - 1],
                     conv3_grid(batch * g.hw * g.hw), dim3(DRLA_CONV_BLOCK),
                     0, cur_stream(), BF16P(dy), BF16P(w),
                     static_cast<const bf16raw*>(nullptr), maskp, addp,
                     BF16PM(dx), batch, 0);
  return dx;
}

std::tuple<torch::Tensor, torch::Tensor> conv_fwd(
    int layer, torch::Tensor in, torch::Tensor w, torch::Tensor bias,
    bool stash_input, c10::optional<torch::Tensor> out_slab,
    c10::optional<torch::Tensor> slot, std::vector<int64_t> slot_dist,
    bool relu_in, c10::optional<torch::Tensor> residual) {
  if (is_conv3(layer)) {
    TORCH_CHECK(!stash_input && !out_slab.has_value() && !slot.has_value(),
                "the 3x3 layers take no stash, slab or slot");
    return {conv3_fwd(layer, in, w, bias, relu_in, residual),
            torch::Tensor()};
  }
  TORCH_CHECK(!relu_in && !residual.has_value(),
              "relu_in/residual are 3x3-layer options");
  check_gpu_contig(in, "in");
  TORCH_CHECK(!slot.has_value() || layer < 2,
              "only the u8 input layers take a slot");
  const int* slotp = slot_ptr(slot, slot_dist, 1);
  const long long in_dist = slotp ? slot_dist[0] : 0;
  check_gpu_contig(w, "w");
  check_gpu_contig(bias, "bias");
  const auto& cfg = conv_layer(layer);
  const int batch = in.size(0);
  // out_slab (bf16 layers): a wider row-major [batch, R] bf16 buffer whose
  // leading ho*wo*co columns receive the output; the returned y is that
  // strided view (the gate-GEMM input is assembled in place, no cat)
  torch::Tensor out;
  long long out_n_stride = 0;
  if (out_slab.has_value()) {
    const auto& slab = *out_slab;
    const long long row = (long long)cfg.ho * cfg.wo * cfg.co;
    TORCH_CHECK(layer >= 2, "out_slab is a bf16-layer feature");
    TORCH_CHECK(slab.is_cuda() && slab.dim() == 2 &&
                    slab.scalar_type() == torch::kBFloat16 &&
                    slab.size(0) == batch && slab.size(1) >= row &&
                    slab.stride(1) == 1 && slab.stride(0) >= slab.size(1),
                "out_slab must be a row-major [batch, >= ho*wo*co] bf16 "
                "buffer");
    out_n_stride = slab.stride(0);
    out = slab.as_strided(
        {batch, cfg.ho, cfg.wo, cfg.co},
        {out_n_stride, (long long)cfg.wo * cfg.co, cfg.co, 1});
  } else {
    out = torch::empty({batch, cfg.ho, cfg.wo, cfg.co},
                       in.options().dtype(torch::kBFloat16));
  }
  const dim3 grid(conv_m_tiles(batch * cfg.ho * cfg.wo));
  // stashed-input mode (u8 layers only): the kernel bundles a
  // pass-through copy of the input so the backward never re-reads the
  // (possibly upload-overlapped) source buffer
  torch::Tensor x_stash;
  unsigned char* stashp = nullptr;
  if (stash_input) {
    TORCH_CHECK(layer <= 1, "input stash is a u8-layer feature");
    TORCH_CHECK((in.numel() % 16) == 0, "stash wants 16-divisible bytes");
    x_stash = torch::empty_like(in);
    stashp = x_stash.data_ptr<uint8_t>();
  }
  if (layer <= 1) {
    hipLaunchKernelGGL(kConvFwdU8[layer], grid, dim3(DRLA_CONV_BLOCK), 0,
                       cur_stream(), in.data_ptr<uint8_t>(), BF16P(w),
                       BF16P(bias), BF16PM(out), batch, stashp, slotp,
                       in_dist);
  } else {
    hipLaunchKernelGGL(kConvFwdBf16[layer - 2], grid, dim3(DRLA_CONV_BLOCK),
                       0, cur_stream(), BF16P(in), BF16P(w), BF16P(bias),
                       BF16PM(out), batch, out_n_stride);
  }
  return {out, x_stash};
}

// persistent [DRLA_DBIAS_SLOTS][DRLA_DBIAS_STRIDE] bias-grad partial slots
// shared by relu_mask_bwd (atomic producers, compute stream) and
// wgrad_finalize (sum + re-zero consumer — which may run on the SIDE
// wgrad stream, see ops/conv_op.py),
// so each conv layer owns its own slot set: a later layer's mask must not
// touch slots a pending finalize still reads.
static torch::Tensor& dbias_slot_buf(const torch::Tensor& like,
                                     int64_t slot_id) {
  static torch::Tensor bufs[4];
  TORCH_CHECK(slot_id >= 0 && slot_id < 4, "bad slot id");
  if (!bufs[slot_id].defined()) {
    bufs[slot_id] =
        torch::zeros({DRLA_DBIAS_SLOTS * DRLA_DBIAS_STRIDE},
                     like.options().dtype(torch::kFloat));
  }
  return bufs[slot_id];
}

torch::Tensor relu_mask_bwd(torch::Tensor dy, torch::Tensor y, int64_t CO,
                            int64_t slot_id) {
  TORCH_CHECK(dy.is_cuda() && y.is_cuda(), "dy and y must be on GPU");
  TORCH_CHECK(dy.numel() == y.numel() && dy.size(0) == y.size(0),
              "dy and y must hold the same rows");
  // dy may be an N-strided view (slice of the fused xh grad) and y one too
  // (a conv output living in the xh slab): inner dims contiguous, only
  // stride(0) loose. Returns stride(0) in elements.
  long long row_elems = dy.numel() / std::max<int64_t>(dy.size(0), 1);
  auto n_stride_of = [row_elems](const torch::Tensor& t, const char* name) {
    if (t.is_contiguous()) return row_elems;
    for (int d = 1; d < t.dim(); ++d) {
      TORCH_CHECK(t.stride(d - 1) >= t.stride(d), name, " must be row-major");
    }
    TORCH_CHECK(t.stride(t.dim() - 1) == 1 && t.stride(0) >= row_elems &&
                    row_elems % 8 == 0 && t.stride(0) % 8 == 0 &&
                    t.storage_offset() % 8 == 0,
                name, " view must be inner-contiguous and 16 B aligned");
    for (int d = 1; d + 1 < t.dim(); ++d) {
      TORCH_CHECK(t.stride(d) == t.size(d + 1) * t.stride(d + 1), name,
                  " inner dims must be contiguous");
    }
    return (long long)t.stride(0);
  };
  const long long n_stride = n_stride_of(dy, "dy");
  const long long y_n_stride = n_stride_of(y, "y");
  auto out = torch::empty(dy.sizes(), dy.options());
  auto& slots = dbias_slot_buf(dy, slot_id);
  const long long n = dy.numel();
  TORCH_CHECK(n % 8 == 0, "relu_mask_bwd wants numel % 8 == 0");
  int grid = drla_grid(n / 8);
  if (grid > 640) grid = 640;
  hipLaunchKernelGGL(drla_relu_mask_bwd, dim3(grid), dim3(DRLA_BLOCK),
                     0, cur_stream(), BF16P(dy), BF16P(y), BF16PM(out),
                     slots.data_ptr<float>(), n, (int)CO, n_stride,
                     row_elems, y_n_stride);
  return out;
}

// the wgrad M-split in effect: DRLA_WGRAD_SPLIT (read once, for sweeps) or
// the per-layer default from profiles/wgrad_sweep_r05.md (512 / 64 before
// the row-major staging made a chunk cheaper)
int conv_wgrad_split(int layer) {
  static int split_env = [] {
    const char* e = getenv("DRLA_WGRAD_SPLIT");
    return e ? atoi(e) : 0;
  }();
  if (is_conv3(layer)) {
    // 3x3 family: the fastest of a sweep at the training batch of 640
    // frames (profiles/resnet_conv_r06.md). More blocks hide the per-chunk
    // load latency; each block adds (9 ci + 1) * co atomics, which is what
    // caps the split of the K = 288 layers.
    constexpr int kSplit[DRLA_CONV3_COUNT] = {2048, 1536, 1536, 512, 256};
    return split_env > 0 ? split_env : kSplit[layer - DRLA_CONV3_FIRST];
  }
  conv_layer(layer);
  return split_env > 0 ? split_env : ((layer <= 1) ? 256 : 48);
}

// 3x3 family: one scratch for all five layers. Calls are stream-ordered and
// each finalize leaves it zero, so the next layer finds it zero.
std::tuple<torch::Tensor, torch::Tensor> conv3_wgrad(int layer,
                                                     const torch::Tensor& in,
                                                     const torch::Tensor& dy,
                                                     bool relu_in) {
  const auto& g = conv3_layer(layer);
  check_conv3_tensor(in, g, g.ci, "in");
  check_conv3_tensor(dy, g, g.co, "dy");
  TORCH_CHECK(in.size(0) == dy.size(0), "in and dy differ in batch");
  const int batch = in.size(0);
  const int K = 9 * g.ci;
  static torch::Tensor scratch;
  if (!scratch.defined()) {
    scratch = torch::zeros({DRLA_CONV3_SCRATCH_ELEMS},
                           dy.options().dtype(torch::kFloat));
  }
  TORCH_CHECK((K + 1) * g.co <= DRLA_CONV3_SCRATCH_ELEMS, "scratch too small");
  hipLaunchKernelGGL(kConv3Wgrad[layer - DRLA_CONV3_FIRST],
                     dim3(conv_wgrad_split(layer)), dim3(DRLA_CONV_BLOCK), 0,
                     cur_stream(), BF16P(in), BF16P(dy),
                     scratch.data_ptr<float>(), batch, (int)relu_in);
  auto dw = torch::empty({g.co, K}, dy.options());
  auto dbias = torch::empty({g.co}, dy.options());
  hipLaunchKernelGGL(drla_c3_wgrad_finalize,
                     dim3(drla_grid((long long)(K + 1) * g.co)),
                     dim3(DRLA_BLOCK), 0, cur_stream(),
                     scratch.data_ptr<float>(), BF16PM(dw), BF16PM(dbias), K,
                     g.co);
  return {dw, dbias};
}

std::tuple<torch::Tensor, torch::Tensor> conv_wgrad(int layer,
                                                    torch::Tensor in,
                                                    torch::Tensor dy,
                                                    bool relu_in) {
  if (is_conv3(layer)) return conv3_wgrad(layer, in, dy, relu_in);
  TORCH_CHECK(!relu_in, "relu_in is a 3x3-layer option");
  check_gpu_contig(in, "in");
  check_gpu_contig(dy, "dy");
  const auto& cfg = conv_layer(layer);
  const int batch = in.size(0);
  const int K = cfg.kh * cfg.kw * cfg.ci;
  const int split = conv_wgrad_split(layer);
  // persistent zero-between-calls scratch (finalize re-zeroes on read)
  static torch::Tensor scratch_cache[4];
  if (!scratch_cache[layer].defined()) {
    scratch_cache[layer] =
        torch::zeros({K, cfg.co}, dy.options().dtype(torch::kFloat));
  }
  auto scratch = scratch_cache[layer];
  const dim3 grid((K + DRLA_CONV_WGRAD_BK - 1) / DRLA_CONV_WGRAD_BK, split);
  if (layer <= 1) {
    hipLaunchKernelGGL(kConvWgradU8[layer], grid, dim3(DRLA_CONV_BLOCK), 0,
                       cur_stream(), in.data_ptr<uint8_t>(), BF16P(dy),
                       scratch.data_ptr<float>(), batch);
  } else {
    hipLaunchKernelGGL(kConvWgradBf16[layer - 2], grid,
                       dim3(DRLA_CONV_BLOCK), 0, cur_stream(), BF16P(in),
                       BF16P(dy), scratch.data_ptr<float>(), batch);
  }
  auto dw = torch::empty({cfg.co, K}, dy.options().dtype(torch::kBFloat16));
  auto dbias = torch::empty({cfg.co}, dy.options().dtype(torch::kBFloat16));
  auto& slots = dbias_slot_buf(dy, layer);
  hipLaunchKernelGGL(drla_wgrad_finalize,
                     dim3(drla_grid((long long)K * cfg.co)),
                     dim3(DRLA_BLOCK), 0, cur_stream(),
                     scratch.data_ptr<float>(), BF16PM(dw), K, cfg.co,
                     slots.data_ptr<float>(), BF16PM(dbias));
  return {dw, dbias};
}

torch::Tensor conv_dgrad(int layer, torch::Tensor dy, torch::Tensor w,
                         c10::optional<torch::Tensor> mask_src,
                         c10::optional<torch::Tensor> addend) {
  if (is_conv3(layer)) return conv3_dgrad(layer, dy, w, mask_src, addend);
  TORCH_CHECK(!mask_src.has_value() && !addend.has_value(),
              "mask_src/addend are 3x3-layer options");
  check_gpu_contig(dy, "dy");
  check_gpu_contig(w, "w");
  TORCH_CHECK(layer == 2 || layer == 3, "dgrad only for l2/l3");
  const auto& cfg = conv_layer(layer);
  const int batch = dy.size(0);
  auto dx = torch::empty({batch, cfg.hi, cfg.wi, cfg.ci},
                         dy.options().dtype(torch::kBFloat16));
  // blockIdx.y = the (hi % s, wi % s) class, batch * (hi/s) * (wi/s) rows each
  const int s = cfg.stride;
  hipLaunchKernelGGL(
      kConvDgrad[layer - 2],
      dim3(conv_m_tiles(batch * (cfg.hi / s) * (cfg.wi / s)), s * s),
      dim3(DRLA_CONV_BLOCK), 0, cur_stream(), BF16P(dy), BF16P(w), BF16PM(dx),
      batch);
  return dx;
}

std::tuple<torch::Tensor, torch::Tensor> dqn_loss_fwd(
    torch::Tensor main_q, torch::Tensor next_main, torch::Tensor next_tgt,
    torch::Tensor actions, torch::Tensor rewards, torch::Tensor discounts,
    torch::Tensor weights) {
  check_all_gpu_contig("dqn_loss input", main_q, next_main, next_tgt,
                       actions, rewards, discounts, weights);
  TORCH_CHECK(actions.scalar_type() == torch::kInt, "actions must be i32");
  const int B = main_q.size(0), A = main_q.size(1);
  const DualPtr mq = dual_ptr(main_q);
  auto fopt = rewards.options().dtype(torch::kFloat);
  auto loss = torch::zeros({1}, fopt);
  auto td = torch::empty({B}, fopt);
  hipLaunchKernelGGL(
      drla_dqn_loss_fwd, dim3((B + 255) / 256), dim3(256), 0, cur_stream(),
      mq.bf16, mq.f32, next_main.data_ptr<float>(), next_tgt.data_ptr<float>(),
      actions.data_ptr<int>(), rewards.data_ptr<float>(),
      discounts.data_ptr<float>(), weights.data_ptr<float>(),
      loss.data_ptr<float>(), td.data_ptr<float>(), B, A);
  return {loss, td};
}

torch::Tensor dqn_loss_bwd(torch::Tensor td, torch::Tensor actions,
                           torch::Tensor weights, torch::Tensor gloss,
                           int64_t A, bool want_bf16) {
  check_all_gpu_contig("dqn_loss bwd input", td, actions, weights, gloss);
  const int B = td.numel();
  auto dmq = torch::empty(
      {B, A},
      td.options().dtype(want_bf16 ? torch::kBFloat16 : torch::kFloat));
  const DualPtr out = dual_ptr(dmq);
  hipLaunchKernelGGL(
      drla_dqn_loss_bwd, dim3(((long long)B * A + 255) / 256), dim3(256), 0,
      cur_stream(), td.data_ptr<float>(), actions.data_ptr<int>(),
      weights.data_ptr<float>(), gloss.data_ptr<float>(), out.bf16, out.f32,
      B, (int)A);
  return dmq;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> a2c_loss_fwd(
    torch::Tensor logits, torch::Tensor value, torch::Tensor next_value,
    torch::Tensor actions, torch::Tensor rewards, torch::Tensor done,
    double gamma, int64_t clip_mode, double c_bl, double c_ent) {
  check_all_gpu_contig("a2c loss input", logits, value, next_value, actions,
                       rewards, done);
  TORCH_CHECK(actions.scalar_type() == torch::kInt, "actions must be i32");
  TORCH_CHECK(done.scalar_type() == torch::kBool, "done must be bool");
  const int N = logits.size(0), A = logits.size(1);
  const DualPtr lg = dual_ptr(logits);
  auto fopt = value.options().dtype(torch::kFloat);
  auto losses = torch::zeros({4}, fopt);
  auto p_stash = torch::empty({N, A}, fopt);
  auto adv_st = torch::empty({N}, fopt);
  hipLaunchKernelGGL(
      drla_a2c_loss_fwd, dim3((N + 255) / 256), dim3(256), 0, cur_stream(),
      lg.bf16, lg.f32, value.data_ptr<float>(),
      next_value.data_ptr<float>(), actions.data_ptr<int>(),
      rewards.data_ptr<float>(), boolp(done), static_cast<float>(gamma),
      static_cast<int>(clip_mode),
      static_cast<float>(c_bl), static_cast<float>(c_ent),
      losses.data_ptr<float>(), p_stash.data_ptr<float>(),
      adv_st.data_ptr<float>(), N, A);
  return {losses, p_stash, adv_st};
}

std::tuple<torch::Tensor, torch::Tensor> a2c_loss_bwd(
    torch::Tensor p_stash, torch::Tensor adv_st, torch::Tensor actions,
    torch::Tensor grad3, bool from_total, double c_bl, double c_ent,
    bool want_bf16) {
  check_all_gpu_contig("a2c bwd input", p_stash, adv_st, actions, grad3);
  const int N = p_stash.size(0), A = p_stash.size(1);
  auto dlg = torch::empty(
      {N, A}, p_stash.options().dtype(want_bf16 ? torch::kBFloat16
                                                : torch::kFloat));
  auto dvalue = torch::empty({N}, p_stash.options());
  const DualPtr out = dual_ptr(dlg);
  hipLaunchKernelGGL(
      drla_a2c_loss_bwd, dim3((N + 255) / 256), dim3(256), 0, cur_stream(),
      p_stash.data_ptr<float>(), adv_st.data_ptr<float>(),
      actions.data_ptr<int>(), grad3.data_ptr<float>(),
      from_total ? 1 : 0, static_cast<float>(c_bl),
      static_cast<float>(c_ent), out.bf16, out.f32,
      dvalue.data_ptr<float>(), N, A);
  return {dlg, dvalue};
}

static int next_pow2(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> r2d2_loss_fwd(
    torch::Tensor mq, torch::Tensor tq, torch::Tensor actions,
    torch::Tensor rewards, torch::Tensor done, torch::Tensor weights,
    double gamma, int64_t clip_mode, int64_t n_step, double priority_eta) {
  check_all_gpu_contig("r2d2 loss input", mq, tq, actions, rewards, done,
                       weights);
  TORCH_CHECK(n_step >= 1, "n_step must be >= 1");
  TORCH_CHECK(priority_eta <= 1.0,
              "priority_eta must be <= 1 (negative: |mean td| priority)");
  TORCH_CHECK(actions.scalar_type() == torch::kInt, "actions must be i32");
  TORCH_CHECK(done.scalar_type() == torch::kBool, "done must be bool");
  const int B = mq.size(0), W = mq.size(1), A = mq.size(2);
  TORCH_CHECK(W >= 2 && W <= 1024, "window out of range");
  TORCH_CHECK(tq.scalar_type() == mq.scalar_type(), "mq/tq dtype mismatch");
  const DualPtr m = dual_ptr(mq), t = dual_ptr(tq);
  auto fopt = rewards.options().dtype(torch::kFloat);
  auto loss = torch::zeros({1}, fopt);
  auto td_st = torch::empty({B, W - 1}, fopt);
  auto td_out = torch::empty({B}, fopt);
  const int block = next_pow2(W - 1);
  if (n_step == 1 && priority_eta < 0.0) {
    hipLaunchKernelGGL(
        drla_r2d2_loss_fwd, dim3(B), dim3(block), 0, cur_stream(),
        m.bf16, m.f32, t.bf16, t.f32, actions.data_ptr<int>(),
        rewards.data_ptr<float>(), boolp(done), weights.data_ptr<float>(),
        static_cast<float>(gamma), static_cast<int>(clip_mode),
        loss.data_ptr<float>(), td_st.data_ptr<float>(),
        td_out.data_ptr<float>(), B, W, A);
    return {loss, td_st, td_out};
  }
  // every n >= W-1 truncates at the window end alike
  const int n = static_cast<int>(std::min<int64_t>(n_step, W));
  hipLaunchKernelGGL(
      drla_r2d2_nstep_loss_fwd, dim3(B), dim3(block), 0, cur_stream(),
      m.bf16, m.f32, t.bf16, t.f32, actions.data_ptr<int>(),
      rewards.data_ptr<float>(), boolp(done), weights.data_ptr<float>(),
      static_cast<float>(gamma), static_cast<int>(clip_mode), n,
      static_cast<float>(priority_eta), loss.data_ptr<float>(),
      td_st.data_ptr<float>(), td_out.data_ptr<float>(), B, W, A);
  return {loss, td_st, td_out};
}

torch::Tensor dueling_head_fwd(torch::Tensor h, torch::Tensor Wt,
                               torch::Tensor bt, torch::Tensor Wo,
                               torch::Tensor bo, int64_t burn) {
  check_all_gpu_contig("dueling head input", h, Wt, bt, Wo, bo);
  TORCH_CHECK(h.dim() == 3 && h.scalar_type() == torch::kFloat,
              "h must be [B,L,IN] f32");
  const int B = h.size(0), L = h.size(1), IN = h.size(2);
  const int MID = Wt.size(0), AO = Wo.size(0);
  TORCH_CHECK(Wt.size(1) == IN && Wo.size(1) == MID, "weight shape");
  TORCH_CHECK(IN <= DHEAD_MAX_IN && MID <= DHEAD_MAX_MID &&
                  AO <= DHEAD_MAX_AO && AO >= 2,
              "dueling head dims out of range");
  const int W = L - (int)burn;
  auto q = torch::empty({B, W, AO - 1},
                        h.options().dtype(torch::kBFloat16));
  const size_t lds = drla_dhead_fwd_lds_bytes(IN, MID, AO);
  TORCH_CHECK(lds <= DRLA_LDS_BUDGET,
              "dueling head weights exceed the 160 KB LDS budget");
  const long long npairs = ((long long)B * W + 1) / 2;
  // few blocks, many row-pairs each: every block stages the full weight
  // set in LDS, so the grid must amortize that (~24 KB/block) over rows
  const int gx = (int)std::min<long long>((npairs + 7) / 8, 64);
  hipLaunchKernelGGL(drla_dueling_head_fwd, dim3(gx), dim3(256), lds,
                     cur_stream(), h.data_ptr<float>(), BF16P(Wt),
                     BF16P(bt), BF16P(Wo), BF16P(bo), BF16PM(q), B, L,
                     (int)burn, IN, MID, AO);
  return q;
}

std::tuple<torch::Tensor, torch::Tensor> dhead_train_fwd(
    torch::Tensor h, torch::Tensor Wt, torch::Tensor bt, torch::Tensor Wo,
    torch::Tensor bo) {
  check_all_gpu_contig("dhead fwd input", h, Wt, bt, Wo, bo);
  TORCH_CHECK(h.dim() == 2 && h.scalar_type() == torch::kFloat,
              "h must be [N,IN] f32");
  const int N = h.size(0), IN = h.size(1);
  const int MID = Wt.size(0), AO = Wo.size(0);
  TORCH_CHECK(Wt.size(1) == IN && Wo.size(1) == MID && AO >= 2,
              "dhead weight shape");
  const size_t lds = drla_dhead_fwd_lds_bytes(IN, MID, AO);
  TORCH_CHECK(lds <= DRLA_LDS_BUDGET, "dhead fwd LDS budget");
  auto q = torch::empty({N, AO - 1},
                        h.options().dtype(torch::kBFloat16));
  auto x_st = torch::empty({N, MID},
                           h.options().dtype(torch::kBFloat16));
  const long long npairs = ((long long)N + 1) / 2;
  const int gx = (int)std::min<long long>((npairs + 7) / 8, 64);
  hipLaunchKernelGGL(drla_dhead_train_fwd, dim3(gx), dim3(256), lds,
                     cur_stream(), h.data_ptr<float>(), BF16P(Wt), BF16P(bt),
                     BF16P(Wo), BF16P(bo), BF16PM(q), BF16PM(x_st), N, IN,
                     MID, AO);
  return {q, x_st};
}

std::vector<torch::Tensor> dhead_train_bwd(
    torch::Tensor dq, torch::Tensor x_st, torch::Tensor h,
    torch::Tensor Wt, torch::Tensor Wo) {
  check_all_gpu_contig("dhead bwd input", dq, x_st, h, Wt, Wo);
  const int N = h.size(0), IN = h.size(1);
  const int MID = Wt.size(0), AO = Wo.size(0);
  const size_t lds = (size_t)(MID * IN + AO * MID) * 2 +
                     (size_t)(2 * (MID * IN + AO * MID)
                              + 2 * MID + 2 * AO + MID + IN) * 4;
  TORCH_CHECK(lds <= DRLA_LDS_BUDGET, "dhead bwd LDS budget");
  auto fopt = h.options();
  auto bopt = h.options().dtype(torch::kBFloat16);
  auto dh = torch::empty({N, IN}, fopt);
  const int ws_n = MID * IN + MID + AO * MID + AO;
  auto ws = torch::zeros({ws_n}, fopt);
  const int gx =
      (int)std::min<long long>(((long long)N + 7) / 8, 64);
  hipLaunchKernelGGL(drla_dhead_train_bwd, dim3(gx), dim3(256), lds,
                     cur_stream(), BF16P(dq), BF16P(x_st),
                     h.data_ptr<float>(), BF16P(Wt), BF16P(Wo),
                     dh.data_ptr<float>(), ws.data_ptr<float>(), N, IN,
                     MID, AO);
  auto dWt = torch::empty({MID, IN}, bopt);
  auto dbt = torch::empty({MID}, bopt);
  auto dWo = torch::empty({AO, MID}, bopt);
  auto dbo = torch::empty({AO}, bopt);
  hipLaunchKernelGGL(drla_dhead_train_fin, dim3(drla_grid(ws_n)),
                     dim3(DRLA_BLOCK), 0, cur_stream(),
                     ws.data_ptr<float>(), BF16PM(dWt), BF16PM(dbt),
                     BF16PM(dWo), BF16PM(dbo), IN, MID, AO);
  return {dh, dWt, dbt, dWo, dbo};
}

torch::Tensor r2d2_loss_bwd(torch::Tensor td_st, torch::Tensor actions,
                            torch::Tensor weights, torch::Tensor gloss,
                            int64_t W, int64_t A, bool want_bf16) {
  check_all_gpu_contig("r2d2 bwd input", td_st, actions, weights, gloss);
  const int B = td_st.size(0);
  auto dmq = torch::empty(
      {B, W, A}, td_st.options().dtype(want_bf16 ? torch::kBFloat16
                                                 : torch::kFloat));
  const long long total = (long long)B * W * A;
  const DualPtr out = dual_ptr(dmq);
  hipLaunchKernelGGL(drla_r2d2_loss_bwd, dim3(drla_grid(total)),
                     dim3(DRLA_BLOCK), 0, cur_stream(),
                     td_st.data_ptr<float>(), actions.data_ptr<int>(),
                     weights.data_ptr<float>(), gloss.data_ptr<float>(),
                     out.bf16, out.f32, B, (int)W, (int)A);
  return dmq;
}

void per_update(torch::Tensor tree, torch::Tensor idxs,
                torch::Tensor prios, int64_t cap) {
  check_all_gpu_contig("per tensor", tree, idxs, prios);
  TORCH_CHECK(idxs.scalar_type() == torch::kLong, "idxs must be i64");
  const int n = idxs.numel();
  if (n == 0) return;  // a zero-block grid is an invalid launch
  hipLaunchKernelGGL(drla_per_update, dim3((n + 255) / 256), dim3(256), 0,
                     cur_stream(), tree.data_ptr<float>(), i64p(idxs),
                     prios.data_ptr<float>(), n, cap);
}

void per_rebuild(torch::Tensor tree, int64_t cap) {
  // bottom-up level-by-level recompute of the interior sums from the
  // leaves (drift repair for the float32 atomicAdd delta chains); the
  // level loop lives here so Python pays one call
  check_gpu_contig(tree, "tree");
  // interior nodes are [0, cap-2]; process descending ranges [hi>>1, hi):
  // any i >= hi>>1 has children 2i+1 >= hi, already final from the prior
  // launch — correct for any capacity, ~log2(cap) launches
  long long hi = cap - 1;
  while (hi > 0) {
    const long long lo = hi >> 1;
    const long long count = hi - lo;
    hipLaunchKernelGGL(drla_per_rebuild_level,
                       dim3((count + 255) / 256), dim3(256), 0,
                       cur_stream(), tree.data_ptr<float>(), lo, count);
    hi = lo;
  }
}

void multi_gather(torch::Tensor rows, torch::Tensor srcs,
                  torch::Tensor dsts, torch::Tensor fbytes,
                  int64_t max_chunks) {
  check_all_gpu_contig("multi_gather table", rows, srcs, dsts, fbytes);
  TORCH_CHECK(rows.scalar_type() == torch::kLong, "rows must be i64");
  const int B = rows.numel();
  const int F = srcs.numel();
  if (B == 0 || F == 0) return;  // a zero-block grid is an invalid launch
  const long long total = (long long)B * max_chunks;
  const int gx = (int)std::min<long long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(drla_multi_gather, dim3(gx, F), dim3(256), 0,
                     cur_stream(), i64p(rows), u64p(srcs), u64p(dsts),
                     i64p(fbytes), B);
}

std::tuple<torch::Tensor, torch::Tensor> per_sample(torch::Tensor tree,
                                                    torch::Tensor s,
                                                    torch::Tensor n_entries,
                                                    int64_t cap) {
  check_gpu_contig(tree, "tree");
  check_gpu_contig(s, "s");
  check_gpu_contig(n_entries, "n_entries");
  const int n = s.numel();
  auto idx = torch::empty({n}, s.options().dtype(torch::kLong));
  auto prio = torch::empty({n}, s.options().dtype(torch::kFloat));
  if (n == 0) return {idx, prio};  // a zero-block grid is an invalid launch
  hipLaunchKernelGGL(drla_per_sample, dim3((n + 255) / 256), dim3(256), 0,
                     cur_stream(), tree.data_ptr<float>(),
                     s.data_ptr<float>(), n_entries.data_ptr<float>(),
                     i64p(idx), prio.data_ptr<float>(), n, cap);
  return {idx, prio};
}

torch::Tensor embed_bwd(torch::Tensor indices, torch::Tensor grad_out,
                        int64_t num_rows, bool want_bf16) {
  check_gpu_contig(indices, "indices");
  check_gpu_contig(grad_out, "grad_out");
  TORCH_CHECK(indices.scalar_type() == torch::kLong, "indices must be i64");
  const long long N = grad_out.size(0);
  const int H = grad_out.size(1);
  const DualPtr go = dual_ptr(grad_out);
  torch::Tensor scratch;
  if (want_bf16) {
    // persistent zero-between-calls scratch (the zeroing cast below
    // restores the invariant); f32 callers own the returned tensor, so
    // they keep the per-call allocation
    static torch::Tensor emb_scratch;
    if (!emb_scratch.defined() || emb_scratch.size(0) != num_rows ||
        emb_scratch.size(1) != H) {
      emb_scratch = torch::zeros({num_rows, H},
                                 grad_out.options().dtype(torch::kFloat));
    }
    scratch = emb_scratch;
  } else {
    scratch = torch::zeros({num_rows, H},
                           grad_out.options().dtype(torch::kFloat));
  }
  hipLaunchKernelGGL(
      drla_embed_bwd_scatter, dim3(drla_grid(N * H)), dim3(DRLA_BLOCK), 0,
      cur_stream(), i64p(indices), go.bf16, go.f32,
      scratch.data_ptr<float>(), N, H, (long long)num_rows);
  if (!want_bf16) return scratch;
  auto out = torch::empty({num_rows, H},
                          grad_out.options().dtype(torch::kBFloat16));
  hipLaunchKernelGGL(drla_f32_to_bf16_zero_kernel,
                     dim3(drla_grid(num_rows * H)), dim3(DRLA_BLOCK), 0,
                     cur_stream(), scratch.data_ptr<float>(), BF16PM(out),
                     (long long)(num_rows * H));
  return out;
}

// One launch for the graphed IMPALA step's per-step host write: the learning
// rate and the input set the coming replay reads (runtime/graphed.py).
void set_lr_slot(torch::Tensor lr_buf, torch::Tensor slot_word, double lr,
                 int64_t slot) {
  TORCH_CHECK(lr_buf.is_cuda() && lr_buf.scalar_type() == torch::kFloat &&
                  lr_buf.numel() == 1, "lr_buf must be one f32 on the GPU");
  TORCH_CHECK(slot_word.is_cuda() && slot_word.scalar_type() == torch::kInt &&
                  slot_word.numel() == 1 && (slot == 0 || slot == 1),
              "slot_word must be one int32 on the GPU, slot 0 or 1");
  hipLaunchKernelGGL(drla_set_lr_slot, dim3(1), dim3(64), 0, cur_stream(),
                     lr_buf.data_ptr<float>(), slot_word.data_ptr<int>(),
                     static_cast<float>(lr), (int)slot);
}

std::vector<torch::Tensor> vtrace_loss_fwd(
    torch::Tensor logits, torch::Tensor value, torch::Tensor mu,
    torch::Tensor actions, torch::Tensor rewards, torch::Tensor done,
    double gamma, int64_t clip_mode, double c_bl, double c_ent,
    bool nofill, bool stash_actions, c10::optional<torch::Tensor> slot,
    std::vector<int64_t> slot_dist) {
  // slot_dist: mu, actions, rewards, done
  const int* slotp = slot_ptr(slot, slot_dist, 4);
  const std::vector<int64_t> sd =
      slotp ? slot_dist : std::vector<int64_t>{0, 0, 0, 0};
  check_all_gpu_contig("vtrace_loss input", logits, value, mu, actions,
                       rewards, done);
  TORCH_CHECK(actions.scalar_type() == torch::kInt, "actions must be int32");
  TORCH_CHECK(done.scalar_type() == torch::kBool, "done must be bool");
  const int B = logits.size(0), T = logits.size(1), A = logits.size(2);
  TORCH_CHECK(A <= VT_MAX_A, "num_action cap is ", VT_MAX_A);
  TORCH_CHECK(T <= VT_MAX_T, "trajectory cap is ", VT_MAX_T);
  const DualPtr lg = dual_ptr(logits);
  auto fopt = value.options().dtype(torch::kFloat);
  auto p_stash = torch::empty({B, T, A}, fopt);
  auto vs_stash = torch::empty({B, T - 2}, fopt);
  auto adv_stash = torch::empty({B, T - 2}, fopt);
  // nofill: per-block partials + a ticket counter in persistent buffers
  // (zeroed once here; the kernel's last block restores the counter), so
  // losses needs no zero-fill launch. Default: blocks atomicAdd into a
  // zeroed losses.
  torch::Tensor losses, act_stash;
  float* partials_ptr = nullptr;
  unsigned int* counter_ptr = nullptr;
  if (nofill) {
    static torch::Tensor partials, counter;
    // a captured graph keeps the addresses it was captured with, so a
    // replaced pair is retired, never freed (64 KB covers B <= 4096)
    static std::vector<torch::Tensor> retired;
    if (!partials.defined() || partials.size(0) < B ||
        partials.device() != value.device()) {
      if (partials.defined()) {
        retired.push_back(partials);
        retired.push_back(counter);
      }
      partials = torch::zeros({std::max<int64_t>(B, 4096), 4}, fopt);
      counter = torch::zeros({1}, fopt.dtype(torch::kInt));
    }
    partials_ptr = partials.data_ptr<float>();
    counter_ptr = reinterpret_cast<unsigned int*>(counter.data_ptr<int>());
    losses = torch::empty({4}, fopt);
  } else {
    losses = torch::zeros({4}, fopt);
  }
  int* act_stash_ptr = nullptr;
  if (stash_actions) {
    act_stash = torch::empty_like(actions);
    act_stash_ptr = act_stash.data_ptr<int>();
  }
  hipLaunchKernelGGL(
      drla_vtrace_loss_fwd, dim3(B), dim3(256), 0, cur_stream(),
      lg.bf16, lg.f32, value.data_ptr<float>(), mu.data_ptr<float>(),
      actions.data_ptr<int>(), rewards.data_ptr<float>(), boolp(done),
      static_cast<float>(gamma), (int)clip_mode, static_cast<float>(c_bl),
      static_cast<float>(c_ent), p_stash.data_ptr<float>(),
      vs_stash.data_ptr<float>(), adv_stash.data_ptr<float>(),
      losses.data_ptr<float>(), B, T, A, partials_ptr, counter_ptr,
      act_stash_ptr, slotp, (long long)sd[0], (long long)sd[1],
      (long long)sd[2], (long long)sd[3]);
  if (stash_actions) return {losses, p_stash, vs_stash, adv_stash, act_stash};
  return {losses, p_stash, vs_stash, adv_stash};
}

std::tuple<torch::Tensor, torch::Tensor> vtrace_loss_bwd(
    torch::Tensor p_stash, torch::Tensor vs_stash, torch::Tensor adv_stash,
    torch::Tensor value, torch::Tensor actions, torch::Tensor grad3,
    bool from_total, double c_bl, double c_ent, bool want_bf16) {
  check_all_gpu_contig("vtrace_loss bwd input", p_stash, vs_stash,
                       adv_stash, value, actions, grad3);
  const int B = p_stash.size(0), T = p_stash.size(1), A = p_stash.size(2);
  auto dlogits = torch::empty(
      {B, T, A},
      value.options().dtype(want_bf16 ? torch::kBFloat16 : torch::kFloat));
  auto dvalue = torch::empty({B, T}, value.options().dtype(torch::kFloat));
  const DualPtr out = dual_ptr(dlogits);
  hipLaunchKernelGGL(
      drla_vtrace_loss_bwd, dim3(drla_grid((long long)B * T)), dim3(256), 0,
      cur_stream(), p_stash.data_ptr<float>(), vs_stash.data_ptr<float>(),
      adv_stash.data_ptr<float>(), value.data_ptr<float>(),
      actions.data_ptr<int>(), grad3.data_ptr<float>(),
      from_total ? 1 : 0, static_cast<float>(c_bl),
      static_cast<float>(c_ent), out.bf16, out.f32, dvalue.data_ptr<float>(),
      B, T, A);
  return {dlogits, dvalue};
}

// stash_c: also returns a copy of c_prev made in-kernel (4th element) for a
// backward that must not re-read the caller's c_prev buffer
std::vector<torch::Tensor> lstm_tail_fwd(
    torch::Tensor gates, torch::Tensor c_prev, double forget_bias,
    bool stash_c, c10::optional<torch::Tensor> slot,
    std::vector<int64_t> slot_dist) {
  const int* slotp = slot_ptr(slot, slot_dist, 1);
  const long long c_dist = slotp ? slot_dist[0] : 0;
  check_gpu_contig(gates, "gates");
  check_gpu_contig(c_prev, "c_prev");
  const bool bf16 = gates.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || gates.scalar_type() == torch::kFloat,
              "gates must be bf16 or float32");
  TORCH_CHECK(c_prev.scalar_type() == torch::kFloat, "c_prev must be float32");
  const long long N = gates.size(0);
  const int H4 = gates.size(1);
  TORCH_CHECK(H4 % 4 == 0, "gates dim1 must be 4*H");
  const int H = H4 / 4;
  TORCH_CHECK(c_prev.size(1) == H, "c_prev width mismatch");
  auto new_h = torch::empty_like(c_prev);
  auto new_c = torch::empty_like(c_prev);
  auto stash = torch::empty({N, (long long)H4},
                            c_prev.options().dtype(torch::kFloat));
  torch::Tensor c_stash;
  float* c_stash_ptr = nullptr;
  if (stash_c) {
    c_stash = torch::empty_like(c_prev);
    c_stash_ptr = c_stash.data_ptr<float>();
  }
  if (bf16) {
    hipLaunchKernelGGL(drla_lstm_tail_fwd_bf16, dim3(drla_grid(N * H)),
                       dim3(DRLA_BLOCK), 0, cur_stream(), BF16P(gates),
                       c_prev.data_ptr<float>(), new_h.data_ptr<float>(),
                       new_c.data_ptr<float>(), stash.data_ptr<float>(),
                       static_cast<float>(forget_bias), N, H, c_stash_ptr,
                       slotp, c_dist);
  } else {
    hipLaunchKernelGGL(drla_lstm_tail_fwd, dim3(drla_grid(N * H)),
                       dim3(DRLA_BLOCK), 0, cur_stream(),
                       gates.data_ptr<float>(), c_prev.data_ptr<float>(),
                       new_h.data_ptr<float>(), new_c.data_ptr<float>(),
                       stash.data_ptr<float>(),
                       static_cast<float>(forget_bias), N, H, c_stash_ptr,
                       slotp, c_dist);
  }
  if (stash_c) return {new_h, new_c, stash, c_stash};
  return {new_h, new_c, stash};
}

std::tuple<torch::Tensor, torch::Tensor> lstm_tail_bwd(
    torch::Tensor grad_h, c10::optional<torch::Tensor> grad_c_opt,
    torch::Tensor stash, torch::Tensor c_prev, torch::Tensor new_c,
    bool bf16_gates) {
  check_all_gpu_contig("lstm bwd input", stash, c_prev, new_c);
  // grad_c is null when new_c is unused downstream (saves the zero-fill)
  const float* grad_c_ptr = nullptr;
  if (grad_c_opt.has_value()) {
    check_gpu_contig(*grad_c_opt, "grad_c");
    grad_c_ptr = grad_c_opt->data_ptr<float>();
  }
  // grad_h may be an N-strided [N,H] view (slice of the xh gradient)
  TORCH_CHECK(grad_h.is_cuda() && grad_h.dim() == 2 &&
              grad_h.stride(1) == 1, "grad_h must be row-contiguous");
  const long long gh_stride = grad_h.stride(0);
  const long long N = stash.size(0);
  const int H = stash.size(1) / 4;
  auto grad_c_prev = torch::empty_like(c_prev);
  if (bf16_gates) {
    auto grad_gates = torch::empty(
        {N, (long long)stash.size(1)},
        stash.options().dtype(torch::kBFloat16));
    hipLaunchKernelGGL(drla_lstm_tail_bwd_bf16, dim3(drla_grid(N * H)),
                       dim3(DRLA_BLOCK), 0, cur_stream(),
                       grad_h.data_ptr<float>(), grad_c_ptr,
                       stash.data_ptr<float>(), c_prev.data_ptr<float>(),
                       new_c.data_ptr<float>(), BF16PM(grad_gates),
                       grad_c_prev.data_ptr<float>(), N, H, gh_stride);
    return {grad_gates, grad_c_prev};
  }
  auto grad_gates = torch::empty_like(stash);
  hipLaunchKernelGGL(drla_lstm_tail_bwd, dim3(drla_grid(N * H)),
                     dim3(DRLA_BLOCK), 0, cur_stream(),
                     grad_h.data_ptr<float>(), grad_c_ptr,
                     stash.data_ptr<float>(), c_prev.data_ptr<float>(),
                     new_c.data_ptr<float>(), grad_gates.data_ptr<float>(),
                     grad_c_prev.data_ptr<float>(), N, H, gh_stride);
  return {grad_gates, grad_c_prev};
}

// ---- fused MLP heads, action-embedding MLP ---------------------------------
int mh_row_tiles(int N) { return (N + MH_BM - 1) / MH_BM; }

std::vector<torch::Tensor> mlp_heads_fwd(
    torch::Tensor h, std::vector<torch::Tensor> weights,
    std::vector<torch::Tensor> biases, int64_t A, bool want_bwd_bufs) {
  // want_bwd_bufs: the kernel also zeroes the backward's f32 workspace and
  // writes the packed W^T (the mlp_heads_pack_wt layout); both are appended
  // to the result, and the backward then needs neither a fill nor a pack
  // launch (mlp_heads_bwd's ws argument)
  check_gpu_contig(h, "h");
  TORCH_CHECK(weights.size() == 6 && biases.size() == 6);
  for (auto& t : weights) check_gpu_contig(t, "W");
  for (auto& t : biases) check_gpu_contig(t, "b");
  const int N = h.size(0);
  TORCH_CHECK(h.size(1) == MH_HID && A <= MH_MAX_A);
  auto bopt = h.options().dtype(torch::kBFloat16);
  auto logits = torch::empty({N, A}, bopt);
  auto value = torch::empty({N}, h.options().dtype(torch::kFloat));
  auto stash = torch::empty({N, 5 * 256}, bopt);
  torch::Tensor ws, wt;
  float* ws_ptr = nullptr;
  bf16raw* wt_ptr = nullptr;
  if (want_bwd_bufs) {
    ws = torch::empty({(long long)N * 256 + 4 * 256 + A + 1},
                      h.options().dtype(torch::kFloat));
    wt = torch::empty({4 * 65536 + 256 * 32 + 256}, bopt);
    ws_ptr = ws.data_ptr<float>();
    wt_ptr = BF16PM(wt);
  }
  hipLaunchKernelGGL(
      drla_mlp_heads_fwd, dim3(mh_row_tiles(N), 2), dim3(256), 0,
      cur_stream(), h.data_ptr<float>(),
      BF16P(weights[0]), BF16P(biases[0]), BF16P(weights[1]),
      BF16P(biases[1]), BF16P(weights[2]), BF16P(biases[2]),
      BF16P(weights[3]), BF16P(biases[3]), BF16P(weights[4]),
      BF16P(biases[4]), BF16P(weights[5]), BF16P(biases[5]),
      BF16PM(logits), value.data_ptr<float>(), BF16PM(stash), N, (int)A,
      wt_ptr, ws_ptr);
  if (want_bwd_bufs) return {logits, value, stash, ws, wt};
  return {logits, value, stash};
}

// ws_opt: the workspace a want_bwd_bufs forward already zeroed (one use per
// forward: the kernel accumulates into it); absent -> zero-filled here
std::vector<torch::Tensor> mlp_heads_bwd(
    torch::Tensor dlogits, torch::Tensor dvalue, torch::Tensor stash,
    std::vector<torch::Tensor> weights, int64_t A,
    c10::optional<torch::Tensor> ws_opt) {
  check_gpu_contig(dlogits, "dlogits");
  check_gpu_contig(dvalue, "dvalue");
  check_gpu_contig(stash, "stash");
  TORCH_CHECK(weights.size() == 6);
  const int N = dvalue.numel();
  auto bopt = dlogits.options().dtype(torch::kBFloat16);
  auto fopt = dvalue.options().dtype(torch::kFloat);
  auto dz1p = torch::empty({N, 256}, bopt);
  auto dz2p = torch::empty({N, 256}, bopt);
  auto dz1v = torch::empty({N, 256}, bopt);
  auto dz2v = torch::empty({N, 256}, bopt);
  // dh + all six bias grads live in ONE zeroed workspace (atomics targets;
  // one fill kernel instead of seven)
  const long long ws_n = (long long)N * 256 + 4 * 256 + A + 1;
  torch::Tensor ws;
  if (ws_opt.has_value()) {
    ws = *ws_opt;
    check_gpu_contig(ws, "ws");
    TORCH_CHECK(ws.scalar_type() == torch::kFloat && ws.numel() == ws_n,
                "ws must be f32 [N*256 + 4*256 + A + 1]");
  } else {
    ws = torch::zeros({ws_n}, fopt);
  }
  long long off = 0;
  auto dh = ws.narrow(0, off, (long long)N * 256).view({N, 256});
  off += (long long)N * 256;
  auto db1p = ws.narrow(0, off, 256); off += 256;
  auto db2p = ws.narrow(0, off, 256); off += 256;
  auto db3p = ws.narrow(0, off, A); off += A;
  auto db1v = ws.narrow(0, off, 256); off += 256;
  auto db2v = ws.narrow(0, off, 256); off += 256;
  auto db3v = ws.narrow(0, off, 1);
  hipLaunchKernelGGL(
      drla_mlp_heads_bwd, dim3(mh_row_tiles(N), 2), dim3(256), 0,
      cur_stream(), BF16P(dlogits), dvalue.data_ptr<float>(), BF16P(stash),
      BF16P(weights[0]), BF16P(weights[1]), BF16P(weights[2]),
      BF16P(weights[3]), BF16P(weights[4]), BF16P(weights[5]), BF16PM(dz1p),
      BF16PM(dz2p), BF16PM(dz1v), BF16PM(dz2v), dh.data_ptr<float>(),
      db1p.data_ptr<float>(), db2p.data_ptr<float>(),
      db3p.data_ptr<float>(), db1v.data_ptr<float>(),
      db2v.data_ptr<float>(), db3v.data_ptr<float>(), N, (int)A);
  // ws comes back too so the wrapper can cast the contiguous bias-grad
  // tail (db1p..db3v) to bf16 in ONE kernel instead of six
  return {dz1p, dz2p, dz1v, dz2v, dh,   db1p, db2p, db3p, db1v, db2v,
          db3v, ws};
}

// Returns {out, a1}, then the in-kernel copy of the clamped indices when
// stash_idx, then W2^T ([256,256], for embed_mlp_bwd's w2t argument) when
// want_w2t.
std::vector<torch::Tensor> embed_mlp_fwd(
    torch::Tensor pa, torch::Tensor table, torch::Tensor b1,
    torch::Tensor w2, torch::Tensor b2, bool stash_idx, bool want_w2t,
    c10::optional<torch::Tensor> xh_slab, int64_t emb_col,
    c10::optional<torch::Tensor> h_opt, c10::optional<torch::Tensor> slot,
    std::vector<int64_t> slot_dist) {
  // slot_dist: pa, h (0 for an input that is not double-buffered)
  const int* slotp = slot_ptr(slot, slot_dist, 2);
  const long long pa_dist = slotp ? slot_dist[0] : 0;
  const long long h_dist = slotp ? slot_dist[1] : 0;
  check_all_gpu_contig("embed fwd input", pa, table, b1, w2, b2);
  TORCH_CHECK(pa.scalar_type() == torch::kLong, "pa must be int64");
  const int N = pa.numel();
  auto bopt = table.options();
  // xh_slab: the gate-GEMM input [N, emb_col + 256 + H + 8] bf16, assembled
  // in place — out becomes the slab's columns [emb_col, emb_col + 256) and
  // the kernel also writes bf16(h) and the (1, 0 x 7) pad after them
  torch::Tensor out;
  long long slab_stride = 0;
  const float* h_ptr = nullptr;
  int H = 0;
  if (xh_slab.has_value()) {
    const auto& slab = *xh_slab;
    TORCH_CHECK(h_opt.has_value(), "xh_slab needs h");
    const auto& h = *h_opt;
    check_gpu_contig(h, "h");
    check_gpu_contig(slab, "xh_slab");
    TORCH_CHECK(h.scalar_type() == torch::kFloat && h.dim() == 2 &&
                    h.size(0) == N && h.size(1) % 8 == 0,
                "h must be f32 [N, H], H % 8 == 0");
    H = h.size(1);
    TORCH_CHECK(slab.dim() == 2 && slab.scalar_type() == torch::kBFloat16 &&
                    slab.size(0) == N && emb_col >= 0 && emb_col % 8 == 0 &&
                    slab.size(1) == emb_col + 256 + H + 8 &&
                    slab.storage_offset() % 8 == 0,
                "xh_slab must be bf16 [N, emb_col + 256 + H + 8]");
    slab_stride = slab.stride(0);
    h_ptr = h.data_ptr<float>();
    out = slab.narrow(1, emb_col, 256);
  } else {
    out = torch::empty({N, 256}, bopt);
  }
  auto a1 = torch::empty({N, 256}, bopt);
  std::vector<torch::Tensor> res = {out, a1};
  long long* idx_ptr = nullptr;
  bf16raw* w2t_ptr = nullptr;
  if (stash_idx) {
    res.push_back(torch::empty({N}, pa.options()));
    idx_ptr = reinterpret_cast<long long*>(res.back().data_ptr<int64_t>());
  }
  if (want_w2t) {
    res.push_back(torch::empty({256, 256}, bopt));
    w2t_ptr = BF16PM(res.back());
  }
  hipLaunchKernelGGL(drla_embed_mlp_fwd, dim3(mh_row_tiles(N)), dim3(256), 0,
                     cur_stream(), i64p(pa), BF16P(table), BF16P(b1),
                     BF16P(w2), BF16P(b2), BF16PM(out), BF16PM(a1), N,
                     (int)table.size(0), idx_ptr, w2t_ptr, slab_stride, h_ptr,
                     H, slotp, pa_dist, h_dist);
  return res;
}

// w2t_opt: W2^T from a want_w2t forward (skips the pack launch).
// fuse_scatter: the table scatter runs in the dgrad kernel's epilogue (no
// da1 round trip, no scatter launch).
std::vector<torch::Tensor> embed_mlp_bwd(torch::Tensor dy, torch::Tensor out,
                                         torch::Tensor a1, torch::Tensor w2,
                                         torch::Tensor idx, int64_t A,
                                         c10::optional<torch::Tensor> w2t_opt,
                                         bool fuse_scatter) {
  check_all_gpu_contig("embed bwd input", a1, w2);
  check_gpu_contig(idx, "idx");
  // out (the ReLU-2 mask) may be a column slice of the xh slab
  TORCH_CHECK(out.is_cuda() && out.dim() == 2 && out.size(1) == 256 &&
                  out.stride(1) == 1 && out.stride(0) >= 256,
              "out must be row-contiguous [N,256]");
  const long long out_stride = out.stride(0);
  TORCH_CHECK(idx.scalar_type() == torch::kLong && idx.numel() == out.size(0),
              "idx must be int64 [N]");
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 2 && dy.stride(1) == 1,
              "dy must be row-contiguous");
  const int N = out.size(0);
  const long long n_table = (long long)A * 256;
  auto bopt = a1.options();
  // persistent buffers: W2^T (fully overwritten) and the f32 partial
  // scratch (zero-between-calls; drla_embed_finalize re-zeroes it)
  static torch::Tensor w2t_own, scratch;
  if (!scratch.defined() || scratch.numel() != n_table + 512) {
    scratch = torch::zeros({n_table + 512}, bopt.dtype(torch::kFloat));
  }
  torch::Tensor w2t;
  if (w2t_opt.has_value()) {
    w2t = *w2t_opt;
    check_gpu_contig(w2t, "w2t");
    TORCH_CHECK(w2t.numel() == 65536 && w2t.scalar_type() == w2.scalar_type(),
                "w2t must be bf16 [256,256]");
  } else {
    if (!w2t_own.defined()) w2t_own = torch::empty({65536}, bopt);
    w2t = w2t_own;
    hipLaunchKernelGGL(drla_embed_w2t_pack, dim3(drla_grid(65536)),
                       dim3(DRLA_BLOCK), 0, cur_stream(), BF16P(w2),
                       BF16PM(w2t));
  }
  auto dz2 = torch::empty({N, 256}, bopt);
  float* bias_ws = scratch.data_ptr<float>() + n_table;
  if (fuse_scatter) {
    hipLaunchKernelGGL(drla_embed_mlp_bwd, dim3(mh_row_tiles(N)), dim3(256),
                       0, cur_stream(), BF16P(dy), (long long)dy.stride(0),
                       BF16P(out), BF16P(a1), BF16P(w2t), BF16PM(dz2),
                       (bf16raw*)nullptr, bias_ws, N, i64p(idx),
                       scratch.data_ptr<float>(), (int)A, out_stride);
  } else {
    auto da1 = torch::empty({N, 256}, bopt);
    hipLaunchKernelGGL(drla_embed_mlp_bwd, dim3(mh_row_tiles(N)), dim3(256),
                       0, cur_stream(), BF16P(dy), (long long)dy.stride(0),
                       BF16P(out), BF16P(a1), BF16P(w2t), BF16PM(dz2),
                       BF16PM(da1), bias_ws, N, (const long long*)nullptr,
                       (float*)nullptr, (int)A, out_stride);
    // table scatter into the f32 scratch, then one 3-output finalize
    hipLaunchKernelGGL(
        drla_embed_bwd_scatter, dim3(drla_grid((long long)N * 256)),
        dim3(DRLA_BLOCK), 0, cur_stream(), i64p(idx), BF16P(da1), nullptr,
        scratch.data_ptr<float>(), N, 256, (long long)A);
  }
  auto dtable = torch::empty({A, 256}, bopt);
  auto db1 = torch::empty({256}, bopt);
  auto db2 = torch::empty({256}, bopt);
  hipLaunchKernelGGL(drla_embed_finalize, dim3(drla_grid(n_table + 512)),
                     dim3(DRLA_BLOCK), 0, cur_stream(),
                     scratch.data_ptr<float>(), BF16PM(dtable), BF16PM(db1),
                     BF16PM(db2), n_table);
  return {dz2, dtable, db1, db2};
}

torch::Tensor mlp_heads_pack_wt(std::vector<torch::Tensor> weights,
                                int64_t A) {
  TORCH_CHECK(weights.size() == 6);
  for (auto& w : weights) check_gpu_contig(w, "pack weight");
  auto out = torch::empty({4 * 65536 + 256 * 32 + 256},
                          weights[0].options());
  hipLaunchKernelGGL(drla_heads_wt_pack, dim3(drla_grid(out.numel())),
                     dim3(DRLA_BLOCK), 0, cur_stream(), BF16P(weights[0]),
                     BF16P(weights[1]), BF16P(weights[2]), BF16P(weights[3]),
                     BF16P(weights[4]), BF16P(weights[5]), BF16PM(out),
                     (int)A);
  return out;
}

std::vector<torch::Tensor> mlp_heads_wgrad(
    torch::Tensor dz1p, torch::Tensor dz2p, torch::Tensor dz1v,
    torch::Tensor dz2v, torch::Tensor dlogits, torch::Tensor dvalue,
    torch::Tensor stash, torch::Tensor ws, int64_t A) {
  check_all_gpu_contig("wgrad input", dz1p, dz2p, dz1v, dz2v, dlogits, stash,
                       ws);
  check_gpu_contig(dvalue, "dvalue");
  const int N = dvalue.numel();
  auto bopt = dz1p.options();
  auto dw1p = torch::empty({256, 256}, bopt);
  auto dw2p = torch::empty({256, 256}, bopt);
  auto dw3p = torch::empty({A, 256}, bopt);
  auto dw1v = torch::empty({256, 256}, bopt);
  auto dw2v = torch::empty({256, 256}, bopt);
  auto dw3v = torch::empty({1, 256}, bopt);
  auto db1p = torch::empty({256}, bopt);
  auto db2p = torch::empty({256}, bopt);
  auto db3p = torch::empty({A}, bopt);
  auto db1v = torch::empty({256}, bopt);
  auto db2v = torch::empty({256}, bopt);
  auto db3v = torch::empty({1}, bopt);
  // ws tail = the f32 bias-grad partials written by mlp_heads_bwd
  const float* ws_tail = ws.data_ptr<float>() + (long long)N * 256;
  hipLaunchKernelGGL(drla_heads_wgrad, dim3(73), dim3(256), 0, cur_stream(),
                     BF16P(dz1p), BF16P(dz2p), BF16P(dz1v), BF16P(dz2v),
                     BF16P(dlogits), dvalue.data_ptr<float>(), BF16P(stash),
                     BF16PM(dw1p), BF16PM(dw2p), BF16PM(dw3p), BF16PM(dw1v),
                     BF16PM(dw2v), BF16PM(dw3v), ws_tail, BF16PM(db1p),
                     BF16PM(db2p), BF16PM(db3p), BF16PM(db1v), BF16PM(db2v),
                     BF16PM(db3v), N, (int)A);
  return {dw1p, dw2p, dw3p, dw1v, dw2v, dw3v,
          db1p, db2p, db3p, db1v, db2v, db3v};
}

// ---- LSTM sequence kernels ------------------------------------------------
// Sizes the one-thread-per-gate kernels take keep them (no-grad: 4H <= 1024;
// train pair: Wh resident in LDS, H <= 123); every other size up to
// LSTM_SEQ_MAX_HIDDEN runs the wide family, which streams Wh from global
// memory.
struct LstmSeqGeom { bool wide, wh_in_lds; int block, lds_bytes; };

LstmSeqGeom lstm_seq_geom(int H, const torch::Tensor& Wh, bool wide,
                          bool wh_in_lds) {
  TORCH_CHECK(H >= 1 && H <= LSTM_SEQ_MAX_HIDDEN, "lstm hidden cap is ",
              LSTM_SEQ_MAX_HIDDEN, ", got H=", H);
  TORCH_CHECK(Wh.numel() == (int64_t)drla_lstm_seq_wh_elems(H),
              "Wh must be [H, 4H] for H=", H);
  if (!wide) {
    return {false, wh_in_lds, 4 * H, drla_lstm_seq_lds_bytes(H, wh_in_lds)};
  }
  // the wide kernels read Wh as pairs of bf16
  TORCH_CHECK(reinterpret_cast<uintptr_t>(Wh.data_ptr()) % 4 == 0,
              "lstm wide kernels need a 4-byte aligned Wh");
  return {true, false, LSTM_SEQ_WIDE_BLOCK, drla_lstm_seq_wide_lds_bytes(H)};
}
// no-grad: wide when there are more gates than one block has threads; a Wh
// too large for LDS is read from global memory instead
LstmSeqGeom lstm_seq_geom_nograd(int H, const torch::Tensor& Wh) {
  return lstm_seq_geom(H, Wh, 4 * H > LSTM_SEQ_MAX_GATES,
                       drla_lstm_seq_wh_fits_lds(H));
}
LstmSeqGeom lstm_seq_geom_train(int H, const torch::Tensor& Wh) {
  return lstm_seq_geom(H, Wh, !drla_lstm_seq_train_in_lds(H), true);
}

// the outputs both forward launchers have
struct LstmSeqOut { torch::Tensor h_out, h_fin, c_fin; };
LstmSeqOut lstm_seq_alloc_out(const torch::Tensor& h0, int B, int L, int H) {
  auto fopt = h0.options().dtype(torch::kFloat);
  return {torch::empty({B, L, H}, fopt), torch::empty({B, H}, fopt),
          torch::empty({B, H}, fopt)};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> lstm_seq_fwd(
    torch::Tensor xgates, torch::Tensor Wh, torch::Tensor h0,
    torch::Tensor c0, torch::Tensor done, double forget_bias) {
  check_all_gpu_contig("lstm_seq input", xgates, Wh, h0, c0, done);
  TORCH_CHECK(done.scalar_type() == torch::kBool, "done must be bool");
  const int B = xgates.size(0), L = xgates.size(1);
  const int H = xgates.size(2) / 4;
  const LstmSeqGeom geom = lstm_seq_geom_nograd(H, Wh);
  const DualPtr xg = dual_ptr(xgates);
  auto out = lstm_seq_alloc_out(h0, B, L, H);
  hipLaunchKernelGGL(
      geom.wide ? drla_lstm_seq_wide_fwd
                : geom.wh_in_lds ? drla_lstm_seq_fwd : drla_lstm_seq_fwd_gmem,
      dim3(B), dim3(geom.block), geom.lds_bytes, cur_stream(), xg.bf16,
      xg.f32, BF16P(Wh), h0.data_ptr<float>(), c0.data_ptr<float>(),
      boolp(done), out.h_out.data_ptr<float>(), out.h_fin.data_ptr<float>(),
      out.c_fin.data_ptr<float>(), static_cast<float>(forget_bias), B, L, H);
  return {out.h_out, out.h_fin, out.c_fin};
}

void grad_gather(torch::Tensor srcs, torch::Tensor offs,
                 torch::Tensor sizes, torch::Tensor dst,
                 c10::optional<torch::Tensor> norm_ws) {
  check_gpu_contig(dst, "dst");
  TORCH_CHECK(dst.scalar_type() == torch::kBFloat16,
              "grad_gather wants a bf16 flat bucket");
  TORCH_CHECK(dst.numel() % 8 == 0, "flat bucket must be 8-aligned");
  for (auto* t : {&srcs, &offs, &sizes}) {
    check_gpu_contig(*t, "gather table");
    TORCH_CHECK(t->scalar_type() == torch::kLong, "table must be int64");
  }
  const long long chunks = dst.numel() / 8;
  float* nw = nullptr;
  int nw_n = 0;
  if (norm_ws.has_value()) {
    check_gpu_contig(*norm_ws, "norm_ws");
    nw = norm_ws->data_ptr<float>();
    nw_n = (int)norm_ws->numel();
  }
  hipLaunchKernelGGL(
      drla_grad_gather, dim3(drla_grid(chunks)), dim3(DRLA_BLOCK), 0,
      cur_stream(), u64p(srcs), i64p(offs), i64p(sizes), BF16PM(dst),
      (int)srcs.numel(), chunks, nw, nw_n);
}

std::vector<torch::Tensor> lstm_seq_train_fwd(
    torch::Tensor xg, torch::Tensor Wh, torch::Tensor h0, torch::Tensor c0,
    torch::Tensor done, double forget_bias) {
  check_all_gpu_contig("lstm_seq_train input", xg, Wh, h0, c0, done);
  const int B = xg.size(0), L = xg.size(1), H = xg.size(2) / 4;
  const LstmSeqGeom geom = lstm_seq_geom_train(H, Wh);
  auto out = lstm_seq_alloc_out(h0, B, L, H);
  auto acts = torch::empty({B, L, 4 * H}, out.h_out.options());
  auto c_prev = torch::empty({B, L, H}, out.h_out.options());
  auto h_prev = torch::empty({B, L, H}, xg.options());
  hipLaunchKernelGGL(
      geom.wide ? drla_lstm_seq_wide_train_fwd : drla_lstm_seq_train_fwd,
      dim3(B), dim3(geom.block), geom.lds_bytes, cur_stream(), BF16P(xg),
      BF16P(Wh), h0.data_ptr<float>(), c0.data_ptr<float>(), boolp(done),
      out.h_out.data_ptr<float>(), out.h_fin.data_ptr<float>(),
      out.c_fin.data_ptr<float>(), acts.data_ptr<float>(),
      c_prev.data_ptr<float>(), BF16PM(h_prev),
      static_cast<float>(forget_bias), B, L, H);
  return {out.h_out, out.h_fin, out.c_fin, acts, c_prev, h_prev};
}

std::vector<torch::Tensor> lstm_seq_train_bwd(
    torch::Tensor dh_out, c10::optional<torch::Tensor> dh_fin,
    c10::optional<torch::Tensor> dc_fin, torch::Tensor acts,
    torch::Tensor c_prev, torch::Tensor Wh, torch::Tensor done) {
  check_all_gpu_contig("lstm_seq_train bwd input", dh_out, acts, c_prev, Wh,
                       done);
  const int B = acts.size(0), L = acts.size(1), H = acts.size(2) / 4;
  const LstmSeqGeom geom = lstm_seq_geom_train(H, Wh);
  auto fopt = dh_out.options().dtype(torch::kFloat);
  auto dxg = torch::empty({B, L, 4 * H},
                          dh_out.options().dtype(torch::kBFloat16));
  auto dh0 = torch::empty({B, H}, fopt);
  auto dc0 = torch::empty({B, H}, fopt);
  hipLaunchKernelGGL(
      geom.wide ? drla_lstm_seq_wide_train_bwd : drla_lstm_seq_train_bwd,
      dim3(B), dim3(geom.block), geom.lds_bytes, cur_stream(),
      dh_out.data_ptr<float>(),
      dh_fin.has_value() ? dh_fin->data_ptr<float>() : nullptr,
      dc_fin.has_value() ? dc_fin->data_ptr<float>() : nullptr,
      acts.data_ptr<float>(), c_prev.data_ptr<float>(), BF16P(Wh),
      boolp(done), BF16PM(dxg), dh0.data_ptr<float>(), dc0.data_ptr<float>(),
      B, L, H);
  return {dxg, dh0, dc0};
}

torch::Tensor sq_norm(torch::Tensor x) {
  check_gpu_contig(x, "x");
  TORCH_CHECK(x.scalar_type() == torch::kFloat, "sq_norm wants float32");
  // DRLA_NORM_SLOTS cache-line-spread partials (total = .sum())
  auto out = torch::zeros({DRLA_NORM_SLOTS * 16}, x.options());
  hipLaunchKernelGGL(drla_sq_norm, dim3(drla_grid(x.numel() / 4 + 1)),
                     dim3(DRLA_BLOCK), 0, cur_stream(), x.data_ptr<float>(),
                     out.data_ptr<float>(), (long long)x.numel());
  return out;
}

torch::Tensor sq_norm_bf16(torch::Tensor x) {
  check_gpu_contig(x, "x");
  auto out = torch::zeros({DRLA_NORM_SLOTS * 16},
                          x.options().dtype(torch::kFloat));
  hipLaunchKernelGGL(drla_sq_norm_bf16, dim3(drla_grid(x.numel() / 4 + 1)),
                     dim3(DRLA_BLOCK), 0, cur_stream(), BF16P(x),
                     out.data_ptr<float>(), (long long)x.numel());
  return out;
}

void rmsprop_step_bf16_t(torch::Tensor p, torch::Tensor g,
                         torch::Tensor master, torch::Tensor ms, double clip,
                         torch::Tensor lr_buf, double rho, double eps,
                         c10::optional<torch::Tensor> norm_ws) {
  check_all_gpu_contig("rmsprop bf16 tensor", p, g, master, ms, lr_buf);
  const long long n = p.numel();
  torch::Tensor norm_buf;
  if (norm_ws.has_value() && clip > 0) {
    // persistent buffer, zeroed by grad_gather earlier on this stream
    norm_buf = *norm_ws;
    hipLaunchKernelGGL(drla_sq_norm_bf16,
                       dim3(drla_grid(g.numel() / 4 + 1)), dim3(DRLA_BLOCK),
                       0, cur_stream(), BF16P(g),
                       norm_buf.data_ptr<float>(), (long long)g.numel());
  } else if (clip > 0) {
    norm_buf = sq_norm_bf16(g);
  } else {
    norm_buf = torch::zeros({DRLA_NORM_SLOTS * 16}, master.options());
  }
  hipLaunchKernelGGL(drla_rmsprop_step_bf16, dim3(drla_grid(n)),
                     dim3(DRLA_BLOCK), 0, cur_stream(), BF16PM(p), BF16P(g),
                     master.data_ptr<float>(), ms.data_ptr<float>(),
                     norm_buf.data_ptr<float>(), static_cast<float>(clip),
                     lr_buf.data_ptr<float>(), static_cast<float>(rho),
                     static_cast<float>(eps), n);
}

void adam_step_bf16_t(torch::Tensor p, torch::Tensor g, torch::Tensor master,
                      torch::Tensor m, torch::Tensor v, double clip,
                      torch::Tensor lr_buf, double beta1, double beta2,
                      double eps) {
  check_all_gpu_contig("adam bf16 tensor", p, g, master, m, v, lr_buf);
  const long long n = p.numel();
  torch::Tensor norm_buf;
  if (clip > 0) {
    norm_buf = sq_norm_bf16(g);
  } else {
    norm_buf = torch::zeros({1}, master.options());
  }
  hipLaunchKernelGGL(drla_adam_step_bf16, dim3(drla_grid(n)),
                     dim3(DRLA_BLOCK), 0, cur_stream(), BF16PM(p), BF16P(g),
                     master.data_ptr<float>(), m.data_ptr<float>(),
                     v.data_ptr<float>(), norm_buf.data_ptr<float>(),
                     static_cast<float>(clip), lr_buf.data_ptr<float>(),
                     static_cast<float>(beta1), static_cast<float>(beta2),
                     static_cast<float>(eps), n);
}

void rmsprop_step_t(torch::Tensor p, torch::Tensor g, torch::Tensor ms,
                    double clip, torch::Tensor lr_buf, double rho,
                    double eps) {
  check_all_gpu_contig("rmsprop tensor", p, g, ms, lr_buf);
  const long long n = p.numel();
  torch::Tensor norm_buf;
  if (clip > 0) {
    norm_buf = sq_norm(g);
  } else {
    norm_buf = torch::zeros({1}, p.options());
  }
  hipLaunchKernelGGL(drla_rmsprop_step, dim3(drla_grid(n)), dim3(DRLA_BLOCK),
                     0, cur_stream(), p.data_ptr<float>(),
                     g.data_ptr<float>(), ms.data_ptr<float>(),
                     norm_buf.data_ptr<float>(), static_cast<float>(clip),
                     lr_buf.data_ptr<float>(), static_cast<float>(rho),
                     static_cast<float>(eps), n);
}

void rmsprop_step(torch::Tensor p, torch::Tensor g, torch::Tensor ms,
                  double clip, double lr, double rho, double eps) {
  auto lr_buf = torch::full({1}, lr, p.options());
  rmsprop_step_t(p, g, ms, clip, lr_buf, rho, eps);
}

void adam_step_t(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                 torch::Tensor v, double clip, torch::Tensor lr_buf,
                 double beta1, double beta2, double eps) {
  check_all_gpu_contig("adam tensor", p, g, m, v, lr_buf);
  const long long n = p.numel();
  torch::Tensor norm_buf;
  if (clip > 0) {
    norm_buf = sq_norm(g);
  } else {
    norm_buf = torch::zeros({1}, p.options());
  }
  hipLaunchKernelGGL(drla_adam_step, dim3(drla_grid(n)), dim3(DRLA_BLOCK), 0,
                     cur_stream(), p.data_ptr<float>(), g.data_ptr<float>(),
                     m.data_ptr<float>(), v.data_ptr<float>(),
                     norm_buf.data_ptr<float>(), static_cast<float>(clip),
                     lr_buf.data_ptr<float>(), static_cast<float>(beta1),
                     static_cast<float>(beta2), static_cast<float>(eps), n);
}

void adam_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
               torch::Tensor v, double clip, double lr_t, double beta1,
               double beta2, double eps) {
  auto lr_buf = torch::full({1}, lr_t, p.options());
  adam_step_t(p, g, m, v, clip, lr_buf, beta1, beta2, eps);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("normalize_frames_f32", &normalize_frames_f32,
        "uint8 frames -> float32/255 (K11)");
  m.def("normalize_frames_bf16", &normalize_frames_bf16,
        "uint8 frames -> bf16/255 (K11)");
  m.def("vtrace_scan", &vtrace_scan, "fused V-trace reverse scan (K5)");
  // underscore: a helper of runtime/graphed.py, not part of the op surface
  m.def("_set_lr_slot", &set_lr_slot,
        "write the learning rate and the input-slot word in one launch");
  m.def("vtrace_loss_fwd", &vtrace_loss_fwd,
        "fused IMPALA loss pipeline forward (K5+K7+K13); nofill: ticketed "
        "fixed-order loss sums, no zero-fill; stash_actions: also returns "
        "a copy of actions made in-kernel",
        py::arg("logits"), py::arg("value"), py::arg("mu"),
        py::arg("actions"), py::arg("rewards"), py::arg("done"),
        py::arg("gamma"), py::arg("clip_mode"), py::arg("c_bl"),
        py::arg("c_ent"), py::arg("nofill") = false,
        py::arg("stash_actions") = false, py::arg("slot") = py::none(),
        py::arg("slot_dist") = std::vector<int64_t>{});
  m.def("vtrace_loss_bwd", &vtrace_loss_bwd,
        "fused IMPALA loss pipeline backward (closed form)");
  m.def("mfma_probe", &mfma_probe, "16x16x32 bf16 MFMA layout probe");
  m.def("conv_fwd", &conv_fwd,
        "MFMA implicit-GEMM conv fwd, fused normalize+bias+ReLU (K1)",
        py::arg("layer"), py::arg("x"), py::arg("w"), py::arg("bias"),
        py::arg("stash_input"), py::arg("out_slab") = py::none(),
        py::arg("slot") = py::none(),
        py::arg("slot_dist") = std::vector<int64_t>{},
        py::arg("relu_in") = false, py::arg("residual") = py::none());
  m.def("conv_wgrad", &conv_wgrad,
        "MFMA conv weight + bias gradient (K1 bwd; layers 4..8: 3x3 family)",
        py::arg("layer"), py::arg("x"), py::arg("dy"),
        py::arg("relu_in") = false);
  m.def("_conv_wgrad_split", &conv_wgrad_split,
        "M-split of the conv wgrad grid for a layer");
  m.def("conv_dgrad", &conv_dgrad, "MFMA conv data gradient (K1 bwd)",
        py::arg("layer"), py::arg("dy"), py::arg("w"),
        py::arg("mask_src") = py::none(), py::arg("addend") = py::none());
  m.def("relu_mask_bwd", &relu_mask_bwd,
        "fused-ReLU backward mask + bias gradient");
  m.def("dqn_loss_fwd", &dqn_loss_fwd,
        "fused double-DQN target + IS-weighted TD loss (K8)");
  m.def("dqn_loss_bwd", &dqn_loss_bwd, "closed-form K8 backward");
  m.def("a2c_loss_fwd", &a2c_loss_fwd, "fused A2C loss fwd (K6)");
  m.def("a2c_loss_bwd", &a2c_loss_bwd, "fused A2C loss bwd (K6)");
  m.def("r2d2_loss_fwd", &r2d2_loss_fwd,
        "fused R2D2 sequence-TD tail fwd (K9; n_step > 1 or "
        "priority_eta >= 0 selects the n-step kernel)",
        py::arg("mq"), py::arg("tq"), py::arg("actions"), py::arg("rewards"),
        py::arg("done"), py::arg("weights"), py::arg("gamma"),
        py::arg("clip_mode"), py::arg("n_step") = 1,
        py::arg("priority_eta") = -1.0);
  m.def("dhead_train_fwd", &dhead_train_fwd,
        "grad-carrying dueling head fwd (R2D2 trained window)");
  m.def("dhead_train_bwd", &dhead_train_bwd,
        "grad-carrying dueling head bwd chain + weight grads");
  m.def("dueling_head_fwd", &dueling_head_fwd,
        "no-grad dueling head over the post-burn-in window");
  m.def("r2d2_loss_bwd", &r2d2_loss_bwd,
        "fused R2D2 sequence-TD tail bwd (K9)");
  m.def("per_update", &per_update, "GPU PER segment-tree batched update");
  m.def("per_sample", &per_sample, "GPU PER stratified sample descent");
  m.def("multi_gather", &multi_gather,
        "one-kernel replay batch gather (all fields)");
  m.def("per_rebuild", &per_rebuild,
        "GPU PER interior-sum rebuild (float32 drift repair)");
  m.def("embed_bwd", &embed_bwd,
        "action-embedding table gradient (K2 backward)");
  m.def("lstm_tail_fwd", &lstm_tail_fwd, "fused LSTM gate tail fwd (K3)",
        py::arg("gates"), py::arg("c_prev"), py::arg("forget_bias"),
        py::arg("stash_c") = false, py::arg("slot") = py::none(),
        py::arg("slot_dist") = std::vector<int64_t>{});
  m.def("lstm_tail_bwd", &lstm_tail_bwd, "fused LSTM gate tail bwd (K3)");
  m.def("mlp_heads_fwd", &mlp_heads_fwd,
        "fused policy+value MLP heads forward (K4)",
        py::arg("h"), py::arg("weights"), py::arg("biases"), py::arg("A"),
        py::arg("want_bwd_bufs") = false);
  m.def("mlp_heads_bwd", &mlp_heads_bwd,
        "fused heads dgrad chain + ReLU masks + bias grads (K4 bwd)",
        py::arg("dlogits"), py::arg("dvalue"), py::arg("stash"),
        py::arg("weights"), py::arg("A"), py::arg("ws") = py::none());
  m.def("embed_mlp_fwd", &embed_mlp_fwd,
        "fused action-embedding MLP forward (K2)",
        py::arg("pa"), py::arg("table"), py::arg("b1"), py::arg("w2"),
        py::arg("b2"), py::arg("stash_idx") = false,
        py::arg("want_w2t") = false, py::arg("xh_slab") = py::none(),
        py::arg("emb_col") = 0, py::arg("h") = py::none(),
        py::arg("slot") = py::none(),
        py::arg("slot_dist") = std::vector<int64_t>{});
  m.def("embed_mlp_bwd", &embed_mlp_bwd,
        "fused action-embedding MLP backward (K2 bwd)",
        py::arg("dy"), py::arg("out"), py::arg("a1"), py::arg("w2"),
        py::arg("idx"), py::arg("A"), py::arg("w2t") = py::none(),
        py::arg("fuse_scatter") = false);
  m.def("mlp_heads_pack_wt", &mlp_heads_pack_wt,
        "one-kernel transposed-weight pack for the heads dgrad");
  m.def("mlp_heads_wgrad", &mlp_heads_wgrad,
        "all six head wgrads (dW = dz^T @ act) in one MFMA launch");
  m.def("lstm_seq_train_fwd", &lstm_seq_train_fwd,
        "grad-carrying whole-sequence LSTM forward (K3 seq, R2D2 train)");
  m.def("lstm_seq_train_bwd", &lstm_seq_train_bwd,
        "whole-sequence LSTM backward (one kernel over the recurrence)");
  m.def("lstm_seq_fwd", &lstm_seq_fwd,
        "whole no-grad LSTM unroll in one kernel (K3 seq / burn-in)");
  m.def("sq_norm", &sq_norm, "squared L2 norm of a flat tensor (K12)");
  m.def("grad_gather", &grad_gather,
        "one-kernel scattered-grad -> flat bucket pack (K12b)");
  m.def("rmsprop_step", &rmsprop_step,
        "fused global-norm-clip + TF-RMSProp update (K12)");
  m.def("rmsprop_step_t", &rmsprop_step_t,
        "RMSProp update with device-tensor lr (hipGraph-safe)");
  m.def("adam_step", &adam_step,
        "fused global-norm-clip + TF-Adam update (K12)");
  m.def("adam_step_t", &adam_step_t,
        "Adam update with device-tensor lr_t (hipGraph-safe)");
  m.def("sq_norm_bf16", &sq_norm_bf16, "squared L2 norm of a bf16 tensor");
  m.def("rmsprop_step_bf16_t", &rmsprop_step_bf16_t,
        "bf16-model/fp32-master RMSProp (K12, mixed precision)");
  m.def("adam_step_bf16_t", &adam_step_bf16_t,
        "bf16-model/fp32-master Adam (K12, mixed precision)");
}
