// The one declaration of every drla kernel, grouped by the .hip file that
// defines it. Every .hip file and bind.cpp include this header: the kernels
// are extern "C" (no type in the symbol), so a definition and a launch site
// can only be held to the same signature by the compiler seeing this
// declaration next to both — a mismatch is a "conflicting types" error.
// __launch_bounds__ and __restrict__ live on the definitions.
// Keep it cheap: hip_runtime.h + drla_common.h only, never torch.
#pragma once

#include <hip/hip_runtime.h>

#include "drla_common.h"

#define DRLA_KERNEL extern "C" __global__ void

// ---- elementwise.hip ------------------------------------------------------
DRLA_KERNEL drla_set_lr_slot(float*, int*, float, int);
DRLA_KERNEL drla_u8_normalize_f32(const uchar4*, float4*, long long);
DRLA_KERNEL drla_u8_normalize_bf16(const uchar4*, ushort4v*, long long);
DRLA_KERNEL drla_u8_normalize_f32_tail(const unsigned char*, float*,
                                       long long, long long);
DRLA_KERNEL drla_u8_normalize_bf16_tail(const unsigned char*, bf16raw*,
                                        long long, long long);
DRLA_KERNEL drla_embed_bwd_scatter(const long long*, const bf16raw*,
                                   const float*, float*, long long, int,
                                   long long);
DRLA_KERNEL drla_f32_to_bf16_zero_kernel(float*, bf16raw*, long long);

// ---- vtrace.hip -----------------------------------------------------------
DRLA_KERNEL drla_vtrace_scan(const float*, const float*, const float*,
                             float*, int, int);

// ---- vtrace_loss.hip ------------------------------------------------------
DRLA_KERNEL drla_vtrace_loss_fwd(
    const bf16raw*, const float*, const float*, const float*, const int*,
    const float*, const unsigned char*, float, int, float, float, float*,
    float*, float*, float*, int, int, int, float*, unsigned int*, int*,
    const int*, long long, long long, long long, long long);
DRLA_KERNEL drla_vtrace_loss_bwd(
    const float*, const float*, const float*, const float*, const int*,
    const float*, int, float, float, bf16raw*, float*, float*, int, int,
    int);

// ---- lstm_gates.hip -------------------------------------------------------
DRLA_KERNEL drla_lstm_tail_fwd(const float*, const float*, float*, float*,
                               float*, float, long long, int, float*,
                               const int*, long long);
DRLA_KERNEL drla_lstm_tail_bwd(const float*, const float*, const float*,
                               const float*, const float*, float*, float*,
                               long long, int, long long);
DRLA_KERNEL drla_lstm_tail_fwd_bf16(const bf16raw*, const float*, float*,
                                    float*, float*, float, long long, int,
                                    float*, const int*, long long);
DRLA_KERNEL drla_lstm_tail_bwd_bf16(const float*, const float*, const float*,
                                    const float*, const float*, bf16raw*,
                                    float*, long long, int, long long);
DRLA_KERNEL drla_lstm_seq_fwd(
    const bf16raw*, const float*, const bf16raw*, const float*, const float*,
    const unsigned char*, float*, float*, float*, float, int, int, int);
DRLA_KERNEL drla_lstm_seq_fwd_gmem(
    const bf16raw*, const float*, const bf16raw*, const float*, const float*,
    const unsigned char*, float*, float*, float*, float, int, int, int);
DRLA_KERNEL drla_lstm_seq_train_fwd(
    const bf16raw*, const bf16raw*, const float*, const float*,
    const unsigned char*, float*, float*, float*, float*, float*, bf16raw*,
    float, int, int, int);
DRLA_KERNEL drla_lstm_seq_train_bwd(
    const float*, const float*, const float*, const float*, const float*,
    const bf16raw*, const unsigned char*, bf16raw*, float*, float*, int, int,
    int);
DRLA_KERNEL drla_lstm_seq_wide_fwd(
    const bf16raw*, const float*, const bf16raw*, const float*, const float*,
    const unsigned char*, float*, float*, float*, float, int, int, int);
DRLA_KERNEL drla_lstm_seq_wide_train_fwd(
    const bf16raw*, const bf16raw*, const float*, const float*,
    const unsigned char*, float*, float*, float*, float*, float*, bf16raw*,
    float, int, int, int);
DRLA_KERNEL drla_lstm_seq_wide_train_bwd(
    const float*, const float*, const float*, const float*, const float*,
    const bf16raw*, const unsigned char*, bf16raw*, float*, float*, int, int,
    int);

// ---- optim.hip ------------------------------------------------------------
DRLA_KERNEL drla_sq_norm(const float*, float*, long long);
DRLA_KERNEL drla_sq_norm_bf16(const bf16raw*, float*, long long);
DRLA_KERNEL drla_rmsprop_step(float*, const float*, float*, const float*,
                              float, const float*, float, float, long long);
DRLA_KERNEL drla_rmsprop_step_bf16(bf16raw*, const bf16raw*, float*, float*,
                                   const float*, float, const float*, float,
                                   float, long long);
DRLA_KERNEL drla_adam_step(float*, const float*, float*, float*,
                           const float*, float, const float*, float, float,
                           float, long long);
DRLA_KERNEL drla_adam_step_bf16(bf16raw*, const bf16raw*, float*, float*,
                                float*, const float*, float, const float*,
                                float, float, float, long long);
DRLA_KERNEL drla_grad_gather(const unsigned long long*, const long long*,
                             const long long*, bf16raw*, int, long long,
                             float*, int);

// ---- conv.hip (layer order = DRLA_CONV_LAYERS) ----------------------------
DRLA_KERNEL drla_mfma_probe(const bf16raw*, const bf16raw*, float*);
DRLA_KERNEL drla_conv_fwd_l1(const unsigned char*, const bf16raw*,
                             const bf16raw*, bf16raw*, int, unsigned char*,
                             const int*, long long);
DRLA_KERNEL drla_conv_fwd_l1_c1(const unsigned char*, const bf16raw*,
                                const bf16raw*, bf16raw*, int,
                                unsigned char*, const int*, long long);
DRLA_KERNEL drla_conv_fwd_l2(const bf16raw*, const bf16raw*, const bf16raw*,
                             bf16raw*, int, long long);
DRLA_KERNEL drla_conv_fwd_l3(const bf16raw*, const bf16raw*, const bf16raw*,
                             bf16raw*, int, long long);
DRLA_KERNEL drla_relu_mask_bwd(const bf16raw*, const bf16raw*, bf16raw*,
                               float*, long long, int, long long, long long,
                               long long);
DRLA_KERNEL drla_wgrad_finalize(float*, bf16raw*, int, int, float*,
                                bf16raw*);
DRLA_KERNEL drla_conv_wgrad_l1(const unsigned char*, const bf16raw*, float*,
                               int);
DRLA_KERNEL drla_conv_wgrad_l1_c1(const unsigned char*, const bf16raw*,
                                  float*, int);
DRLA_KERNEL drla_conv_wgrad_l2(const bf16raw*, const bf16raw*, float*, int);
DRLA_KERNEL drla_conv_wgrad_l3(const bf16raw*, const bf16raw*, float*, int);
DRLA_KERNEL drla_conv_dgrad_l2(const bf16raw*, const bf16raw*, bf16raw*,
                               int);
DRLA_KERNEL drla_conv_dgrad_l3(const bf16raw*, const bf16raw*, bf16raw*,
                               int);

// ---- conv3x3.hip (geometry order = DRLA_CONV3_LAYERS) ---------------------
// fwd and dgrad: in, w, bias, mask, residual/addend, out, batch, relu_in
DRLA_KERNEL drla_c3_fwd_4_16_84(const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, bf16raw*, int, int);
DRLA_KERNEL drla_c3_fwd_16_16_42(const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, bf16raw*, int, int);
DRLA_KERNEL drla_c3_fwd_16_32_42(const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, bf16raw*, int, int);
DRLA_KERNEL drla_c3_fwd_32_32_21(const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, bf16raw*, int, int);
DRLA_KERNEL drla_c3_fwd_32_32_11(const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, bf16raw*, int, int);
DRLA_KERNEL drla_c3_dgrad_16_16_42(const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, bf16raw*, int, int);
DRLA_KERNEL drla_c3_dgrad_16_32_42(const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, bf16raw*, int, int);
DRLA_KERNEL drla_c3_dgrad_32_32_21(const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, bf16raw*, int, int);
DRLA_KERNEL drla_c3_dgrad_32_32_11(const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, bf16raw*, int, int);
// wgrad: in, dy, scratch, batch, relu_in
DRLA_KERNEL drla_c3_wgrad_4_16_84(const bf16raw*, const bf16raw*, float*,
    int, int);
DRLA_KERNEL drla_c3_wgrad_16_16_42(const bf16raw*, const bf16raw*, float*,
    int, int);
DRLA_KERNEL drla_c3_wgrad_16_32_42(const bf16raw*, const bf16raw*, float*,
    int, int);
DRLA_KERNEL drla_c3_wgrad_32_32_21(const bf16raw*, const bf16raw*, float*,
    int, int);
DRLA_KERNEL drla_c3_wgrad_32_32_11(const bf16raw*, const bf16raw*, float*,
    int, int);
DRLA_KERNEL drla_c3_wgrad_finalize(float*, bf16raw*, bf16raw*, int, int);

// ---- per_tree.hip ---------------------------------------------------------
DRLA_KERNEL drla_per_update(float*, const long long*, const float*, int,
                            long long);
DRLA_KERNEL drla_per_rebuild_level(float*, long long, long long);
DRLA_KERNEL drla_multi_gather(const long long*, const unsigned long long*,
                              const unsigned long long*, const long long*,
                              int);
DRLA_KERNEL drla_per_sample(const float*, const float*, const float*,
                            long long*, float*, int, long long);

// ---- dqn_loss.hip ---------------------------------------------------------
DRLA_KERNEL drla_dqn_loss_fwd(
    const bf16raw*, const float*, const float*, const float*, const int*,
    const float*, const float*, const float*, float*, float*, int, int);
DRLA_KERNEL drla_dqn_loss_bwd(const float*, const int*, const float*,
                              const float*, bf16raw*, float*, int, int);

// ---- a2c_loss.hip ---------------------------------------------------------
DRLA_KERNEL drla_a2c_loss_fwd(
    const bf16raw*, const float*, const float*, const float*, const int*,
    const float*, const unsigned char*, float, int, float, float, float*,
    float*, float*, int, int);
DRLA_KERNEL drla_a2c_loss_bwd(const float*, const float*, const int*,
                              const float*, int, float, float, bf16raw*,
                              float*, float*, int, int);

// ---- r2d2_loss.hip --------------------------------------------------------
DRLA_KERNEL drla_r2d2_loss_fwd(
    const bf16raw*, const float*, const bf16raw*, const float*, const int*,
    const float*, const unsigned char*, const float*, float, int, float*,
    float*, float*, int, int, int);
DRLA_KERNEL drla_r2d2_nstep_loss_fwd(
    const bf16raw*, const float*, const bf16raw*, const float*, const int*,
    const float*, const unsigned char*, const float*, float, int, int, float,
    float*, float*, float*, int, int, int);
DRLA_KERNEL drla_r2d2_loss_bwd(const float*, const int*, const float*,
                               const float*, bf16raw*, float*, int, int,
                               int);
DRLA_KERNEL drla_dueling_head_fwd(
    const float*, const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, bf16raw*, int, int, int, int, int, int);
DRLA_KERNEL drla_dhead_train_fwd(
    const float*, const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, bf16raw*, bf16raw*, int, int, int, int);
DRLA_KERNEL drla_dhead_train_bwd(
    const bf16raw*, const bf16raw*, const float*, const bf16raw*,
    const bf16raw*, float*, float*, int, int, int, int);
DRLA_KERNEL drla_dhead_train_fin(const float*, bf16raw*, bf16raw*, bf16raw*,
                                 bf16raw*, int, int, int);

// ---- mlp_heads.hip --------------------------------------------------------
DRLA_KERNEL drla_mlp_heads_fwd(
    const float*, const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, bf16raw*, float*, bf16raw*, int, int, bf16raw*, float*);
DRLA_KERNEL drla_mlp_heads_bwd(
    const bf16raw*, const float*, const bf16raw*, const bf16raw*,
    const bf16raw*, const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, bf16raw*, bf16raw*, bf16raw*, bf16raw*, float*, float*,
    float*, float*, float*, float*, float*, int, int);
DRLA_KERNEL drla_heads_wt_pack(const bf16raw*, const bf16raw*,
                               const bf16raw*, const bf16raw*,
                               const bf16raw*, const bf16raw*, bf16raw*,
                               int);
DRLA_KERNEL drla_heads_wgrad(
    const bf16raw*, const bf16raw*, const bf16raw*, const bf16raw*,
    const bf16raw*, const float*, const bf16raw*, bf16raw*, bf16raw*,
    bf16raw*, bf16raw*, bf16raw*, bf16raw*, const float*, bf16raw*,
    bf16raw*, bf16raw*, bf16raw*, bf16raw*, bf16raw*, int, int);
DRLA_KERNEL drla_embed_mlp_fwd(const long long*, const bf16raw*,
                               const bf16raw*, const bf16raw*,
                               const bf16raw*, bf16raw*, bf16raw*, int, int,
                               long long*, bf16raw*, long long, const float*,
                               int, const int*, long long, long long);
DRLA_KERNEL drla_embed_w2t_pack(const bf16raw*, bf16raw*);
DRLA_KERNEL drla_embed_mlp_bwd(const bf16raw*, long long, const bf16raw*,
                               const bf16raw*, const bf16raw*, bf16raw*,
                               bf16raw*, float*, int, const long long*,
                               float*, int, long long);
DRLA_KERNEL drla_embed_finalize(float*, bf16raw*, bf16raw*, bf16raw*,
                                long long);

#undef DRLA_KERNEL
