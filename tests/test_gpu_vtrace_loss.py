"""Fused V-trace loss kernel pair vs the torch composition (same GPU data):
forward losses and analytic backward gradients. GPU-only."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _torch_composed(logits, value, mu, actions, rewards, discounts,
                    c_b, c_e):
    """The CPU-path composition (algorithms/vtrace.py) evaluated on GPU
    tensors in fp32 — the golden reference."""
    from distributed_reinforcement_learning_amd.algorithms import vtrace
    policy = torch.softmax(logits.float(), dim=-1)
    p_f, p_m, _ = vtrace.split_data(policy)
    v_f, v_m, v_l = vtrace.split_data(value)
    a_f, a_m, _ = vtrace.split_data(actions)
    r_f, r_m, _ = vtrace.split_data(rewards)
    g_f, g_m, _ = vtrace.split_data(discounts)
    mu_f, mu_m, _ = vtrace.split_data(mu)
    vs, rho = vtrace.from_softmax(mu_f, p_f, a_f, g_f, r_f, v_f, v_m)
    vs1, _ = vtrace.from_softmax(mu_m, p_m, a_m, g_m, r_m, v_m, v_l)
    adv = (rho * (r_f + g_f * vs1 - v_f)).detach()
    pi = vtrace.compute_policy_gradient_loss(p_f, a_f, adv)
    bl = vtrace.compute_baseline_loss(vs, v_f)
    ent = vtrace.compute_entropy_loss(p_f)
    return pi, bl, ent


# trajectory-length cap of the fused kernel (VT_MAX_T in ops/hip/drla_common.h:
# it sizes the kernel's LDS scan buffers and the launcher's check)
VT_MAX_T = 128


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_vtrace_loss_matches_torch(dtype):
    _check_fused_vtrace_loss(dtype, 8, 12, 18)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_vtrace_loss_at_the_trajectory_cap(dtype):
    """T = VT_MAX_T fills the kernel's LDS scan buffers exactly; one
    block, two actions."""
    _check_fused_vtrace_loss(dtype, 1, VT_MAX_T, 2)


def test_fused_vtrace_loss_refuses_past_the_trajectory_cap():
    from distributed_reinforcement_learning_amd.ops import fused_vtrace_loss
    B, T, A = 1, VT_MAX_T + 1, 2
    logits = torch.zeros(B, T, A, device="cuda")
    with pytest.raises(RuntimeError, match=f"trajectory cap is {VT_MAX_T}"):
        fused_vtrace_loss(
            logits, torch.zeros(B, T, device="cuda"),
            torch.full((B, T, A), 0.5, device="cuda"),
            torch.zeros(B, T, dtype=torch.long, device="cuda"),
            torch.zeros(B, T, device="cuda"),
            torch.zeros(B, T, dtype=torch.bool, device="cuda"), 0.99,
            "abs_one", 0.7, 0.03)


def _check_fused_vtrace_loss(dtype, B, T, A):
    from distributed_reinforcement_learning_amd.ops import fused_vtrace_loss
    torch.manual_seed(0)
    c_b, c_e = 0.7, 0.03
    logits = (torch.randn(B, T, A, device="cuda") * 2).to(dtype)
    logits_f = logits.detach().clone().requires_grad_(True)
    logits_g = logits.detach().clone().requires_grad_(True)
    value = torch.randn(B, T, device="cuda")
    value_f = value.detach().clone().requires_grad_(True)
    value_g = value.detach().clone().requires_grad_(True)
    mu = torch.softmax(torch.randn(B, T, A, device="cuda"), -1)
    actions = torch.randint(0, A, (B, T), device="cuda")
    rewards = torch.randn(B, T, device="cuda") * 2.0
    done = torch.rand(B, T, device="cuda") < 0.1
    discounts = (~done).float() * 0.99

    # the fused path clips in-kernel (abs_one) and folds the coef-combined
    # total; backward through total exercises the from_total fast path
    pi_g, bl_g, ent_g, total_g = fused_vtrace_loss(
        logits_g, value_g, mu, actions, rewards, done, 0.99, "abs_one",
        c_b, c_e)
    total_g.backward()
    rewards = rewards.clamp(-1, 1)

    pi_f, bl_f, ent_f = _torch_composed(logits_f, value_f, mu, actions,
                                        rewards, discounts, c_b, c_e)
    total_f = pi_f + c_b * bl_f + c_e * ent_f
    total_f.backward()
    assert float(total_g) == pytest.approx(float(total_f), rel=5e-3,
                                           abs=2e-2)

    rtol = 2e-4 if dtype == torch.float32 else 2e-3
    assert float(pi_g) == pytest.approx(float(pi_f), rel=rtol, abs=1e-2)
    assert float(bl_g) == pytest.approx(float(bl_f), rel=rtol, abs=1e-2)
    assert float(ent_g) == pytest.approx(float(ent_f), rel=rtol, abs=1e-2)

    atol = 1e-5 if dtype == torch.float32 else 5e-3
    assert torch.allclose(logits_g.grad.float(), logits_f.grad.float(),
                          atol=atol, rtol=1e-2)
    assert torch.allclose(value_g.grad, value_f.grad, atol=1e-4, rtol=1e-3)


def test_fused_loss_in_agent_train_path():
    """agent.train on GPU (fused path) runs and roughly tracks a CPU agent
    with the same weights on the same batch."""
    from distributed_reinforcement_learning_amd.agents import impala
    common = dict(
        trajectory=8, input_shape=[84, 84, 4], num_action=6,
        lstm_hidden_size=16, discount_factor=0.99, start_learning_rate=1e-3,
        end_learning_rate=0.0, learning_frame=10 ** 9,
        baseline_loss_coef=1.0, entropy_coef=0.05, gradient_clip_norm=40.0,
        reward_clipping="abs_one", seed=0)
    a_gpu = impala.Agent(device="cuda:0", **common)
    a_cpu = impala.Agent(device="cpu", **common)
    # same weights (bf16-quantized on GPU)
    a_gpu.model.load_state_dict(
        {k: v for k, v in a_cpu.model.state_dict().items()})
    a_gpu.optimizer.master.copy_(
        a_cpu.optimizer.flat_params.to("cuda"))
    a_gpu.optimizer._sync_model_from_master()

    rng = np.random.default_rng(0)
    B, T, A, H = 4, 8, 6, 16
    batch = dict(
        state=rng.integers(0, 255, (B, T, 84, 84, 4), dtype=np.uint8),
        reward=rng.normal(size=(B, T)).astype(np.float32),
        action=rng.integers(0, A, (B, T)).astype(np.int32),
        done=np.zeros((B, T), dtype=bool),
        behavior_policy=np.full((B, T, A), 1 / A, dtype=np.float32),
        previous_action=rng.integers(0, A, (B, T)).astype(np.int32),
        initial_h=np.zeros((B, T, H), dtype=np.float32),
        initial_c=np.zeros((B, T, H), dtype=np.float32))
    out_gpu = a_gpu.train(**batch)
    out_cpu = a_cpu.train(**batch)
    # bf16 forward vs fp32 forward: same ballpark
    assert out_gpu[0] == pytest.approx(out_cpu[0], rel=0.1, abs=1.0)
    assert out_gpu[1] == pytest.approx(out_cpu[1], rel=0.15, abs=2.0)
    assert out_gpu[2] == pytest.approx(out_cpu[2], rel=0.05, abs=1.0)
