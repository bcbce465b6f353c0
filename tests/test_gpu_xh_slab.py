"""Gate-GEMM input assembled in place: conv layer 3 and the action-embedding
forward store straight into one [N, 3136 + 256 + H + 8] bf16 slab (the embed
kernel also drops bf16(h) and the ones-pad in), replacing torch.cat and the
h cast. Every piece against today's contiguous call. GPU-only."""

import pytest
import torch

pytestmark = pytest.mark.gpu

N_CONV, N_EMB, PAD = 3136, 256, 8
SENTINEL = -7.0  # exactly representable in bf16; ReLU outputs are >= 0


@pytest.fixture(scope="module")
def ext():
    from distributed_reinforcement_learning_amd import ops
    assert ops.available()
    return ops.require_ext()


def _rel_mean_err(got, ref, floor):
    return ((got.float() - ref.float()).abs().mean()
            / ref.float().abs().mean().clamp(min=floor)).item()


def _conv3_inputs(N, seed=0):
    torch.manual_seed(seed)
    x = torch.randn(N, 9, 9, 64, device="cuda").bfloat16() * 0.5
    w = (torch.randn(64, 3 * 3 * 64, device="cuda") * 0.05).bfloat16()
    b = (torch.randn(64, device="cuda") * 0.1).bfloat16()
    return x, w, b


def test_conv_l3_into_slab_and_strided_mask_backward(ext):
    """N = 3: M = 147 rows cross the 128-row tile."""
    N, H = 3, 32
    R = N_CONV + N_EMB + H + PAD
    x, w, b = _conv3_inputs(N)
    y_ref, _ = ext.conv_fwd(3, x, w, b, False)
    slab = torch.full((N, R), SENTINEL, device="cuda", dtype=torch.bfloat16)
    y, _ = ext.conv_fwd(3, x, w, b, False, slab)
    assert y.shape == (N, 7, 7, 64) and y.stride() == (R, 448, 64, 1)
    assert y.data_ptr() == slab.data_ptr()
    assert torch.equal(slab[:, :N_CONV], y_ref.reshape(N, -1))
    assert torch.equal(y, y_ref)
    assert (slab[:, N_CONV:] == SENTINEL).all()

    # relu_mask_bwd with the strided y, then the wgrad that finalizes dbias
    dy = torch.randn(N, 7, 7, 64, device="cuda").bfloat16()
    m_ref = ext.relu_mask_bwd(dy, y_ref, 64, 3)
    _, dbias_ref = ext.conv_wgrad(3, x, m_ref)
    m = ext.relu_mask_bwd(dy, y, 64, 3)
    _, dbias = ext.conv_wgrad(3, x, m)
    assert torch.equal(m, m_ref)
    # unordered f32 atomics: the bias-grad bound of tests/test_gpu_conv.py
    assert _rel_mean_err(dbias, dbias_ref, 1e-4) < 0.12
    # both operands strided (dy a slice of a wider gradient, as in the step)
    dxh = torch.zeros(N, R, device="cuda", dtype=torch.bfloat16)
    dxh[:, :N_CONV] = dy.reshape(N, -1)
    m2 = ext.relu_mask_bwd(dxh[:, :N_CONV].view(N, 7, 7, 64), y, 64, 3)
    ext.conv_wgrad(3, x, m2)  # drains the bias-grad slots again
    assert torch.equal(m2, m_ref)


def _embed_params(A, seed):
    torch.manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, device="cuda") * 0.5).to(torch.bfloat16)
    return mk(A, 256), mk(256), mk(256, 256), mk(256)


# N = 17 = MH_BM + 1: a second row tile with one live row. H = 32 is one
# partial sweep of the h-convert loop, H = 256 two full ones.
@pytest.mark.parametrize("H", [32, 256])
def test_embed_forward_into_slab(ext, H):
    N, A = 17, 6
    R = N_CONV + N_EMB + H + PAD
    table, b1, w2, b2 = _embed_params(A, seed=H)
    idx = torch.randint(0, A, (N,), device="cuda")
    h = torch.randn(N, H, device="cuda") * 3
    out_ref, a1_ref = ext.embed_mlp_fwd(idx, table, b1, w2, b2)
    # two guard rows behind the slab catch a store past row N
    buf = torch.full((N + 2, R), SENTINEL, device="cuda",
                     dtype=torch.bfloat16)
    slab = buf[:N]
    out, a1 = ext.embed_mlp_fwd(idx, table, b1, w2, b2, xh_slab=slab,
                                emb_col=N_CONV, h=h)
    assert out.shape == (N, 256) and out.stride() == (R, 1)
    assert out.data_ptr() == slab[:, N_CONV:].data_ptr()
    assert torch.equal(a1, a1_ref)
    assert torch.equal(slab[:, N_CONV:N_CONV + 256], out_ref)
    assert torch.equal(slab[:, N_CONV + 256:N_CONV + 256 + H],
                       h.to(torch.bfloat16))
    pad = slab[:, N_CONV + 256 + H:]
    assert pad.shape == (N, PAD)
    assert (pad[:, 0] == 1).all() and (pad[:, 1:] == 0).all()
    assert (slab[:, :N_CONV] == SENTINEL).all()
    assert (buf[N:] == SENTINEL).all()

    # backward reading the ReLU-2 mask from the slab
    dy = torch.randn(N, 256, device="cuda").to(torch.bfloat16)
    ref = ext.embed_mlp_bwd(dy, out_ref, a1_ref, w2, idx, A)
    got = ext.embed_mlp_bwd(dy, out, a1, w2, idx, A)
    assert torch.equal(got[0], ref[0])
    for a, b in zip(got[1:], ref[1:]):
        assert torch.allclose(a.float(), b.float(), atol=0.5, rtol=0.05)


def _agent(H, A, T):
    from distributed_reinforcement_learning_amd.agents import impala
    return impala.Agent(
        trajectory=T, input_shape=[84, 84, 4], num_action=A,
        lstm_hidden_size=H, discount_factor=0.99, start_learning_rate=1e-3,
        end_learning_rate=0.0, learning_frame=10 ** 9,
        baseline_loss_coef=1.0, entropy_coef=0.05, gradient_clip_norm=40.0,
        reward_clipping="abs_one", device="cuda:0", seed=0)


def test_unroll_features_slab_path_matches_cat_path():
    B, T, A, H = 2, 3, 6, 32
    model = _agent(H, A, T).model
    torch.manual_seed(5)
    state = torch.randint(0, 256, (B, T, 84, 84, 4), dtype=torch.uint8,
                          device="cuda")
    pa = torch.randint(0, A, (B, T), device="cuda")
    h0 = torch.randn(B, T, H, device="cuda") * 0.5
    c0 = torch.randn(B, T, H, device="cuda") * 0.5
    g = torch.randn(B * T, H, device="cuda")
    flat = state.reshape(B * T, 84, 84, 4)
    assert model._xh_slab_ok(flat, h0.reshape(B * T, H)), \
        "the seeded agent must select the slab path"

    def run(use_slab):
        model.USE_XH_SLAB = use_slab
        for p in model.parameters():
            p.grad = None
        new_h, _, _ = model._unroll_features(state, pa, h0, c0)
        new_h.backward(g)
        return new_h.detach().clone(), {
            n: p.grad.detach().clone() for n, p in model.named_parameters()
            if p.grad is not None}

    try:
        h_cat, g_cat = run(False)
        h_slab, g_slab = run(True)
    finally:
        model.USE_XH_SLAB = True
    # same xh bits into the same GEMM
    assert torch.equal(h_slab, h_cat)
    assert g_cat.keys() == g_slab.keys() and len(g_cat) >= 10
    for name, ref in g_cat.items():
        got = g_slab[name]
        if name == "action_emb.table":
            # tests/test_gpu_kernels.py embed tolerance
            assert torch.allclose(got.float(), ref.float(), atol=0.6,
                                  rtol=0.05), name
        elif name.endswith("bias") or name.endswith("bias1"):
            # tests/test_gpu_conv.py: 0.12 bias grad, 0.08 weight grad (the
            # heads test asks 0.08 of both)
            assert _rel_mean_err(got, ref, 1e-4) < 0.12, name
        else:
            assert _rel_mean_err(got, ref, 1e-4) < 0.08, name
