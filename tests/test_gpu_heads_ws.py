"""Work the heads / action-embedding forwards do for their backwards: the
heads forward zeroes the backward's atomics workspace and emits the packed
W^T, the embed forward emits W2^T, and the embed backward scatters the table
gradient in its own epilogue. Each against the launch it replaces. GPU-only."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def _make_heads(A, seed=0):
    from distributed_reinforcement_learning_amd.models.blocks import MLPHead
    torch.manual_seed(seed)
    ph = MLPHead(256, [256, 256], A, None).cuda().bfloat16()
    vh = MLPHead(256, [256, 256], 1, None).cuda().bfloat16()
    return ph, vh


def _head_tensors(ph, vh):
    weights = [ph.hidden[0].weight, ph.hidden[1].weight, ph.out.weight,
               vh.hidden[0].weight, vh.hidden[1].weight, vh.out.weight]
    biases = [ph.hidden[0].bias, ph.hidden[1].bias, ph.out.bias,
              vh.hidden[0].bias, vh.hidden[1].bias, vh.out.bias]
    return ([w.detach().contiguous() for w in weights],
            [b.detach().contiguous() for b in biases])


def _params(ph, vh):
    return [p for m in (ph, vh) for l in list(m.hidden) + [m.out]
            for p in (l.weight, l.bias)]


# 17 = MH_BM + 1: a second row tile with one live row; 37: three tiles, the
# last one partial
@pytest.mark.parametrize("N", [17, 37])
def test_forward_backward_three_times_no_leakage(N):
    """One backward per forward consumes the workspace the forward zeroed;
    three rounds on fresh inputs, each against the torch heads with the
    tolerances of tests/test_gpu_mlp_heads.py — a workspace that kept an
    earlier round's sums would miss them."""
    from distributed_reinforcement_learning_amd.ops.mlp_heads_op import (
        fused_mlp_heads,
    )
    A = 6
    ph, vh = _make_heads(A)
    ph2, vh2 = _make_heads(A)
    ph2.load_state_dict(ph.state_dict())
    vh2.load_state_dict(vh.state_dict())
    for it in range(3):
        torch.manual_seed(100 + it)
        for p in _params(ph, vh) + _params(ph2, vh2):
            p.grad = None
        h = torch.randn(N, 256, device="cuda", requires_grad=True)
        h2 = h.detach().clone().requires_grad_(True)
        dlog = torch.randn(N, A, device="cuda")
        dval = torch.randn(N, device="cuda")

        logits_f, value_f = fused_mlp_heads(h, ph, vh)
        ((logits_f.float() * dlog).sum() + (value_f * dval).sum()).backward()
        logits_t = ph2.logits(h2)
        value_t = vh2.logits(h2).squeeze(-1).float()
        ((logits_t.float() * dlog).sum() + (value_t * dval).sum()).backward()

        assert torch.allclose(h.grad, h2.grad, atol=0.05, rtol=0.05), \
            f"round {it}: dh max err {(h.grad - h2.grad).abs().max().item()}"
        for g1, g2 in zip(_params(ph, vh), _params(ph2, vh2)):
            scale = g2.grad.float().abs().mean().clamp(min=1e-4)
            rel = (g1.grad.float() - g2.grad.float()).abs().mean() / scale
            assert rel < 0.08, f"round {it}: grad rel err {rel.item():.4f}"


@pytest.mark.parametrize("N", [17, 37])
def test_forward_side_outputs(N):
    from distributed_reinforcement_learning_amd import ops
    ext = ops.require_ext()
    A = 6
    ph, vh = _make_heads(A, seed=3)
    weights, biases = _head_tensors(ph, vh)
    h = torch.randn(N, 256, device="cuda")
    ws_n = N * 256 + 4 * 256 + A + 1
    # leave NaNs where the allocator will most likely place the workspace
    poison = torch.full((ws_n,), float("nan"), device="cuda")
    del poison
    plain = ext.mlp_heads_fwd(h, weights, biases, A)
    full = ext.mlp_heads_fwd(h, weights, biases, A, want_bwd_bufs=True)
    assert len(plain) == 3 and len(full) == 5
    for a, b in zip(plain, full[:3]):
        assert torch.equal(a, b)
    ws, wt = full[3], full[4]
    assert ws.dtype == torch.float32 and ws.numel() == ws_n
    assert torch.equal(ws, torch.zeros_like(ws))
    assert torch.equal(wt, ext.mlp_heads_pack_wt(weights, A))


def test_no_grad_returns_same_outputs_without_backward_buffers():
    from distributed_reinforcement_learning_amd.ops.mlp_heads_op import (
        fused_mlp_heads,
    )
    N, A = 37, 6
    ph, vh = _make_heads(A, seed=5)
    h = torch.randn(N, 256, device="cuda", requires_grad=True)
    wt_bytes = (4 * 65536 + 256 * 32 + 256) * 2

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    (lg, vg), with_grad = peak_of(lambda: fused_mlp_heads(h, ph, vh))

    def no_grad():
        with torch.no_grad():
            return fused_mlp_heads(h, ph, vh)

    (ln, vn), without = peak_of(no_grad)
    assert torch.equal(lg, ln) and torch.equal(vg, vn)
    assert not ln.requires_grad
    # logits + value + stash are ~100 KB at this N; the packed W^T alone is
    # 541 KB
    assert with_grad >= wt_bytes
    assert without < wt_bytes


def _embed_params(A, seed):
    torch.manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, device="cuda") * 0.5).to(torch.bfloat16)
    return mk(A, 256), mk(256), mk(256, 256), mk(256)


def test_embed_forward_emits_w2_transposed():
    from distributed_reinforcement_learning_amd import ops
    ext = ops.require_ext()
    N, A = 17, 6
    table, b1, w2, b2 = _embed_params(A, seed=11)
    idx = torch.randint(0, A, (N,), device="cuda")
    plain = ext.embed_mlp_fwd(idx, table, b1, w2, b2)
    full = ext.embed_mlp_fwd(idx, table, b1, w2, b2, want_w2t=True)
    assert len(plain) == 2 and len(full) == 3
    assert torch.equal(plain[0], full[0]) and torch.equal(plain[1], full[1])
    assert torch.equal(full[2], w2.t().contiguous())


# N = 17: one full tile and a one-row tile; 163: eleven tiles. "runs" repeats
# each action over consecutive rows (what a trajectory looks like), so the
# in-block pre-sum of equal rows is exercised next to the all-distinct case.
@pytest.mark.parametrize("runs", [False, True])
@pytest.mark.parametrize("N", [17, 163])
def test_fused_scatter_matches_three_launch_path(N, runs):
    from distributed_reinforcement_learning_amd import ops
    ext = ops.require_ext()
    A = 6
    table, b1, w2, b2 = _embed_params(A, seed=13)
    if runs:
        idx = (torch.arange(N, device="cuda") // 5) % A
    else:
        idx = torch.randint(0, A, (N,), device="cuda")
    out, a1, w2t = ext.embed_mlp_fwd(idx, table, b1, w2, b2, want_w2t=True)
    dy = torch.randn(N, 256, device="cuda").to(torch.bfloat16)
    ref = ext.embed_mlp_bwd(dy, out, a1, w2, idx, A)
    got = ext.embed_mlp_bwd(dy, out, a1, w2, idx, A, w2t=w2t,
                            fuse_scatter=True)
    # dz2 and the bias grads do not depend on the scatter's placement
    assert torch.equal(got[0], ref[0])
    # table grad: the embed tolerance of tests/test_gpu_kernels.py
    assert torch.allclose(got[1].float(), ref[1].float(), atol=0.6,
                          rtol=0.05), \
        (got[1].float() - ref[1].float()).abs().max()
    for a, b in zip(got[2:], ref[2:]):
        assert torch.allclose(a.float(), b.float(), atol=0.5, rtol=0.05)
    # a second fused call: the persistent scratch was left zero
    again = ext.embed_mlp_bwd(dy, out, a1, w2, idx, A, w2t=w2t,
                              fuse_scatter=True)
    assert torch.allclose(again[1].float(), ref[1].float(), atol=0.6,
                          rtol=0.05)
