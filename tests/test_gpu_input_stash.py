"""Static inputs that a backward kernel needs are stashed by the forward
kernel that reads them (conv_op.STASH_INPUTS): the graphed IMPALA step
uploads the next batch into its static input buffers while the backward
runs, so no backward kernel may read those buffers. GPU-only."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture
def stash_on(monkeypatch):
    from distributed_reinforcement_learning_amd.ops import conv_op
    monkeypatch.setattr(conv_op, "STASH_INPUTS", True)


# ---- the three kernels -----------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lstm_tail_stashes_c_prev(stash_on, dtype):
    from distributed_reinforcement_learning_amd import ops
    from distributed_reinforcement_learning_amd.ops.lstm_op import (
        lstm_fused_step,
    )
    ext = ops.require_ext()
    torch.manual_seed(0)
    N, H = 17, 32
    gates = torch.randn(N, 4 * H, device="cuda").to(dtype)
    c0 = torch.randn(N, H, device="cuda")
    res = ext.lstm_tail_fwd(gates, c0, 1.0, stash_c=True)
    assert len(res) == 4 and torch.equal(res[3], c0)
    assert res[3].data_ptr() != c0.data_ptr()
    plain = ext.lstm_tail_fwd(gates, c0, 1.0)
    assert len(plain) == 3
    for a, b in zip(plain, res[:3]):
        assert torch.equal(a, b)

    gh = torch.randn(N, H, device="cuda")

    def run(overwrite):
        g = gates.detach().clone().requires_grad_(True)
        c = c0.clone()
        new_h, _ = lstm_fused_step(g, c, 1.0)
        if overwrite:
            c.copy_(torch.randn(N, H, device="cuda") * 3 + 1)
        new_h.backward(gh)
        return g.grad

    assert torch.equal(run(False), run(True))


def test_vtrace_loss_stashes_actions(stash_on):
    from distributed_reinforcement_learning_amd import ops
    from distributed_reinforcement_learning_amd.ops import fused_vtrace_loss
    ext = ops.require_ext()
    torch.manual_seed(1)
    B, T, A = 3, 3, 6
    logits = torch.randn(B, T, A, device="cuda") * 2
    value = torch.randn(B, T, device="cuda")
    mu = torch.softmax(torch.randn(B, T, A, device="cuda"), -1)
    actions = torch.randint(0, A, (B, T), device="cuda", dtype=torch.int32)
    rewards = torch.randn(B, T, device="cuda")
    done = torch.rand(B, T, device="cuda") < 0.1
    res = ext.vtrace_loss_fwd(logits, value, mu, actions, rewards, done,
                              0.99, 0, 0.7, 0.03, nofill=True,
                              stash_actions=True)
    assert len(res) == 5 and torch.equal(res[4], actions)
    assert res[4].data_ptr() != actions.data_ptr()

    def run(overwrite):
        lg = logits.detach().clone().requires_grad_(True)
        v = value.detach().clone().requires_grad_(True)
        a = actions.clone()
        total = fused_vtrace_loss(lg, v, mu, a, rewards, done, 0.99,
                                  "abs_one", 0.7, 0.03)[3]
        if overwrite:
            a.copy_((a + 1) % A)  # every index changes, all stay valid
        total.backward()
        return lg.grad, v.grad

    g0, g1 = run(False), run(True)
    assert torch.equal(g0[0], g1[0]) and torch.equal(g0[1], g1[1])


def test_embed_forward_stashes_indices(stash_on):
    from distributed_reinforcement_learning_amd import ops
    from distributed_reinforcement_learning_amd.ops.embed_op import (
        fused_action_embed,
    )
    ext = ops.require_ext()
    torch.manual_seed(2)
    N, A = 17, 6
    mk = lambda *s: (torch.randn(*s, device="cuda") * 0.5).to(torch.bfloat16)
    table, b1, w2, b2 = mk(A, 256), mk(256), mk(256, 256), mk(256)
    idx0 = torch.randint(0, A, (N,), device="cuda")
    res = ext.embed_mlp_fwd(idx0, table, b1, w2, b2, stash_idx=True)
    assert len(res) == 3 and torch.equal(res[2], idx0)
    assert res[2].data_ptr() != idx0.data_ptr()
    dy = torch.randn(N, 256, device="cuda").to(torch.bfloat16)

    def run(overwrite):
        t = table.detach().clone().requires_grad_(True)
        idx = idx0.clone()
        out = fused_action_embed(idx, t, b1, w2, b2)
        if overwrite:
            idx.copy_((idx + 1) % A)
        out.backward(dy)
        return t.grad

    # the embed tolerance of tests/test_gpu_kernels.py (atomics order)
    assert torch.allclose(run(False).float(), run(True).float(), atol=0.6,
                          rtol=0.05)


def test_embed_lookup_fallback_clones_for_itself(stash_on):
    """The non-fused lookup has no kernel to stash in: its wrapper clones."""
    from distributed_reinforcement_learning_amd.ops.embed_op import (
        embed_lookup,
    )
    torch.manual_seed(3)
    N, A = 17, 6
    table = torch.randn(A, 64, device="cuda")
    idx0 = torch.randint(0, A, (N,), device="cuda")
    go = torch.randn(N, 64, device="cuda")

    def run(overwrite):
        t = table.detach().clone().requires_grad_(True)
        idx = idx0.clone()
        out = embed_lookup(t, idx)
        if overwrite:
            idx.copy_((idx + 1) % A)
        out.backward(go)
        return t.grad

    assert torch.allclose(run(False), run(True), atol=1e-5, rtol=1e-5)


# ---- the graphed step ------------------------------------------------------

def _agent(A, H, T, seed=0):
    from distributed_reinforcement_learning_amd.agents import impala
    return impala.Agent(
        trajectory=T, input_shape=[84, 84, 4], num_action=A,
        lstm_hidden_size=H, discount_factor=0.99, start_learning_rate=1e-3,
        end_learning_rate=0.0, learning_frame=10 ** 9,
        baseline_loss_coef=1.0, entropy_coef=0.05, gradient_clip_norm=40.0,
        reward_clipping="abs_one", device="cuda:0", seed=seed)


def _batch(B, T, A, H, seed, shift=0):
    """shift moves EVERY action / previous_action index (mod A)."""
    rng = np.random.default_rng(seed)
    base = np.random.default_rng(1234)
    act = base.integers(0, A, (B, T))
    pact = base.integers(0, A, (B, T))
    return dict(
        state=rng.integers(0, 255, (B, T, 84, 84, 4), dtype=np.uint8),
        reward=rng.normal(size=(B, T)).astype(np.float32),
        action=((act + shift) % A).astype(np.int32),
        done=np.zeros((B, T), dtype=bool),
        behavior_policy=np.full((B, T, A), 1 / A, dtype=np.float32),
        previous_action=((pact + shift) % A).astype(np.int64),
        initial_h=(rng.normal(size=(B, T, H)) * 0.1).astype(np.float32),
        initial_c=(rng.normal(size=(B, T, H)) * 0.1).astype(np.float32),
    )


def _saved_tensors(node):
    out = []
    if hasattr(node, "saved_tensors"):       # python autograd.Function
        out.extend(t for t in node.saved_tensors if t is not None)
    for name in dir(node):
        if not name.startswith("_saved_"):
            continue
        try:
            v = getattr(node, name)
        except RuntimeError:                  # released buffer
            continue
        vs = v if isinstance(v, (list, tuple)) else [v]
        out.extend(t for t in vs if isinstance(t, torch.Tensor))
    return out


# (A, H, B, T): the tests/test_gpu_graph.py shape, and one that takes the
# fused heads path (H = 256) at the flagship action count
@pytest.mark.parametrize("A,H,B,T", [(6, 32, 4, 8), (18, 256, 2, 3)])
def test_no_saved_tensor_aliases_a_static_input(A, H, B, T):
    from distributed_reinforcement_learning_amd.runtime import (
        GraphedImpalaStep,
    )
    graphed = GraphedImpalaStep(_agent(A, H, T), batch_size=B)
    inputs = {t.untyped_storage().data_ptr(): k
              for k, t in graphed.inputs.items()}
    seen, stack, n_saved = set(), [graphed._total.grad_fn], 0
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        for t in _saved_tensors(node):
            n_saved += 1
            if not t.is_cuda:
                continue
            ptr = t.untyped_storage().data_ptr()
            assert ptr not in inputs, (
                f"{type(node).__name__} saved a tensor that shares storage "
                f"with static input {inputs.get(ptr)!r}")
        stack.extend(fn for fn, _ in node.next_functions)
    assert len(seen) > 10 and n_saved > 10  # the walk saw the real graph


def test_pipelined_steps_match_synchronous_steps():
    """step(pinned_src=...) replays on the batch uploaded during the
    PREVIOUS step's backward: over X, Y, Z it consumes X, X, Y. A twin
    agent fed exactly that sequence synchronously must end up in the same
    place; a backward that read a static input the upload had already
    rewritten (Y's or Z's indices) would not."""
    from distributed_reinforcement_learning_amd.runtime import (
        GraphedImpalaStep,
    )
    A, H, B, T = 6, 32, 4, 8
    a_pipe, a_sync = _agent(A, H, T), _agent(A, H, T)
    a_sync.model.load_state_dict(a_pipe.model.state_dict())
    a_sync.optimizer.flat_params.copy_(a_pipe.optimizer.flat_params)
    g_pipe = GraphedImpalaStep(a_pipe, batch_size=B)
    g_sync = GraphedImpalaStep(a_sync, batch_size=B)
    assert torch.equal(a_pipe.optimizer.flat_params,
                       a_sync.optimizer.flat_params)

    X, Y, Z = (_batch(B, T, A, H, seed=s, shift=s) for s in (0, 1, 2))
    for k in ("action", "previous_action"):
        assert (X[k] != Y[k]).all() and (Y[k] != Z[k]).all()
        assert (X[k] != Z[k]).all()

    def pinned(b):
        return {k: torch.as_tensor(np.asarray(b[k])).to(v.dtype).pin_memory()
                for k, v in g_pipe.pinned.items()}

    staged = [pinned(b) for b in (X, Y, Z)]  # alive until the last upload
    for src, consumed in [(staged[0], X), (staged[1], X), (staged[2], Y)]:
        g_pipe.step(pinned_src=src)
        out_p = g_pipe.last_losses()
        g_sync.step(batch=consumed)
        out_s = g_sync.last_losses()
        # the tolerance of test_graphed_step_matches_eager
        for i in range(3):
            assert out_p[i] == pytest.approx(out_s[i], rel=5e-2, abs=5e-1)
        assert out_p[3] == out_s[3]
    g_pipe.wait_pinned_free()
    torch.cuda.synchronize()
    assert torch.allclose(a_pipe.optimizer.flat_params,
                          a_sync.optimizer.flat_params, atol=1e-2)
